"""nn.CGConv on the device: the recorded reference cases with their launch counts, the kernels of
csrc/cg.hip against the float64 restatement (tests/_cg_ref.py, the UNSPLIT ``cat`` then ``Linear``
form) run on the device, an exact test with every pre-activation at 0, saturated activations,
empty rows, long rows through the chunked schedule, bitwise repeatability, the memory promise,
routing, half inputs, HeteroConv and the registered operators.  Nothing here reads the reference
tree.

Figures measured on one gfx950 device are in profiles/cg_conv.md."""
import math

import numpy as np
import pytest
import torch

import _cg_ref as R
import test_gpu_transformer as T
from _util import assert_close, assert_close_scaled, gen, random_graph

pytestmark = pytest.mark.gpu

NAMES = ('out', 'grad_p', 'grad_q', 'grad_edge', 'grad_Wf', 'grad_Ws', 'grad_residual')
TOL = 2e-5
FUSED = ('pygamd_cg_forward', 'pygamd_cg_backward_dst', 'pygamd_cg_backward_src')


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_the_device(dev, monkeypatch, name, index_dtype):
    """A fused case: ONE forward and ONE launch per backward direction and nothing else that
    touches the edges.  ``max``: the generic route, no cg call."""
    c = T._counted(monkeypatch, lambda: R.check_class_case(R.load_golden(), name, dev,
                                                           index_dtype=index_dtype))
    if name in R.FUSED_CASES:
        for fn in FUSED:
            assert c.calls.get(fn) == 1, c.calls
        assert not [n for n in c.calls if 'spmm' in n or 'scatter' in n or 'softmax' in n], c.calls
    else:
        assert not [n for n in c.calls if 'pygamd_cg_' in n], c.calls


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
def test_golden_stack_on_the_device(dev, monkeypatch, index_dtype):
    c = T._counted(monkeypatch, lambda: R.check_stack(R.load_golden(), dev,
                                                      index_dtype=index_dtype))
    for fn in FUSED:
        assert c.calls.get(fn) == 2, c.calls


# ---- problems ---------------------------------------------------------------------------------------
def _problem(n_src, n_dst, ei, F, De, seed, wide=False, p_rows=None):
    """random normal P [p_rows or n_dst, 2F], Q [n_src, 2F], residual [n_dst, F], grad_out; with
    ``De``: raw edge features and the edge columns of the two ``Linear`` (the pre-activations have
    a standard deviation of about 1.7); ``wide``: the dense edge terms ``a @ [Wf_e ; Ws_e]^T``
    rounded to float32 instead, the kernels' input in that mode"""
    g = gen(seed)
    E = ei.size(1)
    P = {'ei': ei, 'n_src': n_src, 'n_dst': n_dst, 'F': F, 'De': De, 'wide': wide,
         'p': torch.randn(p_rows or n_dst, 2 * F, generator=g),
         'q': torch.randn(n_src, 2 * F, generator=g), 'res': torch.randn(n_dst, F, generator=g),
         'go': torch.randn(n_dst, F, generator=g), 'a': None, 'wf': None, 'ws': None,
         'terms': None}
    if De:
        a = torch.randn(E, De, generator=g)
        wf, ws = [torch.randn(F, De, generator=g) / De ** 0.5 for _ in range(2)]
        if wide:
            P['terms'] = (a.double() @ torch.cat([wf, ws]).double().t()).float()
        else:
            P.update(a=a, wf=wf, ws=ws)
    return P


def _reference(P, mean=False, residual=False, dtype=torch.float64, device='cuda'):
    """the seven of NAMES from the restatement run on ``device`` (None where an input is absent),
    as CPU tensors.  ``x_dst`` is P and ``x_src`` is Q, rows of 2F, and each ``Linear`` reads
    ``cat([P_i, Q_j, e])`` with the weight ``[S | S | W_e]``, S the selector of its half of a row
    (exact), so the edge columns are used UNSPLIT; the dense edge terms are edge features whose
    edge columns are that selector too."""
    F, n_dst = P['F'], P['n_dst']
    p, q, res = [P[n].to(device, dtype).requires_grad_(True) for n in ('p', 'q', 'res')]
    a, wf, ws, terms = [None if P[n] is None else P[n].to(device, dtype).requires_grad_(True)
                        for n in ('a', 'wf', 'ws', 'terms')]
    eye, zero = torch.eye(F, dtype=dtype, device=device), torch.zeros(F, F, dtype=dtype,
                                                                        device=device)
    sel_f, sel_s = torch.cat([eye, zero], dim=1), torch.cat([zero, eye], dim=1)
    edge = a if terms is None else terms
    cols_f = [sel_f, sel_f] + ([] if edge is None else [wf if terms is None else sel_f])
    cols_s = [sel_s, sel_s] + ([] if edge is None else [ws if terms is None else sel_s])
    out = R.cg_aggregate(q, p[:n_dst], edge, (torch.cat(cols_f, dim=1), None),
                         (torch.cat(cols_s, dim=1), None), P['ei'].to(device), n_dst,
                         aggr='mean' if mean else 'add', residual=False)
    if residual:
        out = out + res
    slots = [p, q, edge, wf, ws, res if residual else None]
    leaves = [t for t in slots if t is not None]
    grads = dict(zip([id(t) for t in leaves],
                     torch.autograd.grad(out, leaves, P['go'].to(device, dtype),
                                         allow_unused=True)))
    got = [out] + [None if t is None else grads[id(t)] for t in slots]
    got = [None if t is None else t.detach().cpu() for t in got]
    for i, t in enumerate(slots):    # (no edge anywhere: autograd reports "unused")
        if t is not None and got[i + 1] is None:
            got[i + 1] = torch.zeros(t.shape, dtype=dtype)
    return got


def _device_run(P, dev, index_dtype=torch.int64, edge_grad=True, packed=False, mean=False,
                residual=False):
    """the same seven through the autograd node, and the handle.  ``packed``: P and Q are the
    halves of one [N, 4F] plane and the gradient is ONE plane of that shape"""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import CGAggregateFunction
    F = P['F']
    if packed:
        assert P['p'].size(0) == P['n_src']
        p = torch.cat([P['p'], P['q']], dim=1).to(dev).requires_grad_(True)
        q = None
    else:
        p, q = P['p'].to(dev).requires_grad_(True), P['q'].to(dev).requires_grad_(True)
    a = wf = ws = terms = res = None
    if P['a'] is not None:
        a = P['a'].to(dev).requires_grad_(edge_grad)
        wf, ws = P['wf'].to(dev).requires_grad_(True), P['ws'].to(dev).requires_grad_(True)
    if P['terms'] is not None:
        terms = P['terms'].to(dev).requires_grad_(edge_grad)
    if residual:
        res = P['res'].to(dev).requires_grad_(True)
    graph = P.get('graph')
    if graph is None or graph.edge_index.dtype != index_dtype:
        graph = as_edge_index(P['ei'].to(dev).to(index_dtype), P['n_src'], P['n_dst'])
    out = CGAggregateFunction.apply(p, q, a, wf, ws, terms, res, graph, P['n_dst'], mean)
    slots = [p, q, a if terms is None else terms, wf, ws, res]
    leaves = [t for t in slots if t is not None and t.requires_grad]
    grads = dict(zip([id(t) for t in leaves], torch.autograd.grad(out, leaves, P['go'].to(dev))))
    got = [out.detach()] + [None if t is None else grads.get(id(t)) for t in slots]
    if packed:
        plane = got[1]
        assert plane.shape == (P['n_src'], 4 * F) and plane.is_contiguous()
        got[1], got[2] = plane[:, :2 * F], plane[:, 2 * F:]
    return got, graph


def _check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, f'{what}: {name} should be absent'
            continue
        assert g is not None, f'{what}: {name} is missing'
        assert_close_scaled(g, w.float(), tol=TOL, what=f'{what} {name}')


# ---- the kernels against float64 ------------------------------------------------------------------
_UNIFORM = {}


def _uniform_case(F, De, wide=False):
    """problem and float64 results at one shape, computed once for both index dtypes"""
    key = (F, De, wide)
    if key not in _UNIFORM:
        P = _problem(2000, 2000, T._uniform_graph(), F, De, 400 + F + 7 * De, wide=wide)
        P['want'] = {(False, False): _reference(P), (True, True): _reference(P, True, True)}
        _UNIFORM[key] = P
    return _UNIFORM[key]


NONE_SHAPES = [(F, 0, False) for F in (1, 5, 24, 64, 100, 128, 132, 256, 512)]
LINEAR_SHAPES = [(F, De, False) for F, De in (
    (8, 1), (24, 3), (64, 7), (128, 16), (256, 8), (512, 4), (64, 32), (400, 5), (292, 7),
    (290, 7), (200, 10), (136, 15), (130, 15), (100, 20))]
WIDE_SHAPES = [(64, 41, True), (132, 5, True)]


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('F,De,wide', NONE_SHAPES + LINEAR_SHAPES + WIDE_SHAPES)
def test_kernels_match_float64(dev, F, De, wide, index_dtype):
    """F below one lane group, odd, the float4 widths and the limit; the raw-feature mode at (F,
    De) through the register capacities for De and the corners of its envelope ((128, 16), (256,
    8), (512, 4), (64, 32): 32 registers per edge matrix), then the shapes whose sizes round up to
    the lane shapes of 64 registers per matrix, on both sides of the float4 / scalar boundary:
    (EPL, DE) = (8, 8) as float4 units ((400, 5), (292, 7)) and scalar ((290, 7)), (4, 16) as
    float4 units ((200, 10), (136, 15)) and scalar ((130, 15)), (2, 32) ((100, 20)); the dense
    edge terms at CGCNN's (64, 41) and at (132, 5).  Contiguous P and Q with the sum and no
    residual, then the halves of one [N, 4F] plane, whose gradient is one plane, with the mean and
    the residual."""
    P = _uniform_case(F, De, wide)
    got, graph = _device_run(P, dev, index_dtype=index_dtype)
    P['graph'] = graph
    _check(got, P['want'][(False, False)], f'({F}, {De})')
    got, _ = _device_run(P, dev, index_dtype=index_dtype, packed=True, mean=True, residual=True)
    _check(got, P['want'][(True, True)], f'({F}, {De}) packed, mean, residual')


@pytest.mark.parametrize('F,De,wide', [(24, 3, False), (132, 0, False), (24, 41, True),
                                       (292, 7, False), (100, 20, False)])
def test_the_other_pairings_of_layout_and_epilogue(dev, F, De, wide):
    """contiguous with the mean and the residual, packed with the sum and no residual, and each of
    the mean and the residual alone; (292, 7) and (100, 20) hold 64 registers per edge matrix"""
    P = _uniform_case(F, De, wide)
    got, graph = _device_run(P, dev, mean=True, residual=True)
    P['graph'] = graph
    _check(got, P['want'][(True, True)], f'({F}, {De}) contiguous, mean, residual')
    got, _ = _device_run(P, dev, packed=True)
    _check(got, P['want'][(False, False)], f'({F}, {De}) packed')
    for mean, residual in ((True, False), (False, True)):
        got, _ = _device_run(P, dev, mean=mean, residual=residual)
        _check(got, _reference(P, mean, residual), f'({F}, {De}) mean {mean} residual {residual}')


@pytest.mark.parametrize('F,De,wide', [(24, 0, False), (24, 3, False), (132, 5, False),
                                       (24, 41, True)])
def test_destinations_a_prefix_empty_rows_and_no_edges(dev, F, De, wide):
    """300 destinations, a prefix of 900 sources whose P has 900 rows; a destination without slots
    gets exactly its residual (or exactly 0) under the sum and under the mean, sources without
    slots (and the rows of P beyond the destinations) zero gradients; a graph without edges."""
    ei = random_graph(900, 300, 5000, 43)
    ei = ei[:, (ei[1] % 7 != 0) & (ei[0] % 5 != 0)]
    P = _problem(900, 300, ei, F, De, 11, wide=wide, p_rows=900)
    empty_dst = torch.bincount(ei[1], minlength=300) == 0
    empty_src = torch.bincount(ei[0], minlength=900) == 0
    assert int(empty_dst.sum()) >= 40 and int(empty_src.sum()) >= 180
    for packed, mean, residual in ((False, False, False), (True, True, True),
                                   (False, True, False), (True, False, True)):
        got, _ = _device_run(P, dev, packed=packed, mean=mean, residual=residual)
        _check(got, _reference(P, mean, residual), f'prefix ({F}, {De}) {packed} {mean} {residual}')
        assert got[0].shape == (300, F) and got[1].shape == (900, 2 * F)
        assert got[2].shape == (900, 2 * F)
        rows = got[0].cpu()[empty_dst]
        if residual:
            assert torch.equal(rows, P['res'][empty_dst])              # exactly the residual
            assert torch.equal(got[6].cpu(), P['go'])                  # its gradient: grad_out
        else:
            assert float(rows.abs().max()) == 0.0                      # exact zeros
        assert float(got[1].cpu()[:300][empty_dst].abs().max()) == 0.0
        assert float(got[1][300:].abs().max()) == 0.0
        assert float(got[2].cpu()[empty_src].abs().max()) == 0.0
    Z = _problem(50, 40, torch.zeros(2, 0, dtype=torch.int64), F, De, 12, wide=wide)
    for mean, residual in ((False, False), (True, True)):
        got, _ = _device_run(Z, dev, mean=mean, residual=residual)
        assert got[0].shape == (40, F)
        assert torch.equal(got[0].cpu(), Z['res'] if residual else torch.zeros(40, F))
        assert all(float(g.abs().max()) == 0.0 for g in got[1:3])
        assert got[1].shape == (40, 2 * F) and got[2].shape == (50, 2 * F)
        if De:
            assert got[3].shape == (0, 2 * F if wide else De)
        if De and not wide:
            assert float(got[4].abs().max()) == 0.0 and float(got[5].abs().max()) == 0.0


# ---- exact: every pre-activation at 0 --------------------------------------------------------------
def test_messages_of_half_ln_two_are_exact(dev):
    """P = Q = 0 without an edge term: zf = zs = 0, the sigmoid is exactly 0.5 and the softplus
    log1pf(1) = ln 2 in float32, so every message is m = 0.5 * fl(ln 2), exactly.  Destination i
    has i % 65 slots; a wave adds its slots in order, so the sum is m added ``deg`` times in
    float32 and the mean that sum divided once: bit for bit."""
    n, F = 195, 24
    deg = torch.arange(n) % 65
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (dst.numel(), ), generator=gen(61))
    perm = torch.randperm(dst.numel(), generator=gen(62))
    ei = torch.stack([src, dst])[:, perm].contiguous()
    P = _problem(n, n, ei, F, 0, 63)
    P['p'], P['q'] = torch.zeros(n, 2 * F), torch.zeros(n, 2 * F)
    m = np.float32(0.5) * np.float32(math.log(2.0))
    sums = np.zeros(65, dtype=np.float32)
    for k in range(1, 65):
        sums[k] = np.float32(sums[k - 1] + m)
    want_sum = torch.from_numpy(sums)[deg].view(n, 1).expand(n, F)
    want_mean = torch.from_numpy(sums / np.maximum(np.arange(65), 1).astype(np.float32))[deg]
    for packed in (False, True):
        got, _ = _device_run(P, dev, packed=packed)
        assert torch.equal(got[0].cpu(), want_sum), 'sum is not exact'
        got, _ = _device_run(P, dev, packed=packed, mean=True)
        assert torch.equal(got[0].cpu(), want_mean.view(n, 1).expand(n, F)), 'mean is not exact'
        got, _ = _device_run(P, dev, packed=packed, residual=True)
        assert torch.equal(got[0].cpu(), want_sum + P['res']), 'sum + residual is not exact'


# ---- saturated activations ---------------------------------------------------------------------------
def test_saturated_activations(dev):
    """zf in +-100, +-30 and zs in +-100, -25, 19.5, 20.5 per (row, column), Q = 0: outputs and
    gradients are finite and match float64.  Beyond the range of expf the gate is exactly 0 or 1:
    zf = -100 gives an output of exactly 0 and, with zs = 100 (past the softplus threshold, where
    it is z itself), zf = +100 gives exactly 100 per slot."""
    n, F = 2000, 24
    P = _problem(n, n, T._uniform_graph(), F, 0, 71)
    g = gen(72)
    zf = torch.tensor([-100., 100., -30., 30.])[torch.randint(0, 4, (n, F), generator=g)]
    zs = torch.tensor([-100., 100., -25., 19.5, 20.5])[torch.randint(0, 5, (n, F), generator=g)]
    P['p'], P['q'] = torch.cat([zf, zs], dim=1), torch.zeros(n, 2 * F)
    want = _reference(P)
    for packed in (False, True):
        got, _ = _device_run(P, dev, packed=packed)
        assert all(bool(torch.isfinite(t).all()) for t in got[:3])
        _check(got, want, 'saturated')
        out = got[0].cpu()
        deg = torch.bincount(P['ei'][1], minlength=n).float().view(n, 1).expand(n, F)
        assert float(out[zf == -100].abs().max()) == 0.0
        one = (zf == 100) & (zs == 100)
        assert int(one.sum()) > 1000 and torch.equal(out[one], 100 * deg[one])
        # the gate's own gradient is exactly 0 where it is exactly 0 or 1
        assert float(got[1].cpu()[:, :F][zf.abs() == 100].abs().max()) == 0.0
    # both sides of the threshold, through the edge term too
    L = _problem(n, n, T._uniform_graph(), 24, 3, 73)
    L['p'][:, 24:] += 20.0
    got, _ = _device_run(L, dev)
    _check(got, _reference(L), 'around the softplus threshold')
    zs_all = (L['p'][L['ei'][1], 24:] + L['q'][L['ei'][0], 24:] + L['a'] @ L['ws'].t())
    assert int((zs_all > 20).sum()) > 1000 and int((zs_all < 20).sum()) > 1000


# ---- long rows ------------------------------------------------------------------------------------
THRESHOLD, CHUNK = 512, 128
_LONG = {}


def _long_case(De, wide=False):
    """N = 1500: destination 5 has 700 slots, destination 11 exactly THRESHOLD + 1, source 7 has
    650 out-slots; the rest is uniform.  F = 64, random normal inputs"""
    key = (De, wide)
    if key not in _LONG:
        g = gen(51)
        n = 1500
        src = torch.cat([torch.randint(0, n, (8000 + 700 + THRESHOLD + 1, ), generator=g),
                         torch.full((650, ), 7)])
        base = torch.randint(0, n, (8000, ), generator=g)
        base[(base == 5) | (base == 11)] = 12
        dst = torch.cat([base, torch.full((700, ), 5), torch.full((THRESHOLD + 1, ), 11),
                         torch.randint(12, n, (650, ), generator=g)])
        perm = torch.randperm(src.numel(), generator=g)
        P = _problem(n, n, torch.stack([src, dst])[:, perm].contiguous(), 64, De, 57 + De,
                     wide=wide)
        P['want'] = {False: _reference(P), True: _reference(P, True, True)}
        _LONG[key] = P
    return _LONG[key]


def _lower_the_threshold(monkeypatch):
    """the package's hub threshold and chunk until the test ends (handles made after this)"""
    from pytorch_geometric_amd import _native
    monkeypatch.setattr(_native, 'HUB_THRESHOLD', THRESHOLD)
    monkeypatch.setattr(_native, 'HUB_CHUNK', CHUNK)
    return _native


@pytest.mark.parametrize('De,wide', [(0, False), (6, False), (41, True)])
def test_long_rows_match_float64_and_are_chunked(dev, monkeypatch, De, wide):
    """Rows past the (lowered) threshold are split into chunks whose partials are merged in chunk
    order; the epilogue runs once after the merge: the mean divides once, the residual is added
    once."""
    native = _lower_the_threshold(monkeypatch)
    P = dict(_long_case(De, wide), graph=None)
    for mean in (False, True):
        sink = []
        monkeypatch.setattr(native, 'timing_sink', sink)
        got, graph = _device_run(P, dev, mean=mean, residual=mean, packed=mean)
        torch.cuda.synchronize()
        monkeypatch.setattr(native, 'timing_sink', None)
        P['graph'] = graph
        ptr = graph.by_dst().ptr
        assert int(ptr[6] - ptr[5]) == 700 and int(ptr[12] - ptr[11]) == THRESHOLD + 1
        _check(got, P['want'][mean], f'long rows De = {De}, mean {mean}')
        info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'cg'}
        assert set(info) == {'forward', 'backward_dst', 'backward_src'}
        want = -(-700 // CHUNK) + -(-(THRESHOLD + 1) // CHUNK)
        for op in ('forward', 'backward_dst'):
            assert info[op]['n_hub'] == 2 and info[op]['n_chunks'] == want
        assert info['backward_src']['n_hub'] == 1                       # source 7
        assert info['backward_src']['n_chunks'] >= -(-650 // CHUNK)
        for rec in info.values():
            assert rec['F'] == 64 and rec['De'] == (0 if wide else De)
        assert info['backward_dst']['grad_edge_attr'] is (De > 0)


@pytest.mark.parametrize('De,wide', [(0, False), (6, False), (41, True)])
def test_two_runs_are_bitwise_identical(dev, monkeypatch, De, wide):
    """No float atomics anywhere and grids that depend on the problem only: every output and
    gradient, grad_Wf and grad_Ws from the per-workgroup partials included, repeats bit for bit on
    random inputs, long rows included."""
    _lower_the_threshold(monkeypatch)
    P = dict(_long_case(De, wide), graph=None)
    for kw in (dict(), dict(mean=True, residual=True, packed=True)):
        a, graph = _device_run(P, dev, **kw)
        P['graph'] = graph
        b, _ = _device_run(P, dev, **kw)
        for name, x, y in zip(NAMES, a, b):
            assert (x is None) == (y is None)
            if x is not None:
                assert torch.equal(x, y), f'De = {De}: {name} differs between two runs'
    if De and not wide:
        for shape in ((64, 7), (292, 7), (130, 15), (100, 20)):   # the last three: 64 registers each
            U = _uniform_case(*shape)
            a, _ = _device_run(U, dev)
            b, _ = _device_run(U, dev)
            assert all(torch.equal(x, y) for x, y in zip(a, b) if x is not None), shape


# ---- edge_attr without a gradient -----------------------------------------------------------------------
def test_without_a_gradient_for_edge_attr(dev, monkeypatch):
    from pytorch_geometric_amd import _native
    for P in (_uniform_case(64, 7), _uniform_case(200, 10), _uniform_case(290, 7),
              _uniform_case(64, 41, True)):
        full, _ = _device_run(P, dev)
        sink = []
        monkeypatch.setattr(_native, 'timing_sink', sink)
        lean, _ = _device_run(P, dev, edge_grad=False)
        torch.cuda.synchronize()
        monkeypatch.undo()
        rec = [i for i, _, _ in sink if i.get('kind') == 'cg' and i['op'] == 'backward_dst']
        assert len(rec) == 1 and rec[0]['grad_edge_attr'] is False
        assert lean[3] is None and full[3] is not None
        for name, x, y in zip(NAMES, lean, full):
            if name != 'grad_edge' and y is not None:
                assert torch.equal(x, y), f'{name} differs without the edge gradient'


# ---- nothing of size E x F (the dense edge terms: one E x 2F plane and its gradient) -----------------
@pytest.mark.parametrize('mode', ['linear', 'none', 'wide'])
def test_keeps_nothing_of_edge_times_width(dev, mode):
    """Above the inputs, over forward + backward.  Without an edge term and with raw features: out
    (2 MiB), the [N, 4F] gradient plane (8 MiB), grad_edge_attr (8 MiB), the stacked edge matrices
    and the per-workgroup partials (4 MiB) — below ONE [E, F] plane, which is 128 MiB here.  With
    the dense edge terms (an input of 2 planes) the backward writes their gradient, 2 planes, and
    nothing else per edge: below three."""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import CGAggregateFunction
    N, E, F, De = 4096, 262144, 128, 8
    graph = as_edge_index(random_graph(N, N, E, 71).to(dev), N, N)
    graph.fill_cache_()
    g = gen(72)
    pq = torch.randn(N, 4 * F, generator=g).to(dev).requires_grad_(True)
    res = torch.randn(N, F, generator=g).to(dev).requires_grad_(True)
    leaves = [pq, res]
    a = wf = ws = terms = None
    if mode == 'linear':
        a = torch.randn(E, De, generator=g).to(dev).requires_grad_(True)
        wf = torch.randn(F, De, generator=g).to(dev).requires_grad_(True)
        ws = torch.randn(F, De, generator=g).to(dev).requires_grad_(True)
        leaves += [a, wf, ws]
    if mode == 'wide':
        terms = torch.randn(E, 2 * F, generator=g).to(dev).requires_grad_(True)
        leaves += [terms]
    go = torch.randn(N, F, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = CGAggregateFunction.apply(pq, None, a, wf, ws, terms, res, graph, N, True)
    grads = torch.autograd.grad(out, leaves, go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    plane = E * F * 4
    print(f'{mode}: peak above the inputs: {extra / 2 ** 20:.1f} MiB (one [E, F]: '
          f'{plane / 2 ** 20:.0f} MiB)')
    assert plane >= 64 * 2 ** 20
    assert extra < (3 * plane if mode == 'wide' else plane)
    assert all(bool(torch.isfinite(t).all()) for t in grads)


# ---- routing --------------------------------------------------------------------------------------------
def _layer64(conv, x_src, x_dst, a, ei, **kw):
    state = {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu())
             for k, v in conv.state_dict().items()}
    return R.cg_layer(state, x_src, x_dst, a, ei, **kw)


def test_routing(dev, monkeypatch):
    """More than 512 channels, target_to_source, ``max``, ``fuse = False``, host tensors, a
    message hook (which sees the messages), explain mode and a subclass with its own ``message`` (which is used) take the
    generic or the host route and match float64; the supported layers — no edge term, raw
    features, the dense edge terms past the register envelope, the mean, a batch norm — take the
    new route."""
    from pytorch_geometric_amd.nn import CGConv

    class _Scaled(CGConv):
        def message(self, x_i, x_j, edge_attr):
            return 0.5 * super().message(x_i, x_j, edge_attr)

    ei = random_graph(300, 300, 3000, 91)
    for what, F, De, kw, device in (
            ('channels = 520', 520, 0, {}, dev),
            ('target_to_source', 24, 3, dict(flow='target_to_source'), dev),
            ('max', 24, 3, dict(aggr='max'), dev),
            ('fuse = False', 24, 3, {}, dev),
            ('host tensors', 24, 3, {}, 'cpu'),
            ('message hook', 24, 3, {}, dev),
            ('explain mode', 24, 3, {}, dev),
            ('subclass with its own message', 24, 3, {}, dev),
            ('supported', 24, 3, {}, dev),
            ('supported without dim', 24, 0, {}, dev),
            ('supported, dim = 41', 24, 41, {}, dev),
            ('supported, mean', 24, 3, dict(aggr='mean'), dev),
            ('supported, batch norm', 24, 3, dict(batch_norm=True), dev)):
        torch.manual_seed(9)
        kind = _Scaled if what.startswith('subclass') else CGConv
        dtype = torch.float32
        conv = kind(F, dim=De, **kw).to(device)
        conv.fuse = True                   # (whatever the switch's default names)
        if what == 'explain mode':
            conv.explain = True
        seen = []
        if what == 'message hook':
            conv.register_message_forward_hook(lambda mod, args, out: seen.append(out.shape))
        if what == 'fuse = False':
            conv.fuse = False
        g = gen(92)
        x0 = torch.randn(300, F, generator=g)
        a0 = torch.randn(3000, De, generator=g) if De else None
        x = x0.to(device, dtype).requires_grad_(True)
        a = None if a0 is None else a0.to(device, dtype).requires_grad_(True)
        leaves = [x] + ([] if a is None else [a])
        state = {}

        def step():
            state['out'] = conv(x, ei.to(device), edge_attr=a)
            state['grad'] = torch.autograd.grad(state['out'].sum(), leaves)

        c = T._counted(monkeypatch, step)
        fused = sorted(n for n in c.calls if n in FUSED)
        if what.startswith('supported'):
            assert fused == sorted(FUSED), (what, c.calls)
        else:
            assert not fused, (what, c.calls)
        if what == 'message hook':
            assert seen == [(3000, F)], seen
        assert state['out'].dtype == dtype and all(t.dtype == dtype for t in state['grad']), what
        x64 = x0.double().requires_grad_(True)
        a64 = None if a0 is None else a0.double().requires_grad_(True)
        want = _layer64(conv, x64, x64, a64, ei, aggr=kw.get('aggr', 'add'),
                        flow=kw.get('flow', 'source_to_target'))
        if kind is _Scaled:      # (0.5 * message, then the residual)
            want = 0.5 * (want - x64) + x64
        assert_close_scaled(state['out'], want.detach().float(), tol=TOL, what=f'{what} out')
        for n, got, w in zip(('grad_x', 'grad_edge_attr'), state['grad'],
                             torch.autograd.grad(want.sum(), [x64] + ([] if a64 is None else [a64]))):
            assert_close_scaled(got, w.float(), tol=TOL, what=f'{what} {n}')


def test_float64_tensors_are_never_narrowed(dev, monkeypatch):
    """"float32 after widening" means float32, half or bfloat16 in.  float64 device tensors do not
    take the fused route, so no kernel runs and nothing is cast down; this package's generic route
    serves float32 on the device and refuses float64 by name (``ValueError``), and float32 ``x``
    with float64 ``edge_attr`` is refused as ``torch.nn.Linear`` refuses mixed dtypes.  On the
    host the same float64 layer computes in float64 and matches the restatement."""
    from pytorch_geometric_amd.nn import CGConv
    ei = random_graph(300, 300, 3000, 91)
    x0 = torch.randn(300, 24, generator=gen(93))
    a0 = torch.randn(3000, 3, generator=gen(94))
    for what, De, x_dtype, a_dtype in (('float64 x', 0, torch.float64, None),
                                       ('float64 x and edge_attr', 3, torch.float64, torch.float64),
                                       ('float64 edge_attr', 3, torch.float32, torch.float64)):
        torch.manual_seed(9)
        conv = CGConv(24, dim=De).to(dev, x_dtype)
        conv.fuse = True
        x = x0.to(dev, x_dtype)
        a = a0.to(dev, a_dtype) if De else None

        def step():
            with pytest.raises((ValueError, RuntimeError), match='float32|dtype|Float|Double'):
                conv(x, ei.to(dev), edge_attr=a)

        c = T._counted(monkeypatch, step)
        assert not [n for n in c.calls if 'pygamd_cg_' in n], (what, c.calls)
        if a_dtype is not torch.float32 and x_dtype is torch.float64:
            host = conv.cpu()
            x64 = x0.double().requires_grad_(True)
            a64 = a0.double().requires_grad_(True) if De else None
            out = host(x64, ei, edge_attr=a64)
            assert out.dtype == torch.float64
            want = _layer64(host, x64, x64, a64, ei)
            err = float((out - want).detach().abs().max())
            assert err <= 1e-12 * float(want.detach().abs().max()), what


def test_half_layer_with_batch_norm_is_widened(dev, monkeypatch):
    """a layer moved to float16 or bfloat16 holds its batch norm in that dtype; the fused route
    widens its parameters and statistics as it widens the weights.  Against the float32 layer that
    holds the SAME rounded values: the output at one unit in the last place of the low dtype, as
    test_half_inputs_are_widened; the running statistics, float32 values rounded once to the low
    dtype, at the same bound; and the backward takes the fused route too."""
    import copy
    from pytorch_geometric_amd.nn import CGConv
    torch.manual_seed(4)
    conv = CGConv(16, dim=4, aggr='mean', batch_norm=True).to(dev)
    conv.bn.weight.data.normal_(1.0, 0.2)
    conv.bn.bias.data.normal_(0, 0.3)
    conv.fuse = True
    x = torch.randn(300, 16, generator=gen(94)).to(dev)
    ei = random_graph(300, 300, 3000, 95).to(dev)
    ea = torch.randn(3000, 4, generator=gen(98)).to(dev)
    for low, ulp in ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)):
        half = copy.deepcopy(conv).to(low)
        wide = copy.deepcopy(half).float()              # the rounded parameters, in float32
        assert half.bn.weight.dtype == low and half.bn.running_mean.dtype == low
        xl, el = x.to(low), ea.to(low)
        want = wide(xl.float(), ei, el.float())
        state = {}
        c = T._counted(monkeypatch, lambda: state.update(out=half(xl, ei, el)))
        assert c.calls.get('pygamd_cg_forward') == 1, (low, c.calls)
        got = state['out']
        assert got.dtype == low
        assert_close(got.float(), want, rtol=ulp, atol=1e-6, what=f'{low} with batch norm')
        assert half.bn.running_mean.dtype == low and int(half.bn.num_batches_tracked) == 1
        for name in ('running_mean', 'running_var'):
            assert_close(getattr(half.bn, name).float(), getattr(wide.bn, name), rtol=ulp,
                         atol=1e-6, what=f'{low} {name}')
        xg = xl.clone().requires_grad_(True)
        c = T._counted(monkeypatch, lambda: half(xg, ei, el).float().sum().backward())
        assert c.calls.get('pygamd_cg_backward_dst') == 1, (low, c.calls)
        assert c.calls.get('pygamd_cg_backward_src') == 1, (low, c.calls)
        assert xg.grad.dtype == low and bool(torch.isfinite(xg.grad).all())
        assert half.bn.weight.grad is not None and half.bn.weight.grad.dtype == low


def test_the_switch_names_the_modes_that_fuse(dev, monkeypatch):
    """a layer whose edge mode the switch does not name starts with ``fuse = False`` and takes
    the generic route; ``fuse = True`` on the layer overrides it"""
    from pytorch_geometric_amd.nn import CGConv
    from pytorch_geometric_amd.nn.conv import cg_conv
    monkeypatch.setattr(cg_conv, 'FUSE_CG', ('linear', ))
    convs = {De: CGConv(24, dim=De).to(dev) for De in (0, 3, 41)}
    monkeypatch.undo()                      # (the counting below undoes every patch anyway)
    x = torch.randn(300, 24, generator=gen(93)).to(dev)
    ei = random_graph(300, 300, 3000, 91).to(dev)
    for De, fuse in ((0, False), (3, True), (41, False)):
        conv = convs[De]
        assert conv.fuse is fuse
        a = torch.randn(3000, De, generator=gen(94)).to(dev) if De else None
        state = {}
        c = T._counted(monkeypatch, lambda: state.update(out=conv(x, ei, edge_attr=a)))
        assert (c.calls.get('pygamd_cg_forward') == 1) is fuse, c.calls
        conv.fuse = True
        c = T._counted(monkeypatch, lambda: state.update(fused=conv(x, ei, edge_attr=a)))
        assert c.calls.get('pygamd_cg_forward') == 1, c.calls
        assert_close_scaled(state['fused'], state['out'], tol=TOL, what=f'dim = {De}')


def test_half_inputs_are_widened(dev, monkeypatch):
    """float16 and bfloat16 layers take the fused route, compute in float32 and hand the result
    back in their dtype: against the float32 layer whose parameters and inputs hold the SAME
    rounded values, the only difference is the last rounding to the low dtype, one unit in the
    last place of 2^-11 (float16) or 2^-8 (bfloat16) relative to each entry."""
    import copy
    from pytorch_geometric_amd.nn import CGConv
    for dim in (0, 4, 41):
        torch.manual_seed(4)
        conv = CGConv(16, dim=dim, aggr='mean').to(dev)
        conv.fuse = True
        x = torch.randn(300, 16, generator=gen(94)).to(dev)
        ei = random_graph(300, 300, 3000, 95).to(dev)
        ea = torch.randn(3000, dim, generator=gen(98)).to(dev) if dim else None
        for low, ulp in ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)):
            half = copy.deepcopy(conv).to(low)
            wide = copy.deepcopy(half).float()              # the rounded parameters, in float32
            xl, el = x.to(low), None if ea is None else ea.to(low)
            want = wide(xl.float(), ei, None if el is None else el.float())
            state = {}
            c = T._counted(monkeypatch, lambda: state.update(out=half(xl, ei, el)))
            assert c.calls.get('pygamd_cg_forward') == 1, (low, c.calls)
            got = state['out']
            assert got.dtype == low
            assert_close(got.float(), want, rtol=ulp, atol=1e-6, what=f'{low} dim = {dim}')
            xg = xl.clone().requires_grad_(True)            # the backward takes the fused route too
            c = T._counted(monkeypatch, lambda: half(xg, ei, el).float().sum().backward())
            assert c.calls.get('pygamd_cg_backward_dst') == 1, (low, c.calls)
            assert c.calls.get('pygamd_cg_backward_src') == 1, (low, c.calls)
            assert xg.grad.dtype == low and bool(torch.isfinite(xg.grad).all())


def test_inside_hetero_conv_with_edge_attr_dict(dev, monkeypatch):
    from pytorch_geometric_amd.nn import CGConv, HeteroConv
    torch.manual_seed(6)
    layer = CGConv((16, 12), dim=3)
    plain = CGConv((12, 16), aggr='mean')
    layer.fuse = plain.fuse = True
    hetero = HeteroConv({('a', 'to', 'b'): layer, ('b', 'back', 'a'): plain}).to(dev)
    ei, ei_back = random_graph(400, 150, 2500, 97), random_graph(150, 400, 2000, 98)
    g = gen(96)
    xa0, xb0 = torch.randn(400, 16, generator=g), torch.randn(150, 12, generator=g)
    ea0 = torch.randn(2500, 3, generator=g)
    xa, xb, ead = [t.to(dev).requires_grad_(True) for t in (xa0, xb0, ea0)]
    state = {}

    def step():
        state['out'] = hetero({'a': xa, 'b': xb},
                              {('a', 'to', 'b'): ei.to(dev), ('b', 'back', 'a'): ei_back.to(dev)},
                              edge_attr_dict={('a', 'to', 'b'): ead})

    c = T._counted(monkeypatch, step)
    assert c.calls.get('pygamd_cg_forward') == 2, c.calls
    out = state['out']
    assert set(out) == {'a', 'b'} and out['b'].shape == (150, 12) and out['a'].shape == (400, 16)
    go = torch.randn(150, 12, generator=g)
    grads = torch.autograd.grad((out['b'] * go.to(dev)).sum() + out['a'].sum(), [xa, xb, ead])
    leaves = [t.double().requires_grad_(True) for t in (xa0, xb0, ea0)]
    want_b = _layer64(layer, leaves[0], leaves[1], leaves[2], ei)
    want_a = _layer64(plain, leaves[1], leaves[0], None, ei_back, aggr='mean')
    assert_close_scaled(out['b'], want_b.detach().float(), tol=TOL, what='hetero out b')
    assert_close_scaled(out['a'], want_a.detach().float(), tol=TOL, what='hetero out a')
    for name, got, ref in zip(('grad a', 'grad b', 'grad edge_attr'), grads,
                              torch.autograd.grad((want_b * go.double()).sum() + want_a.sum(),
                                                  leaves)):
        assert_close_scaled(got, ref.float(), tol=TOL, what=f'hetero {name}')


# ---- the registered operators -----------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'cg_aggregate' in ops.OPS and 'cg_aggregate_backward' in ops.OPS
    op = torch.ops.pyg_amd.cg_aggregate
    with FakeTensorMode():
        p = torch.empty(12, 48, device='cuda', requires_grad=True)
        q = torch.empty(50, 48, device='cuda', requires_grad=True)
        pq = torch.empty(12, 96, device='cuda', requires_grad=True)
        a = torch.empty(400, 5, device='cuda')
        wf, ws = torch.empty(24, 5, device='cuda'), torch.empty(24, 5, device='cuda')
        terms, res = torch.empty(400, 48, device='cuda'), torch.empty(12, 24, device='cuda')
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        eid = torch.empty(400, dtype=torch.int32, device='cuda')
        for args in ((p, q, a, wf, ws, None, res, ptr, col, eid, False),
                     (p, q, None, None, None, terms, None, ptr, col, None, True),
                     (pq, None, None, None, None, None, None, ptr, col, None, False)):
            out = op(*args)
            assert out.shape == (12, 24) and out.requires_grad
            assert out.device.type == 'cuda' and out.dtype == torch.float32

    P = _uniform_case(64, 7)
    want = P['want'][(True, True)]
    order = torch.argsort(P['ei'][1], stable=True)
    col = P['ei'][0][order].to(dev)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], 2000).to(dev)
    eid = order.to(dev)                 # slot -> the caller's edge: edge_attr stays in COO order
    go = P['go'].to(dev)

    def fn(p, q, a, wf, ws, res):
        return (op(p * 1.0, q, a, wf, ws, None, res, ptr, col, eid, True) * go).sum()

    def leaves():
        return [P[n].to(dev).requires_grad_(True) for n in ('p', 'q', 'a', 'wf', 'ws', 'res')]

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        y = f(*ls)
        results.append([y.detach()] + list(torch.autograd.grad(y, ls)))
    for x, y in zip(*results):
        assert_close(y, x, what='compiled vs eager')
    ls = [t.detach() for t in leaves()]
    out = op(*ls[:5], None, ls[5], ptr, col, eid, True)
    _check([out] + results[0][1:], want, 'operator')
    # edge_id = None: edge_attr follows the slots of col
    assert torch.equal(op(ls[0], ls[1], ls[2][eid], ls[3], ls[4], None, ls[5], ptr, col, None,
                          True), out)
    # the packed plane and the dense edge terms
    W = _uniform_case(64, 41, True)
    pq = torch.cat([W['p'], W['q']], dim=1).to(dev).requires_grad_(True)
    terms = W['terms'].to(dev).requires_grad_(True)
    y = op(pq, None, None, None, None, terms, None, ptr, col, eid, False)
    g_pq, g_terms = torch.autograd.grad(y, [pq, terms], W['go'].to(dev))
    _check([y.detach(), g_pq[:, :128], g_pq[:, 128:], g_terms], W['want'][(False, False)][:4],
           'operator, packed and wide')
    ls = leaves()
    torch.library.opcheck(op, (*ls[:5], None, ls[5], ptr, col, eid, True))
    torch.library.opcheck(op, (pq.detach().requires_grad_(True), None, None, None, None,
                               terms.detach().requires_grad_(True), None, ptr, col, eid, False))
