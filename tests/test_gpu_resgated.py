"""nn.ResGatedGraphConv on the device: the recorded reference cases with their launch counts, the
kernels of csrc/resgated.hip against the float64 restatement (tests/_resgated_ref.py, the UNSPLIT
``cat`` then ``Linear`` form) run on the device, an exact test with every gate at 0.5, saturated
gates, non-finite inputs, empty rows, long rows through the chunked schedule, bitwise repeatability,
the memory promise, routing, half inputs, HeteroConv and the registered operators.  Nothing here
reads the reference tree.

Figures measured on one gfx950 device are in profiles/resgated_conv.md."""
import pytest
import torch

import _resgated_ref as R
import test_gpu_transformer as T
from _util import assert_close, assert_close_scaled, gen, random_graph

pytestmark = pytest.mark.gpu

NAMES = ('out', 'grad_k', 'grad_q', 'grad_v', 'grad_edge_attr', 'grad_Wg', 'grad_Wv')
TOL = 2e-5
FUSED = ('pygamd_resgated_forward', 'pygamd_resgated_backward_dst', 'pygamd_resgated_backward_src')


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_the_device(dev, monkeypatch, name, index_dtype):
    """A fused case: ONE forward and ONE launch per backward direction and nothing else that
    touches the edges.  ``tanh`` and ``mean``: the generic route, no resgated call."""
    c = T._counted(monkeypatch, lambda: R.check_class_case(R.load_golden(), name, dev,
                                                           index_dtype=index_dtype))
    if name in R.FUSED_CASES:
        for fn in FUSED:
            assert c.calls.get(fn) == 1, c.calls
        assert not [n for n in c.calls if 'spmm' in n or 'scatter' in n or 'softmax' in n], c.calls
    else:
        assert not [n for n in c.calls if 'pygamd_resgated_' in n], c.calls


def test_golden_stack_on_the_device(dev, monkeypatch):
    c = T._counted(monkeypatch, lambda: R.check_stack(R.load_golden(), dev))
    for fn in FUSED:
        assert c.calls.get(fn) == 2, c.calls


# ---- problems ---------------------------------------------------------------------------------------
def _problem(n_src, n_dst, ei, F, De, seed, k_rows=None):
    """random normal K [k_rows or n_dst, F], Q, V [n_src, F], grad_out; with ``De``: raw edge
    features and the edge columns of the three ``Linear`` (z has a standard deviation of about 2)"""
    g = gen(seed)
    E = ei.size(1)
    P = {'ei': ei, 'n_src': n_src, 'n_dst': n_dst, 'F': F, 'De': De,
         'k': torch.randn(k_rows or n_dst, F, generator=g),
         'q': torch.randn(n_src, F, generator=g), 'v': torch.randn(n_src, F, generator=g),
         'go': torch.randn(n_dst, F, generator=g), 'a': None, 'wk': None, 'wq': None, 'wv': None}
    if De:
        P['a'] = torch.randn(E, De, generator=g)
        for n in ('wk', 'wq', 'wv'):
            P[n] = torch.randn(F, De, generator=g) / De ** 0.5
    return P


def _reference(P, dtype=torch.float64, device='cuda'):
    """the seven of NAMES from the restatement run on ``device`` (None where an input is absent),
    as CPU tensors.  With ``De`` each ``Linear`` reads ``cat([row, a])`` with the weight ``[I | W_e]``
    (the identity block is exact), so its edge columns are used UNSPLIT; grad_Wg is the gradient of
    the key's edge columns (the query's is the same)."""
    F = P['F']
    k, q, v = [P[n].to(device, dtype).requires_grad_(True) for n in ('k', 'q', 'v')]
    a, wk, wq, wv = [None if P[n] is None else P[n].to(device, dtype).requires_grad_(True)
                     for n in ('a', 'wk', 'wq', 'wv')]
    lins = None
    if a is not None:
        eye = torch.eye(F, dtype=dtype, device=device)
        lins = [(torch.cat([eye, w], dim=1), None) for w in (wk, wq, wv)]
    out = R.resgated_aggregate(k, q, v, a, lins, P['ei'].to(device), P['n_dst'])
    leaves = [t for t in (k, q, v, a, wk, wv) if t is not None]
    if P['ei'].size(1) == 0:
        grads = [torch.zeros_like(t) for t in leaves]
    else:
        grads = torch.autograd.grad(out, leaves, P['go'].to(device, dtype))
    grads = list(grads) + [None] * (6 - len(leaves))
    return [out.detach().cpu()] + [None if g is None else g.detach().cpu() for g in grads]


def _device_run(P, dev, index_dtype=torch.int64, edge_grad=True, strided=False):
    """the same seven through the autograd node, and the handle"""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import ResGatedAggregateFunction
    F = P['F']
    qv0 = torch.cat([P['q'], P['v']], dim=1)
    if strided:   # column blocks of wider tensors, read in place
        wide_k = torch.zeros(P['k'].size(0), 2 * F)
        wide_k[:, :F] = P['k']
        k = wide_k.to(dev)[:, :F].detach().requires_grad_(True)
        wide_qv = torch.zeros(P['n_src'], 3 * F)
        wide_qv[:, F:] = qv0
        qv = wide_qv.to(dev)[:, F:].detach().requires_grad_(True)
        assert k.stride(0) == 2 * F and qv.stride(0) == 3 * F
    else:
        k, qv = P['k'].to(dev).requires_grad_(True), qv0.to(dev).requires_grad_(True)
    a = wg = wv = None
    if P['a'] is not None:
        a = P['a'].to(dev).requires_grad_(edge_grad)
        wg = (P['wk'] + P['wq']).to(dev).requires_grad_(True)
        wv = P['wv'].to(dev).requires_grad_(True)
    graph = P.get('graph')
    if graph is None or graph.edge_index.dtype != index_dtype:
        graph = as_edge_index(P['ei'].to(dev).to(index_dtype), P['n_src'], P['n_dst'])
    out = ResGatedAggregateFunction.apply(k, qv, a, wg, wv, graph, P['n_dst'])
    leaves = [t for t in (k, qv, a, wg, wv) if t is not None and t.requires_grad]
    grads = dict(zip([id(t) for t in leaves], torch.autograd.grad(out, leaves, P['go'].to(dev))))
    g_qv = grads[id(qv)]
    return [out.detach(), grads[id(k)], g_qv[:, :F], g_qv[:, F:]] + [
        None if t is None else grads.get(id(t)) for t in (a, wg, wv)], graph


def _check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, f'{what}: {name} should be absent'
            continue
        assert g is not None, f'{what}: {name} is missing'
        assert_close_scaled(g, w.float(), tol=TOL, what=f'{what} {name}')


# ---- the kernels against float64 ------------------------------------------------------------------
_UNIFORM = {}


def _uniform_case(F, De):
    """problem and float64 results at one shape, computed once for both index dtypes"""
    if (F, De) not in _UNIFORM:
        P = _problem(2000, 2000, T._uniform_graph(), F, De, 300 + F + 7 * De)
        P['want'] = _reference(P)
        _UNIFORM[(F, De)] = P
    return _UNIFORM[(F, De)]


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('F,De', [(1, 0), (5, 0), (24, 0), (64, 0), (100, 0), (128, 0), (132, 0),
                                  (256, 0), (512, 0), (8, 1), (24, 3), (64, 7), (128, 16),
                                  (256, 8), (512, 4), (64, 32), (400, 5), (292, 7), (290, 7),
                                  (200, 10), (136, 15), (130, 15), (100, 20)])
def test_kernels_match_float64(dev, F, De, index_dtype):
    """F below one lane group, odd, the float4 widths and the limit; (F, De) through the register
    capacities for De and the corners of the envelope, where a lane holds 32 registers per edge
    matrix ((EPL, DE) = (2, 16), (4, 8), (8, 4), (1, 32)); then the shapes whose sizes round up to
    the five lane shapes of 64 registers per matrix, the ones with one slot in flight and, by
    destination, 256 VGPRs plus AGPRs: (8, 8) as float4 units ((400, 5), (292, 7)) and scalar
    ((290, 7)), (4, 16) as float4 units ((200, 10), (136, 15)) and scalar ((130, 15)), (2, 32)
    ((100, 20)).  Contiguous inputs, then K and QV as column blocks of wider tensors."""
    P = _uniform_case(F, De)
    got, graph = _device_run(P, dev, index_dtype=index_dtype)
    P['graph'] = graph
    _check(got, P['want'], f'({F}, {De})')
    got, _ = _device_run(P, dev, index_dtype=index_dtype, strided=True)
    _check(got, P['want'], f'({F}, {De}) strided')


@pytest.mark.parametrize('F,De', [(24, 0), (24, 3), (132, 5)])
def test_destinations_a_prefix_empty_rows_and_no_edges(dev, F, De):
    """300 destinations, a prefix of 900 sources whose K has 900 rows; destinations without slots
    get exact zeros, sources without slots (and the rows of K beyond the destinations) zero
    gradients; a graph without edges."""
    ei = random_graph(900, 300, 5000, 43)
    ei = ei[:, (ei[1] % 7 != 0) & (ei[0] % 5 != 0)]
    P = _problem(900, 300, ei, F, De, 11, k_rows=900)
    want = _reference(P)
    for strided in (False, True):
        got, _ = _device_run(P, dev, strided=strided)
        _check(got, want, f'prefix ({F}, {De})')
        assert got[0].shape == (300, F) and got[1].shape == (900, F) and got[2].shape == (900, F)
        empty_dst = torch.bincount(ei[1], minlength=300) == 0
        empty_src = torch.bincount(ei[0], minlength=900) == 0
        assert int(empty_dst.sum()) >= 40 and int(empty_src.sum()) >= 180
        assert float(got[0].cpu()[empty_dst].abs().max()) == 0.0      # exact zeros
        assert float(got[1].cpu()[:300][empty_dst].abs().max()) == 0.0
        assert float(got[1][300:].abs().max()) == 0.0
        assert float(got[2].cpu()[empty_src].abs().max()) == 0.0
        assert float(got[3].cpu()[empty_src].abs().max()) == 0.0
    Z = _problem(50, 40, torch.zeros(2, 0, dtype=torch.int64), F, De, 12)
    got, _ = _device_run(Z, dev)
    assert got[0].shape == (40, F) and float(got[0].abs().max()) == 0.0
    assert all(float(g.abs().max()) == 0.0 for g in got[1:4])
    assert got[1].shape == (40, F) and got[2].shape == (50, F)
    if De:
        assert got[4].shape == (0, De)
        assert float(got[5].abs().max()) == 0.0 and float(got[6].abs().max()) == 0.0


# ---- exact: every gate at 0.5 --------------------------------------------------------------------------
@pytest.mark.parametrize('graph', ['uniform', 'hub'])
def test_gates_of_one_half_are_exact(dev, graph):
    """Q_j = c for every source and K_i = -c: z = 0 and the sigmoid is exactly 0.5.  With V and
    grad_out on the grid of eighths, out = sum v / 2, grad_V = sum g / 2, grad_K = g * sum v / 4 and
    grad_Q = v * sum g / 4 are computed in integers and reproduced bit for bit."""
    ei, n = (T._uniform_graph(), 2000) if graph == 'uniform' else (T._long_problem()['ei'], 3000)
    F = 24
    g = gen(61)
    c = torch.randint(-16, 17, (F, ), generator=g).float() / 8
    v8 = torch.randint(-16, 17, (n, F), generator=g)
    g8 = torch.randint(-16, 17, (n, F), generator=g)
    P = {'ei': ei, 'n_src': n, 'n_dst': n, 'F': F, 'De': 0, 'a': None, 'wk': None, 'wq': None,
         'wv': None, 'k': (-c).expand(n, F).contiguous(), 'q': c.expand(n, F).contiguous(),
         'v': v8.float() / 8, 'go': g8.float() / 8}
    src, dst = ei[0], ei[1]
    sum_v = torch.zeros(n, F, dtype=torch.int64).index_add(0, dst, v8[src])     # eighths
    sum_g = torch.zeros(n, F, dtype=torch.int64).index_add(0, src, g8[dst])
    assert int((g8 * sum_v).abs().max()) < 2 ** 24 and int((v8 * sum_g).abs().max()) < 2 ** 24
    want = [sum_v.double() / 16, (g8 * sum_v).double() / 256, (v8 * sum_g).double() / 256,
            sum_g.double() / 16]
    got, _ = _device_run(P, dev)
    for name, a, b in zip(NAMES, got[:4], want):
        assert torch.equal(a.cpu(), b.float()), f'{graph}: {name} is not exact'


# ---- saturated gates ---------------------------------------------------------------------------------
@pytest.mark.parametrize('big', [100.0, 1e4])
def test_saturated_gates(dev, big):
    """z = +-big per (row, column): outputs and gradients are finite and match float64; beyond the
    range of expf the gate is exactly 0 or 1 and its gradient exactly 0."""
    P = _problem(2000, 2000, T._uniform_graph(), 24, 0, 71)
    sign = torch.randint(0, 2, (2000, 24), generator=gen(72)).float() * 2 - 1
    P['k'], P['q'] = sign * big, torch.zeros(2000, 24)
    got, _ = _device_run(P, dev)
    assert all(bool(torch.isfinite(t).all()) for t in got[:4])
    _check(got, _reference(P), f'z = +-{big}')
    if big >= 1e4:
        assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
        keep = (sign > 0).float()                  # gate 1 where z > 0, else 0: out = sum of those v
        out = torch.zeros(2000, 24, dtype=torch.float64).index_add(
            0, P['ei'][1], P['v'][P['ei'][0]].double()) * keep.double()
        assert_close_scaled(got[0], out.float(), tol=TOL, what='gates of exactly 0 and 1')


# ---- non-finite inputs ----------------------------------------------------------------------------------
def _composition(P, dtype):
    """the torch composition on the host at the level of the kernels' inputs, in ``dtype``: gather,
    the two edge terms as products with the raw features, sigmoid, product, index_add (``cat`` with
    an identity block would spread one infinity over its whole row as inf * 0)"""
    k, q, v = [P[n].to(dtype).requires_grad_(True) for n in ('k', 'q', 'v')]
    src, dst = P['ei'][0], P['ei'][1]
    z, u = k[dst] + q[src], v[src]
    leaves = [k, q, v]
    if P['a'] is not None:
        a, wg, wv = [t.to(dtype).requires_grad_(True)
                     for t in (P['a'], P['wk'] + P['wq'], P['wv'])]
        z, u = z + a @ wg.t(), u + a @ wv.t()
        leaves += [a, wg, wv]
    out = torch.zeros(P['n_dst'], P['F'], dtype=dtype).index_add(0, dst, torch.sigmoid(z) * u)
    grads = list(torch.autograd.grad(out, leaves, P['go'].to(dtype))) + [None] * (6 - len(leaves))
    return [out.detach()] + grads


@pytest.mark.parametrize('De', [0, 3])
def test_non_finite_inputs(dev, De):
    """+inf, -inf and NaN planted in single entries of K, Q and V poison exactly the entries of the
    output and of the gradients that the float32 torch composition poisons (NaN for NaN, the same
    infinity for an infinity); every other entry still matches the float64 composition at the
    project's bound."""
    G = R.load_golden()
    ei = G['edge_index']
    P = _problem(48, 48, ei, 16, De, 81)
    P['k'][3, 2], P['k'][17, 5], P['k'][40, 11] = float('inf'), float('nan'), float('-inf')
    P['q'][5, 1], P['q'][20, 7], P['q'][33, 9] = float('-inf'), float('inf'), float('nan')
    P['v'][8, 3], P['v'][21, 14], P['v'][45, 0] = float('nan'), float('inf'), float('-inf')
    want = _composition(P, torch.float32)
    want64 = _composition(P, torch.float64)
    got, _ = _device_run(P, dev)
    assert int(want[0].isnan().sum()) >= 1 and int(want[0].isinf().sum()) >= 1
    assert int(torch.isfinite(want[0]).sum()) >= 48 * 16 - 40
    for name, g, w, w64 in zip(NAMES, got, want, want64):
        if w is None:
            continue
        g = g.cpu()
        assert torch.equal(g.isnan(), w.isnan()), f'{name}: NaN entries differ'
        assert torch.equal(g.isinf(), w.isinf()), f'{name}: infinite entries differ'
        inf = w.isinf()
        assert torch.equal(g[inf], w[inf]), f'{name}: signs of the infinities'
        ok = torch.isfinite(w)
        assert_close_scaled(g[ok], w64[ok].float(), tol=TOL,
                            what=f'{name}: the entries that stay finite')


# ---- long rows ------------------------------------------------------------------------------------
_LONG = {}


def _long_case(De):
    """the graph of test_gpu_transformer._long_problem (a 6000-slot destination, one of threshold +
    1 slots, a 2000-slot source) at F = 64, random normal inputs"""
    if De not in _LONG:
        P = _problem(3000, 3000, T._long_problem()['ei'], 64, De, 57 + De)
        P['want'] = _reference(P)
        _LONG[De] = P
    return _LONG[De]


@pytest.mark.parametrize('De', [0, 6])
def test_long_rows_match_float64_and_are_chunked(dev, monkeypatch, De):
    from pytorch_geometric_amd import _native
    P = _long_case(De)
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    got, graph = _device_run(P, dev)
    torch.cuda.synchronize()
    monkeypatch.undo()
    P['graph'] = graph
    ptr = graph.by_dst().ptr
    assert int(ptr[6] - ptr[5]) == 6000 and int(ptr[12] - ptr[11]) == _native.HUB_THRESHOLD + 1
    _check(got, P['want'], f'long rows De = {De}')
    info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'resgated'}
    assert set(info) == {'forward', 'backward_dst', 'backward_src'}
    chunk = _native.HUB_CHUNK
    want = -(-6000 // chunk) + -(-(_native.HUB_THRESHOLD + 1) // chunk)
    for op in ('forward', 'backward_dst'):
        assert info[op]['n_hub'] == 2 and info[op]['n_chunks'] == want
    assert info['backward_src']['n_hub'] == 1                       # source 7
    assert info['backward_src']['n_chunks'] >= -(-2000 // chunk)
    for rec in info.values():
        assert rec['F'] == 64 and rec['De'] == De
    assert info['backward_dst']['grad_edge_attr'] is (De > 0)


@pytest.mark.parametrize('De', [0, 6])
def test_two_runs_are_bitwise_identical(dev, De):
    """No float atomics anywhere and grids that depend on the problem only: every output and
    gradient, grad_Wg and grad_Wv from the per-workgroup partials included, repeats bit for bit on
    random inputs, long rows included."""
    P = _long_case(De)
    a, graph = _device_run(P, dev)
    P['graph'] = graph
    b, _ = _device_run(P, dev)
    for name, x, y in zip(NAMES, a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y), f'De = {De}: {name} differs between two runs'
    for shape in ((64, 7), (292, 7), (130, 15), (100, 20)):   # the last three: 64 registers each
        U = _uniform_case(*shape)
        a, _ = _device_run(U, dev)
        b, _ = _device_run(U, dev)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), shape


# ---- edge_attr without a gradient -----------------------------------------------------------------------
def test_without_a_gradient_for_edge_attr(dev, monkeypatch):
    from pytorch_geometric_amd import _native
    for P in (_uniform_case(64, 7), _uniform_case(200, 10), _uniform_case(290, 7),
              _long_case(6)):
        full, _ = _device_run(P, dev)
        sink = []
        monkeypatch.setattr(_native, 'timing_sink', sink)
        lean, _ = _device_run(P, dev, edge_grad=False)
        torch.cuda.synchronize()
        monkeypatch.undo()
        rec = [i for i, _, _ in sink if i.get('kind') == 'resgated' and i['op'] == 'backward_dst']
        assert len(rec) == 1 and rec[0]['grad_edge_attr'] is False
        assert lean[4] is None and full[4] is not None
        for name, x, y in zip(NAMES, lean, full):
            if name != 'grad_edge_attr':
                assert torch.equal(x, y), f'{name} differs without grad_edge_attr'


# ---- nothing of size E x F --------------------------------------------------------------------------
@pytest.mark.parametrize('De', [8, 0])
def test_keeps_nothing_of_edge_times_width(dev, De):
    """Above the inputs: out, grad_K (2 MiB each), the packed grad_QV (4 MiB), grad_edge_attr
    (8 MiB), the stacked edge matrices and the per-workgroup partials (4 MiB) — far below ONE
    [E, F] tensor, which is 128 MiB here."""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import ResGatedAggregateFunction
    N, E, F = 4096, 262144, 128
    graph = as_edge_index(random_graph(N, N, E, 71).to(dev), N, N)
    graph.fill_cache_()
    g = gen(72)
    k = torch.randn(N, F, generator=g).to(dev).requires_grad_(True)
    qv = torch.randn(N, 2 * F, generator=g).to(dev).requires_grad_(True)
    leaves = [k, qv]
    a = wg = wv = None
    if De:
        a = torch.randn(E, De, generator=g).to(dev).requires_grad_(True)
        wg = torch.randn(F, De, generator=g).to(dev).requires_grad_(True)
        wv = torch.randn(F, De, generator=g).to(dev).requires_grad_(True)
        leaves += [a, wg, wv]
    go = torch.randn(N, F, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ResGatedAggregateFunction.apply(k, qv, a, wg, wv, graph, N)
    grads = torch.autograd.grad(out, leaves, go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'De = {De}: peak above the inputs: {extra / 2 ** 20:.1f} MiB')
    assert E * F * 4 >= 64 * 2 ** 20
    assert extra < E * F * 4 // 2                              # 64 MiB; one [E, F] is 128 MiB
    assert all(bool(torch.isfinite(t).all()) for t in grads)


# ---- routing --------------------------------------------------------------------------------------------
def _layer64(conv, x_src, x_dst, a, ei, **kw):
    state = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
    return R.resgated_layer(state, x_src, x_dst, a, ei, **kw)


def test_routing(dev, monkeypatch):
    """Layouts outside the envelope, target_to_source, another aggregation, another gate, ``fuse
    = False``, host tensors, a message hook (which sees the messages) and a subclass with its own
    ``message`` (which is used) take the generic or the host route and match float64; the
    supported layer takes the new route."""
    from pytorch_geometric_amd.nn import ResGatedGraphConv

    class _Scaled(ResGatedGraphConv):
        def message(self, k_i, q_j, v_j, edge_attr):
            return 0.5 * super().message(k_i, q_j, v_j, edge_attr)

    ei = random_graph(300, 300, 3000, 91)
    for what, F, De, kw, device in (
            ('F * De = 4096', 512, 8, {}, dev),
            ('F = 1024', 1024, 0, {}, dev),
            ('edge_dim = 33', 24, 33, {}, dev),
            ('target_to_source', 24, 3, dict(flow='target_to_source'), dev),
            ('mean', 24, 3, dict(aggr='mean'), dev),
            ('tanh', 24, 3, dict(act=torch.nn.Tanh()), dev),
            ('fuse = False', 24, 3, {}, dev),
            ('host tensors', 24, 3, {}, 'cpu'),
            ('message hook', 24, 3, {}, dev),
            ('subclass with its own message', 24, 3, {}, dev),
            ('supported', 24, 3, {}, dev),
            ('supported without edge_dim', 24, 0, {}, dev)):
        torch.manual_seed(9)
        kind = _Scaled if what.startswith('subclass') else ResGatedGraphConv
        conv = kind(20, F, edge_dim=De or None, **kw).to(device)
        conv.bias.data.normal_(0, 0.3)
        seen = []
        if what == 'message hook':
            conv.register_message_forward_hook(lambda mod, args, out: seen.append(out.shape))
        if what == 'fuse = False':
            conv.fuse = False
        g = gen(92)
        x0 = torch.randn(300, 20, generator=g)
        a0 = torch.randn(3000, De, generator=g) if De else None
        x = x0.to(device).requires_grad_(True)
        a = None if a0 is None else a0.to(device).requires_grad_(True)
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
        x64 = x0.double().requires_grad_(True)
        a64 = None if a0 is None else a0.double().requires_grad_(True)
        act = kw.get('act', torch.sigmoid)
        if kind is _Scaled:
            act = lambda z: 0.5 * torch.sigmoid(z)                       # noqa: E731
        if what == 'message hook':
            assert seen == [(3000, F)], seen
        want = _layer64(conv, x64, x64, a64, ei, mean=kw.get('aggr') == 'mean', act=act,
                        flow=kw.get('flow', 'source_to_target'))
        assert_close_scaled(state['out'], want.detach().float(), tol=TOL, what=f'{what} out')
        for n, got, w in zip(('grad_x', 'grad_edge_attr'), state['grad'],
                             torch.autograd.grad(want.sum(), [x64] + ([] if a64 is None else [a64]))):
            assert_close_scaled(got, w.float(), tol=TOL, what=f'{what} {n}')


def test_half_inputs_are_widened(dev, monkeypatch):
    """float16 and bfloat16 layers take the fused route, compute in float32 and hand the result
    back in their dtype: against the float32 layer whose parameters and inputs hold the SAME
    rounded values, the only difference is the last rounding to the low dtype, one unit in the
    last place of 2^-11 (float16) or 2^-8 (bfloat16) relative to each entry."""
    import copy
    from pytorch_geometric_amd.nn import ResGatedGraphConv
    for edge_dim in (None, 4):
        torch.manual_seed(4)
        conv = ResGatedGraphConv(16, 16, edge_dim=edge_dim).to(dev)
        conv.bias.data.normal_(0, 0.3)
        x = torch.randn(300, 16, generator=gen(94)).to(dev)
        ei = random_graph(300, 300, 3000, 95).to(dev)
        ea = None if edge_dim is None else torch.randn(3000, edge_dim, generator=gen(98)).to(dev)
        for low, ulp in ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)):
            half = copy.deepcopy(conv).to(low)
            wide = copy.deepcopy(half).float()              # the rounded parameters, in float32
            xl, el = x.to(low), None if ea is None else ea.to(low)
            want = wide(xl.float(), ei, None if el is None else el.float())
            state = {}
            c = T._counted(monkeypatch, lambda: state.update(out=half(xl, ei, el)))
            assert c.calls.get('pygamd_resgated_forward') == 1, (low, c.calls)
            got = state['out']
            assert got.dtype == low
            assert_close(got.float(), want, rtol=ulp, atol=1e-6,
                         what=f'{low} edge_dim = {edge_dim}')
            xg = xl.clone().requires_grad_(True)            # the backward takes the fused route too
            c = T._counted(monkeypatch, lambda: half(xg, ei, el).float().sum().backward())
            assert c.calls.get('pygamd_resgated_backward_dst') == 1, (low, c.calls)
            assert c.calls.get('pygamd_resgated_backward_src') == 1, (low, c.calls)
            assert xg.grad.dtype == low and bool(torch.isfinite(xg.grad).all())


def test_inside_hetero_conv_with_edge_attr_dict(dev, monkeypatch):
    from pytorch_geometric_amd.nn import HeteroConv, ResGatedGraphConv
    torch.manual_seed(6)
    layer = ResGatedGraphConv((16, 12), 24, edge_dim=3)
    plain = ResGatedGraphConv((12, 16), 24)
    layer.bias.data.normal_(0, 0.3)
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
    assert c.calls.get('pygamd_resgated_forward') == 2, c.calls
    out = state['out']
    assert set(out) == {'a', 'b'} and out['b'].shape == (150, 24) and out['a'].shape == (400, 24)
    go = torch.randn(150, 24, generator=g)
    grads = torch.autograd.grad((out['b'] * go.to(dev)).sum() + out['a'].sum(), [xa, xb, ead])
    leaves = [t.double().requires_grad_(True) for t in (xa0, xb0, ea0)]
    want_b = _layer64(layer, leaves[0], leaves[1], leaves[2], ei)
    want_a = _layer64(plain, leaves[1], leaves[0], None, ei_back)
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
    assert 'resgated_aggregate' in ops.OPS and 'resgated_aggregate_backward' in ops.OPS
    op = torch.ops.pyg_amd.resgated_aggregate
    with FakeTensorMode():
        k = torch.empty(12, 24, device='cuda', requires_grad=True)
        qv = torch.empty(50, 48, device='cuda', requires_grad=True)
        a = torch.empty(400, 5, device='cuda')
        wg, wv = torch.empty(24, 5, device='cuda'), torch.empty(24, 5, device='cuda')
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        eid = torch.empty(400, dtype=torch.int32, device='cuda')
        for args in ((k, qv, a, wg, wv, ptr, col, eid), (k, qv, None, None, None, ptr, col, None)):
            out = op(*args)
            assert out.shape == (12, 24) and out.requires_grad
            assert out.device.type == 'cuda' and out.dtype == torch.float32

    P = _uniform_case(64, 7)
    want = P['want']
    order = torch.argsort(P['ei'][1], stable=True)
    col = P['ei'][0][order].to(dev)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], 2000).to(dev)
    eid = order.to(dev)                 # slot -> the caller's edge: edge_attr stays in COO order
    go = P['go'].to(dev)

    def fn(k, qv, a, wg, wv):
        return (op(k * 1.0, qv, a, wg, wv, ptr, col, eid) * go).sum()

    def leaves():
        return [t.to(dev).requires_grad_(True) for t in (
            P['k'], torch.cat([P['q'], P['v']], dim=1), P['a'], P['wk'] + P['wq'], P['wv'])]

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        y = f(*ls)
        results.append([y.detach()] + list(torch.autograd.grad(y, ls)))
    for x, y in zip(*results):
        assert_close(y, x, what='compiled vs eager')
    ls = [t.detach() for t in leaves()]
    out = op(*ls, ptr, col, eid)
    g_k, g_qv, g_a, g_wg, g_wv = results[0][1:]
    _check([out, g_k, g_qv[:, :64], g_qv[:, 64:], g_a, g_wg, g_wv], want, 'operator')
    # edge_id = None: edge_attr follows the slots of col
    ls[2] = ls[2][eid]
    assert torch.equal(op(*ls, ptr, col, None), out)
    torch.library.opcheck(op, (*leaves(), ptr, col, eid))
    ls = leaves()
    torch.library.opcheck(op, (ls[0], ls[1], None, None, None, ptr, col, None))
