"""nn.GENConv on the device: the recorded reference cases with their launch counts, the kernel
pair of csrc/gen.hip against the float64 restatement of the node (tests/_gen_ref.py), an exact
test that needs no ``exp``, a large temperature, long rows through the chunked schedule, bitwise
repeatability, non-finite inputs, the memory promise, routing, half inputs, HeteroConv and the
registered operator.  Nothing here reads the reference tree.

Inputs lie on the dyadic grid of test_gpu_gine.py: ``x``, ``grad_out`` = randint(-16, 17) / 8
(``x`` shifted by 1/16 where there is no edge term); wide ``edge_attr`` = randint(-16, 17) / 8 +
1/16; linear ``edge_attr`` and ``W`` = randint(-4, 5) / 4, ``b`` = randint(-8, 9) / 8 + 1/32.  The
ReLU's argument ``x + e`` is then an ODD multiple of 1/16 (linear: of 1/32) far below 2^24 units:
exact in float32 and never zero, so no mask can differ between float32 and float64; ``_problem``
asserts that.  The float64 values come from the restatement run on the device."""
import pytest
import torch

import _gen_ref as R
import test_gpu_transformer as T
from _util import assert_close, assert_close_scaled, gen, random_graph

pytestmark = pytest.mark.gpu

NAMES = ('out', 'grad_x_src', 'grad_edge_attr', 'grad_W', 'grad_b', 'grad_t')
TOL = 2e-5


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_the_device(dev, monkeypatch, name, index_dtype):
    """A softmax case: ONE forward and ONE backward launch of the new pair and nothing else that
    touches the edges.  ``powermean`` and ``mean``: the generic route, no gen call."""
    c = T._counted(monkeypatch, lambda: R.check_class_case(R.load_golden(), name, dev,
                                                           index_dtype=index_dtype))
    if name in R.SOFTMAX_CASES:
        assert c.calls.get('pygamd_gen_forward') == 1, c.calls
        assert c.calls.get('pygamd_gen_backward') == 1, c.calls
        assert not [n for n in c.calls if 'spmm' in n or 'scatter' in n or 'softmax' in n], c.calls
    else:
        assert not [n for n in c.calls if 'pygamd_gen_' in n], c.calls


def test_golden_stack_on_the_device(dev, monkeypatch):
    c = T._counted(monkeypatch, lambda: R.check_stack(R.load_golden(), dev))
    assert c.calls.get('pygamd_gen_forward') == 2 and c.calls.get('pygamd_gen_backward') == 2


# ---- problems ---------------------------------------------------------------------------------------
def _grid(g, lo, hi, shape, div, shift=0.0):
    return torch.randint(lo, hi, shape, generator=g).float() / div + shift


def _problem(n_src, n_dst, ei, F, De, seed, edge=True, exact=True):
    """``De > 0``: lin_edge; ``De = 0``: edge features of width F, or none (``edge=False``)."""
    g = gen(seed)
    E = ei.size(1)
    P = {'ei': ei, 'n_dst': n_dst, 'F': F, 'De': De, 'a': None, 'W': None, 'b': None}
    if not exact:
        P['x'], P['go'] = torch.randn(n_src, F, generator=g), torch.randn(n_dst, F, generator=g)
        if De:
            P['a'] = torch.randn(E, De, generator=g)
            P['W'] = torch.randn(F, De, generator=g) / De ** 0.5
            P['b'] = torch.randn(F, generator=g)
        elif edge:
            P['a'] = torch.randn(E, F, generator=g)
        return P
    P['x'] = _grid(g, -16, 17, (n_src, F), 8, 0.0 if (edge or De) else 1 / 16)
    P['go'] = _grid(g, -16, 17, (n_dst, F), 8)
    if De:
        P['a'] = _grid(g, -4, 5, (E, De), 4)
        P['W'] = _grid(g, -4, 5, (F, De), 4)
        P['b'] = _grid(g, -8, 9, (F, ), 8, 1 / 32)
    elif edge:
        P['a'] = _grid(g, -16, 17, (E, F), 8, 1 / 16)
    if E:
        # |x| <= 2 + 1/16, |e| <= De + 1 + 1/16: far below 2^24 units of 1/32, and odd
        assert (2 + 1 / 16 + max(De, 1) + 1 + 1 / 16) * 32 < 2 ** 24
        unit = 32 if De else 16
        _, pre32 = R.gen_message(P['x'], P['a'], P['W'], P['b'], ei[0])
        _, pre64 = R.gen_message(*[None if v is None else v.double()
                                   for v in (P['x'], P['a'], P['W'], P['b'])], ei[0])
        assert torch.equal(pre32.double(), pre64) and bool((pre64 * unit % 2 == 1).all())
    return P


def _t(kind, F, seed=0):
    """``(t tensor, learned, semi_grad)`` of a named variant"""
    if kind == 'learn':
        return torch.tensor([0.7]), True, False
    if kind == 'channels':
        return torch.rand(F, generator=gen(900 + seed)) * 1.5 - 0.5, True, False
    if kind == 'semi':
        return torch.tensor([1.5]), False, True
    return torch.tensor([float(kind)]), False, False


def _reference(P, t, learned, semi, dtype=torch.float64, device='cuda'):
    """the six of NAMES from the restatement run on ``device`` (None where an input is absent),
    handed back as CPU tensors"""
    x = P['x'].to(device, dtype).requires_grad_(True)
    a, W, b = [None if P[n] is None else P[n].to(device, dtype).requires_grad_(True)
               for n in ('a', 'W', 'b')]
    tt = t.to(device, dtype).requires_grad_(learned)
    ei = P['ei'].to(device)
    out = R.gen_aggregate(x, a, W, b, tt, ei, P['n_dst'], semi_grad=semi)
    leaves = [v for v in (x, a, W, b, tt) if v is not None and v.requires_grad]
    if P['ei'].size(1) == 0:
        grads = {id(v): torch.zeros_like(v) for v in leaves}
    else:
        grads = dict(zip([id(v) for v in leaves],
                         torch.autograd.grad(out, leaves, P['go'].to(device, dtype),
                                             allow_unused=True)))
    return [out.detach().cpu()] + [None if v is None or id(v) not in grads
                                   else grads[id(v)].detach().cpu() for v in (x, a, W, b, tt)]


def _device_run(P, dev, t, learned, semi, index_dtype=torch.int64, edge_grad=True, strided=False):
    """the same six through the autograd node, and the handle"""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import GenAggregateFunction
    F = P['F']
    if strided:   # the right half of a [n, 2 F] tensor, read in place
        wide = torch.zeros(P['x'].size(0), 2 * F)
        wide[:, F:] = P['x']
        x = wide.to(dev)[:, F:].detach().requires_grad_(True)
        assert x.stride(0) == 2 * F
    else:
        x = P['x'].to(dev).requires_grad_(True)
    a = None if P['a'] is None else P['a'].to(dev).requires_grad_(edge_grad)
    W, b = [None if P[n] is None else P[n].to(dev).requires_grad_(True) for n in ('W', 'b')]
    tt = t.to(dev).requires_grad_(learned)
    graph = P.get('graph')
    if graph is None or graph.edge_index.dtype != index_dtype:
        graph = as_edge_index(P['ei'].to(dev).to(index_dtype), P['x'].size(0), P['n_dst'])
    out = GenAggregateFunction.apply(x, a, W, b, tt, graph, P['n_dst'], 1e-7, semi)
    leaves = [v for v in (x, a, W, b, tt) if v is not None and v.requires_grad]
    grads = dict(zip([id(v) for v in leaves], torch.autograd.grad(out, leaves, P['go'].to(dev))))
    return [out.detach()] + [grads.get(id(v)) for v in (x, a, W, b, tt)], graph


def _check(got, want, P, t, what):
    """out and the gradients but grad_t at the project's 2e-5 of the tensor's scale; grad_t, a long
    cancelling sum, within 2e-5 of the float64 sum of its absolute per-edge terms or no worse than
    4 x the error of the float32 torch composition on the CPU."""
    for name, g, w in zip(NAMES[:5], got, want):
        if w is None:
            assert g is None, f'{what}: {name} should be absent'
            continue
        assert g is not None, f'{what}: {name} is missing'
        assert_close_scaled(g, w.float(), tol=TOL, what=f'{what} {name}')
    if want[5] is None:
        assert got[5] is None, f'{what}: grad_t should be absent'
        return
    assert got[5] is not None and got[5].shape == t.shape, f'{what}: grad_t'
    ins = [None if P[n] is None else P[n].double().cuda() for n in ('x', 'a', 'W', 'b')]
    abs_terms = R.grad_t_abs_terms(*ins, t.double().cuda(), P['ei'].cuda(), P['n_dst'],
                                   P['go'].double().cuda()).cpu()
    err = (got[5].detach().cpu().double() - want[5]).abs()
    print(f'{what}: grad_t max err / abs terms {float((err / abs_terms).max()):.3e}')
    assert bool(torch.isfinite(err).all()), f'{what}: grad_t is not finite'
    if not bool((err <= TOL * abs_terms).all()):
        ref32 = _reference(P, t, True, False, dtype=torch.float32, device='cpu')[5]
        err32 = float((ref32.double() - want[5]).abs().max())
        assert float(err.max()) <= 4 * err32, \
            f'{what}: grad_t err {float(err.max()):.3e} (float32 composition {err32:.3e})'


# ---- the kernels against float64 ------------------------------------------------------------------
_UNIFORM = {}
VARIANTS = ('1', '0.5', '-2', 'learn', 'channels', 'semi')


def _uniform_case(F, De, edge=True):
    """problem and float64 results of every variant at one shape, computed once for both index
    dtypes"""
    key = (F, De, edge)
    if key not in _UNIFORM:
        P = _problem(2000, 2000, T._uniform_graph(), F, De, 300 + F + 7 * De, edge=edge)
        P['t'] = {k: _t(k, F, F + De) for k in VARIANTS}
        P['want'] = {k: _reference(P, *P['t'][k]) for k in VARIANTS}
        _UNIFORM[key] = P
    return _UNIFORM[key]


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('F,De,edge', [(1, 0, True), (5, 0, True), (24, 0, True), (64, 0, True),
                                       (100, 0, True), (512, 0, True), (8, 1, True),
                                       (24, 3, True), (64, 7, True), (128, 32, True),
                                       (512, 8, True), (24, 0, False), (128, 0, False)])
def test_kernels_match_float64(dev, F, De, edge, index_dtype):
    """Wide F below one lane group, odd, the float4 widths and the limit; linear (F, De) through
    the register capacities for De and both limits; no edge term; t fixed (1, 0.5, -2), a learned
    scalar, a learned value per channel, semi_grad; x_src as a column block of a wider tensor."""
    P = _uniform_case(F, De, edge)
    for k in VARIANTS:
        got, graph = _device_run(P, dev, *P['t'][k], index_dtype=index_dtype)
        P['graph'] = graph
        _check(got, P['want'][k], P, P['t'][k][0], f'({F}, {De}, {edge}) t = {k}')
    got, _ = _device_run(P, dev, *P['t']['learn'], index_dtype=index_dtype, strided=True)
    _check(got, P['want']['learn'], P, P['t']['learn'][0], f'({F}, {De}, {edge}) strided x_src')


# ---- exact, without exp ----------------------------------------------------------------------------
@pytest.mark.parametrize('F,De,edge', [(24, 0, True), (24, 3, True), (20, 0, False)])
def test_one_slot_per_destination_is_exact(dev, F, De, edge):
    """In-degree 0 or 1: alpha = 1, so out is the float32 message (or zeros) and the gradients are
    the masked grad_out, bit for bit; with one slot m = out, so semi_grad and the full gradient
    coincide (compared separately)."""
    n_src, n_dst = 700, 900
    g = gen(21)
    dst = torch.randperm(n_dst, generator=g)[:600]
    ei = torch.stack([torch.randint(0, n_src, (600, ), generator=g), dst])
    P = _problem(n_src, n_dst, ei, F, De, 22, edge=edge)
    m, pre = R.gen_message(P['x'], P['a'], P['W'], P['b'], ei[0])
    out = torch.zeros(n_dst, F).index_copy(0, dst, m)
    gm = P['go'][dst] * (pre > 0)
    gx = torch.zeros(n_src, F).index_add(0, ei[0], gm)            # (dyadic: exact in any order)
    for kind in ('1', '-2', 'semi'):
        got, _ = _device_run(P, dev, *_t(kind, F))
        assert torch.equal(got[0].cpu(), out), f'{kind}: out'
        assert torch.equal(got[1].cpu(), gx), f'{kind}: grad_x_src'
        if De:
            assert torch.equal(got[2].cpu(), gm @ P['W']), f'{kind}: grad_edge_attr'
            assert torch.equal(got[3].cpu(), gm.t() @ P['a']) and torch.equal(got[4].cpu(), gm.sum(0))
        elif edge:
            assert torch.equal(got[2].cpu(), gm), f'{kind}: grad_edge_attr'
    got, _ = _device_run(P, dev, *_t('learn', F))                  # S2 = out^2: no gradient for t
    assert float(got[5].abs().max()) <= 1e-3 and torch.equal(got[0].cpu(), out)


# ---- a large temperature ------------------------------------------------------------------------------
@pytest.mark.parametrize('De', [0, 3])
def test_large_temperature(dev, De):
    """t = 50 with messages up to about 4: exp(t m) overflows float32 without the running maximum."""
    P = _problem(2000, 2000, T._uniform_graph(), 24, De, 31)
    m, _ = R.gen_message(P['x'], P['a'], P['W'], P['b'], P['ei'][0])
    assert 3.5 <= float(m.max()) <= 8 and 50 * float(m.max()) > 88.8
    for t, learned in ((torch.tensor([50.0]), True), (torch.full((24, ), -50.0), False)):
        got, _ = _device_run(P, dev, t, learned, False)
        assert all(bool(torch.isfinite(v).all()) for v in got if v is not None)
        _check(got, _reference(P, t, learned, False), P, t, f'De = {De} t = {float(t[0])}')


# ---- prefix, empty rows, no edges -------------------------------------------------------------------
@pytest.mark.parametrize('F,De,edge', [(24, 0, True), (24, 3, True), (24, 0, False)])
def test_destinations_a_prefix_empty_rows_and_no_edges(dev, F, De, edge):
    from pytorch_geometric_amd.nn import GENConv
    ei = random_graph(900, 300, 5000, 43)
    ei = ei[:, (ei[1] % 7 != 0) & (ei[0] % 5 != 0)]
    P = _problem(900, 300, ei, F, De, 11, edge=edge)
    t = _t('learn', F)
    got, _ = _device_run(P, dev, *t)
    _check(got, _reference(P, *t), P, t[0], f'prefix ({F}, {De})')
    assert got[0].shape == (300, F) and got[1].shape == (900, F)
    empty_dst = torch.bincount(ei[1], minlength=300) == 0
    empty_src = torch.bincount(ei[0], minlength=900) == 0
    assert int(empty_dst.sum()) >= 40 and int(empty_src.sum()) >= 180
    assert float(got[0].cpu()[empty_dst].abs().max()) == 0.0      # exact zeros
    assert float(got[1].cpu()[empty_src].abs().max()) == 0.0
    # the layer: destinations (an EdgeIndex with 300 of them) are a prefix of x's 900 rows
    from pytorch_geometric_amd import as_edge_index
    if not De:
        torch.manual_seed(5)
        conv = GENConv(F, F, norm='layer').to(dev)
        x = P['x'].to(dev)
        a = None if P['a'] is None else P['a'].to(dev)
        y = conv(x, as_edge_index(ei.to(dev), 900, 300), edge_attr=a)
        agg, _ = _device_run(P, dev, *_t('1', F))
        assert y.shape == (300, F)
        assert_close(y, conv.mlp(agg[0] + x[:300]), what='prefix layer')
    # no edges at all
    Z = _problem(50, 40, torch.zeros(2, 0, dtype=torch.int64), F, De, 12, edge=edge)
    got, _ = _device_run(Z, dev, *t)
    assert got[0].shape == (40, F) and float(got[0].abs().max()) == 0.0
    assert got[1].shape == (50, F) and float(got[1].abs().max()) == 0.0
    assert float(got[5].abs().max()) == 0.0
    if edge or De:
        assert got[2].shape == (0, De or F)
    if De:
        assert float(got[3].abs().max()) == 0.0 and float(got[4].abs().max()) == 0.0


# ---- long rows ------------------------------------------------------------------------------------
_LONG = {}


def _long_case(De, exact=True):
    """the graph of test_gpu_transformer._long_problem (a 6000-slot destination, one of threshold +
    1 slots, a 2000-slot source) at F = 64, with a learned value of t per channel"""
    key = (De, exact)
    if key not in _LONG:
        ei = T._long_problem()['ei']
        P = _problem(3000, 3000, ei, 64, De, 57 + De, exact=exact)
        P['t'] = _t('channels', 64, 5)
        P['want'] = _reference(P, *P['t'])
        _LONG[key] = P
    return _LONG[key]


@pytest.mark.parametrize('De', [0, 6])
def test_long_rows_are_chunked_and_within_the_bounds(dev, monkeypatch, De):
    from pytorch_geometric_amd import _native
    P = _long_case(De)
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    got, graph = _device_run(P, dev, *P['t'])
    torch.cuda.synchronize()
    monkeypatch.undo()
    P['graph'] = graph
    ptr = graph.by_dst().ptr
    assert int(ptr[6] - ptr[5]) == 6000 and int(ptr[12] - ptr[11]) == _native.HUB_THRESHOLD + 1
    _check(got, P['want'], P, P['t'][0], f'long rows De = {De}')
    info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'gen'}
    assert set(info) == {'forward', 'backward'}
    chunk = _native.HUB_CHUNK
    want = -(-6000 // chunk) + -(-(_native.HUB_THRESHOLD + 1) // chunk)
    assert info['forward']['n_hub'] == 2 and info['forward']['n_chunks'] == want
    assert info['backward']['n_hub'] == 1                       # source 7
    for rec in info.values():
        assert rec['F'] == 64 and rec['De'] == De and rec['grad_t'] is True
    assert info['backward']['grad_edge_attr'] is True


@pytest.mark.parametrize('De', [0, 6])
def test_two_runs_are_bitwise_identical(dev, De):
    """No float atomics anywhere and a grid that depends on the problem only: every output and
    gradient, grad_t and grad_W from the per-workgroup partials included, repeats bit for bit on
    random inputs, long rows included — and stays within the bounds."""
    P = _long_case(De, exact=False)
    a, graph = _device_run(P, dev, *P['t'])
    P['graph'] = graph
    b, _ = _device_run(P, dev, *P['t'])
    for name, x, y in zip(NAMES, a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y), f'De = {De}: {name} differs between two runs'
    assert_close_scaled(a[0], P['want'][0].float(), tol=TOL, what='random long rows out')


# ---- non-finite inputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize('t0', [1.0, -2.0])
def test_non_finite_inputs(dev, t0):
    """+inf and NaN planted in single (source, column) entries poison exactly the (destination,
    column) entries the torch composition poisons; every other entry still matches."""
    G = R.load_golden()
    ei = G['edge_index']
    x = G['x'].detach().clone()
    x[3, 2], x[17, 5], x[40, 11] = float('inf'), float('nan'), float('inf')
    P = {'x': x, 'a': None, 'W': None, 'b': None, 'ei': ei, 'n_dst': 48, 'F': 16, 'De': 0,
         'go': torch.zeros(48, 16)}
    t = torch.tensor([t0])
    want = R.gen_aggregate(x, None, None, None, t, ei, 48)
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import GenAggregateFunction
    graph = as_edge_index(ei.to(dev), 48, 48)
    got = GenAggregateFunction.apply(x.to(dev), None, None, None, t.to(dev), graph, 48).cpu()
    assert int(want.isnan().sum()) >= 3
    assert torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    assert_close(got[ok], want[ok], what='the entries that stay finite')


# ---- edge_attr without a gradient -----------------------------------------------------------------------
def test_without_a_gradient_for_edge_attr(dev, monkeypatch):
    from pytorch_geometric_amd import _native
    for P in (_uniform_case(24, 0), _uniform_case(64, 7), _long_case(6)):
        t = P['t'] if isinstance(P['t'], tuple) else P['t']['channels']
        full, _ = _device_run(P, dev, *t)
        sink = []
        monkeypatch.setattr(_native, 'timing_sink', sink)
        lean, _ = _device_run(P, dev, *t, edge_grad=False)
        torch.cuda.synchronize()
        monkeypatch.undo()
        rec = [i for i, _, _ in sink if i.get('kind') == 'gen' and i['op'] == 'backward']
        assert len(rec) == 1 and rec[0]['grad_edge_attr'] is False
        assert lean[2] is None and full[2] is not None
        for name, x, y in zip(NAMES, lean, full):
            if name != 'grad_edge_attr' and y is not None:
                assert torch.equal(x, y), f'{name} differs without grad_edge_attr'


# ---- nothing of size E x F --------------------------------------------------------------------------
@pytest.mark.parametrize('De', [8, 0])
def test_keeps_nothing_of_edge_times_width(dev, De):
    """Above the inputs: out, the saved planes, the packed rows, grad_x (2 MiB each), the fp64
    reduction of grad_t, grad_edge_attr (8 MiB) and the per-workgroup partials — far below ONE
    [E, F] tensor."""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import GenAggregateFunction
    N, E, F = 4096, 262144, 128
    graph = as_edge_index(random_graph(N, N, E, 71).to(dev), N, N)
    graph.fill_cache_()
    g = gen(72)
    x = torch.randn(N, F, generator=g).to(dev).requires_grad_(True)
    leaves = [x]
    a = W = b = None
    if De:
        a = torch.randn(E, De, generator=g).to(dev).requires_grad_(True)
        W = torch.randn(F, De, generator=g).to(dev).requires_grad_(True)
        b = torch.randn(F, generator=g).to(dev).requires_grad_(True)
        leaves += [a, W, b]
    t = torch.ones(F).to(dev).requires_grad_(True)
    go = torch.randn(N, F, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = GenAggregateFunction.apply(x, a, W, b, t, graph, N)
    grads = torch.autograd.grad(out, leaves + [t], go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'De = {De}: peak above the inputs: {extra / 2 ** 20:.1f} MiB')
    assert extra < E * F * 4 // 2                              # 64 MiB; one [E, F] is 128 MiB
    assert all(bool(torch.isfinite(v).all()) for v in grads)


# ---- routing --------------------------------------------------------------------------------------------
def _layer64(conv, x, x_dst, a, ei, n_dst, aggr='softmax'):
    """GENConv (in = out channels, norm = 'layer', no msg_norm) in float64 from its state dict"""
    p = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
    W, b = p.get('lin_edge.weight'), p.get('lin_edge.bias')
    m, _ = R.gen_message(x, a, W, b, ei[0])
    F = x.size(1)
    outs = []
    for name in ([aggr] if isinstance(aggr, str) else aggr):
        if name == 'softmax':
            outs.append(R.segment_softmax_sum(m, p.get('aggr_module.t', 1.0), ei[1], n_dst)[0])
        elif name == 'mean':
            s = m.new_zeros(n_dst, F).index_add(0, ei[1], m)
            outs.append(s / torch.bincount(ei[1], minlength=n_dst).clamp(min=1).view(-1, 1))
        elif name == 'powermean':
            q = p['aggr_module.p']
            s = m.new_zeros(n_dst, F).index_add(0, ei[1], m.clamp(1e-4, 100.).pow(q))
            s = s / torch.bincount(ei[1], minlength=n_dst).clamp(min=1).view(-1, 1)
            outs.append(s.clamp(1e-4, 100.).pow(1 / q))
    h = torch.cat(outs, dim=1)
    if 'lin_aggr_out.weight' in p:
        h = h @ p['lin_aggr_out.weight'].t()
    h = h + x_dst[:n_dst]
    h = h @ p['mlp.0.weight'].t()
    h = torch.nn.functional.layer_norm(h, (h.size(1), ), p['mlp.1.weight'], p['mlp.1.bias'])
    return h.relu() @ p['mlp.4.weight'].t()


def _layer_problem(F, De, device, seed, edge=True, **kw):
    from pytorch_geometric_amd.nn import GENConv
    torch.manual_seed(seed)
    conv = GENConv(F, F, norm='layer', edge_dim=De or None, bias=False, **kw)
    P = _problem(300, 300, random_graph(300, 300, 3000, 91), F, De, seed + 1, edge=edge)
    if De:
        conv.lin_edge.weight.data.copy_(P['W'])
        P['b'] = None
    return conv.to(device), P


def test_routing(dev, monkeypatch):
    """Layouts outside the envelope, target_to_source, other aggregations, a list of them,
    ``fuse = False`` and host tensors take the generic or the host route and match float64; the
    supported layer takes the new route."""
    for what, F, De, kw, device in (
            ('F * De = 8192', 512, 16, {}, dev),
            ('F = 1024', 1024, 0, {}, dev),
            ('target_to_source', 24, 3, dict(flow='target_to_source'), dev),
            ('powermean', 24, 3, dict(aggr='powermean', p=1.5, learn_p=True), dev),
            ('list', 24, 3, dict(aggr=['softmax', 'mean']), dev),
            ('fuse = False', 24, 3, {}, dev),
            ('host tensors', 24, 3, dict(learn_t=True, t=0.6), 'cpu'),
            ('supported', 24, 3, dict(learn_t=True, t=0.6), dev),
            ('supported wide', 24, 0, {}, dev)):
        conv, P = _layer_problem(F, De, device, 9, **kw)
        if what == 'fuse = False':
            conv.fuse = False
        if what == 'list':
            assert conv.lin_aggr_out.weight.shape == (24, 48)
        ei = P['ei']
        x = P['x'].to(device).requires_grad_(True)
        a = P['a'].to(device).requires_grad_(True)
        state = {}

        def step():
            state['out'] = conv(x, ei.to(device), edge_attr=a)
            state['grad'] = torch.autograd.grad(state['out'].sum(), [x, a])

        c = T._counted(monkeypatch, step)
        fused = sorted(n for n in c.calls if n in ('pygamd_gen_forward', 'pygamd_gen_backward'))
        if what.startswith('supported'):
            assert fused == ['pygamd_gen_backward', 'pygamd_gen_forward'], (what, c.calls)
        else:
            assert not fused, (what, c.calls)
        x64, a64 = P['x'].double().requires_grad_(True), P['a'].double().requires_grad_(True)
        flipped = kw.get('flow') == 'target_to_source'     # the roles of the two rows swap
        want = _layer64(conv, x64, x64, a64, ei.flip(0) if flipped else ei, 300,
                        aggr=kw.get('aggr', 'softmax'))
        assert_close_scaled(state['out'], want.detach().float(), tol=TOL, what=f'{what} out')
        for n, g, w in zip(('grad_x', 'grad_edge_attr'), state['grad'],
                           torch.autograd.grad(want.sum(), [x64, a64])):
            assert_close_scaled(g, w.float(), tol=TOL, what=f'{what} {n}')


def test_half_inputs_are_widened(dev):
    from pytorch_geometric_amd.nn import GENConv
    for edge_dim in (None, 4):
        torch.manual_seed(4)
        conv = GENConv(16, 16, edge_dim=edge_dim, norm='layer').to(dev)
        x = torch.randn(300, 16, generator=gen(94)).to(dev)
        ei = random_graph(300, 300, 3000, 95).to(dev)
        ea = torch.randn(3000, edge_dim or 16, generator=gen(98)).to(dev)
        want = conv(x, ei, ea)
        got = conv.half()(x.half(), ei, ea.half())
        assert got.dtype == torch.float16
        assert_close_scaled(got.float(), want, tol=2e-2, what=f'half edge_dim = {edge_dim}')


def test_inside_hetero_conv_with_edge_attr_dict(dev, monkeypatch):
    from pytorch_geometric_amd.nn import GENConv, HeteroConv
    torch.manual_seed(6)
    layer = GENConv(16, 16, edge_dim=3, norm='layer', learn_t=True, t=0.8)
    hetero = HeteroConv({('a', 'to', 'b'): layer}).to(dev)
    ei = random_graph(400, 150, 2500, 97)
    P = _problem(400, 150, ei, 16, 3, 96)
    layer.lin_edge.weight.data.copy_(P['W'])
    xb0 = _grid(gen(99), -16, 17, (150, 16), 8)
    xa, xb = P['x'].to(dev).requires_grad_(True), xb0.to(dev).requires_grad_(True)
    ead = P['a'].to(dev).requires_grad_(True)
    state = {}

    def step():
        state['out'] = hetero({'a': xa, 'b': xb}, {('a', 'to', 'b'): ei.to(dev)},
                              edge_attr_dict={('a', 'to', 'b'): ead})

    c = T._counted(monkeypatch, step)
    assert c.calls.get('pygamd_gen_forward') == 1, c.calls
    out = state['out']
    assert set(out) == {'b'} and out['b'].shape == (150, 16)
    grads = torch.autograd.grad(out['b'].sum(), [xa, xb, ead])
    leaves = [v.double().requires_grad_(True) for v in (P['x'], xb0, P['a'])]
    want = _layer64(layer, leaves[0], leaves[1], leaves[2], ei, 150)
    assert_close_scaled(out['b'], want.detach().float(), tol=TOL, what='hetero out')
    for name, got, ref in zip(('grad a', 'grad b', 'grad edge_attr'), grads,
                              torch.autograd.grad(want.sum(), leaves)):
        assert_close_scaled(got, ref.float(), tol=TOL, what=f'hetero {name}')


# ---- the registered operator ------------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'gen_aggregate' in ops.OPS and 'gen_aggregate_backward' in ops.OPS
    op = torch.ops.pyg_amd.gen_aggregate
    with FakeTensorMode():
        x = torch.empty(50, 24, device='cuda', requires_grad=True)
        a = torch.empty(400, 5, device='cuda')
        W = torch.empty(24, 5, device='cuda')
        b = torch.empty(24, device='cuda')
        t = torch.empty(24, device='cuda', requires_grad=True)
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        eid = torch.empty(400, dtype=torch.int32, device='cuda')
        for args, planes in (((x, a, W, b, t, ptr, col, eid, 1e-7, False, True), 3),
                             ((x, None, None, None, t.detach()[:1], ptr, col, None), 2)):
            out, saved = op(*args)
            assert out.shape == (12, 24) and out.requires_grad and saved.shape == (planes, 12, 24)
            assert out.device.type == 'cuda' and out.dtype == saved.dtype == torch.float32

    P = _uniform_case(64, 7)
    t0, want = P['t']['channels'][0], P['want']['channels']
    order = torch.argsort(P['ei'][1], stable=True)
    col = P['ei'][0][order].to(dev)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], 2000).to(dev)
    eid = order.to(dev)                 # slot -> the caller's edge: edge_attr stays in COO order
    go = P['go'].to(dev)

    def fn(x, a, W, b, t):
        return (op(x * 1.0, a, W, b, t, ptr, col, eid, 1e-7, False, True)[0] * go).sum()

    def leaves():
        return [v.to(dev).requires_grad_(True) for v in (P['x'], P['a'], P['W'], P['b'], t0)]

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        y = f(*ls)
        results.append([y.detach()] + list(torch.autograd.grad(y, ls)))
    for x, y in zip(*results):
        assert_close(y, x, what='compiled vs eager')
    ls = [v.detach() for v in leaves()]
    out = op(*ls, ptr, col, eid)[0]
    _check([out] + results[0][1:], want, P, t0, 'operator')
    # edge_id = None: edge_attr follows the slots of col
    ls[1] = ls[1][eid]
    assert torch.equal(op(*ls, ptr, col, None)[0], out)
    torch.library.opcheck(op, (*leaves(), ptr, col, eid, 1e-7, False, True))
    torch.library.opcheck(op, (leaves()[0], None, None, None, t0[:1].to(dev), ptr, col, None))
