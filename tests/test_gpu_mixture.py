"""nn.GMMConv and nn.NNConv on the device: the kernels of csrc/mixture.hip alone and
``MixtureConvFunction`` against the float64 message-first restatement (tests/_mixture_ref.py),
destinations that are a prefix, empty rows, no edges, duplicate edges, long rows through the
chunked schedule, bitwise repeatability, the memory promise, the recorded reference cases with
their launch counts, routing, the pruning by ``needs_input_grad``, half inputs and the registered
operators.  Nothing here reads the reference tree.

Figures measured on one gfx950 device are in profiles/mixture_conv.md."""
import pytest
import torch

import _mixture_ref as R
import test_gpu_transformer as T
from _util import _counted, assert_close, assert_close_scaled, gen, random_graph

pytestmark = pytest.mark.gpu

TOL = 2e-5
EXPAND, COEF = 'pygamd_mixture_expand', 'pygamd_mixture_coef_grad'
EDGE_WALKERS = ('spmm', 'scatter', 'softmax', 'gather', 'segment')


def _mixture_calls(c):
    return c.calls.get(EXPAND, 0), c.calls.get(COEF, 0)


def _no_other_edge_pass(c):
    assert not [n for n in c.calls if any(w in n for w in EDGE_WALKERS)], c.calls


# ---- the kernels alone against float64 ---------------------------------------------------------------
_KERNEL = {}


def _kernel_case(F, K):
    """inputs and float64 results (computed on the device, kept on the host) at one shape, once
    for both index dtypes: Z by destination, Z of the transposed handle and grad_coef"""
    if (F, K) not in _KERNEL:
        ei = T._uniform_graph()
        g = gen(500 + 3 * F + K)
        P = {'x': torch.randn(2000, F, generator=g), 'coef': torch.randn(ei.size(1), K, generator=g),
             'wide': torch.randn(2000, K * F, generator=g)}
        src, dst = ei[0].cuda(), ei[1].cuda()
        x, coef, wide = (P[n].cuda().double() for n in ('x', 'coef', 'wide'))
        blocks = [slice(k, min(k + 32, K)) for k in range(0, K, 32)]   # (bounds the [E, k, F] terms)
        P['z'] = torch.cat([R.expand(x, coef[:, b], src, dst, 2000) for b in blocks], 1).cpu()
        P['z_t'] = torch.cat([R.expand(x, coef[:, b], dst, src, 2000) for b in blocks], 1).cpu()
        w3 = wide.view(2000, K, F)
        P['grad_coef'] = torch.cat([R.coef_grad(w3[:, b].reshape(2000, -1), x, src, dst)
                                    for b in blocks], 1).cpu()
        _KERNEL[(F, K)] = P
    return _KERNEL[(F, K)]


_GRAPHS = {}


def _uniform_handle(dev, index_dtype):
    from pytorch_geometric_amd import as_edge_index
    if index_dtype not in _GRAPHS:
        _GRAPHS[index_dtype] = as_edge_index(T._uniform_graph().to(dev).to(index_dtype), 2000, 2000)
    return _GRAPHS[index_dtype]


def _column_block(t, dev):
    """``t`` on the device as the middle column block of a tensor three times as wide"""
    w = t.size(1)
    wide = torch.full((t.size(0), 3 * w), float('nan'))
    wide[:, w:2 * w] = t
    block = wide.to(dev)[:, w:2 * w]
    assert block.stride(0) == 3 * w
    return block


SHAPES = ([(F, K) for F in (1, 5, 64, 100, 128, 132, 256, 512) for K in (1, 3)]
          + [(F, K) for K in (2, 8, 25, 64, 65, 129, 256) for F in (16, 64)])


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('F,K', SHAPES)
def test_kernels_match_float64(dev, F, K, index_dtype):
    """F below a wave, odd, at and past every count of columns per lane and the limit, with one
    coefficient and an odd few; K at the tile sizes, between them, one past 64 and 128 and at the
    limit, at a narrow and a full-wave F.  expand over the by-destination handle and over the
    transposed one, coef_grad over the former; contiguous x, then x as a column block."""
    from pytorch_geometric_amd import _native
    P = _kernel_case(F, K)
    graph = _uniform_handle(dev, index_dtype)
    fwd, bwd = graph.by_dst(), graph.by_src()
    coef, wide = P['coef'].to(dev), P['wide'].to(dev)
    for what, x in (('', P['x'].to(dev)), (' strided', _column_block(P['x'], dev))):
        z = _native.mixture_expand(fwd.ptr, fwd.idx, fwd.perm, x, coef, hub=fwd.hub)
        assert_close_scaled(z, P['z'].float(), tol=TOL, what=f'({F}, {K}){what} expand')
        z_t = _native.mixture_expand(bwd.ptr, bwd.idx, bwd.perm, x, coef, hub=bwd.hub)
        assert_close_scaled(z_t, P['z_t'].float(), tol=TOL, what=f'({F}, {K}){what} expand_t')
        g_c = _native.mixture_coef_grad(fwd.ptr, fwd.idx, fwd.perm, wide, x, hub=fwd.hub)
        assert_close_scaled(g_c, P['grad_coef'].float(), tol=TOL, what=f'({F}, {K}){what} coef_grad')


def test_slots_in_the_callers_order_need_no_edge_id(dev):
    """``edge_id=None``: the coefficients follow the slots of ``col``"""
    from pytorch_geometric_amd import _native
    P = _kernel_case(64, 3)
    fwd = _uniform_handle(dev, torch.int64).by_dst()
    x, coef, wide = (P[n].to(dev) for n in ('x', 'coef', 'wide'))
    z = _native.mixture_expand(fwd.ptr, fwd.idx, None, x, coef[fwd.perm], hub=fwd.hub)
    assert torch.equal(z, _native.mixture_expand(fwd.ptr, fwd.idx, fwd.perm, x, coef, hub=fwd.hub))
    g_slots = _native.mixture_coef_grad(fwd.ptr, fwd.idx, None, wide, x, hub=fwd.hub)
    g_edges = _native.mixture_coef_grad(fwd.ptr, fwd.idx, fwd.perm, wide, x, hub=fwd.hub)
    assert torch.equal(g_slots, g_edges[fwd.perm])


# ---- MixtureConvFunction against float64 -----------------------------------------------------------------
NAMES = ('out', 'grad_x', 'grad_coef', 'grad_weight')


def _problem(n_src, n_dst, ei, F, K, M, seed):
    g = gen(seed)
    return {'ei': ei, 'n_src': n_src, 'n_dst': n_dst, 'F': F, 'K': K, 'M': M,
            'x': torch.randn(n_src, F, generator=g), 'coef': torch.randn(ei.size(1), K, generator=g),
            'w': torch.randn(K, F, M, generator=g) / (K * F) ** 0.5,
            'go': torch.randn(n_dst, M, generator=g)}


def _reference(P, dtype=torch.float64, device='cuda'):
    """the four of NAMES from the message-first restatement in ``dtype`` on ``device``, as CPU
    tensors"""
    x, coef, w = (P[n].to(device, dtype).clone().requires_grad_(True) for n in ('x', 'coef', 'w'))
    ei = P['ei'].to(device)
    out = R.mixture_conv(x, coef, w, ei[0], ei[1], P['n_dst'])
    if P['ei'].size(1) == 0:
        grads = [torch.zeros_like(t) for t in (x, coef, w)]
    else:
        grads = torch.autograd.grad(out, [x, coef, w], P['go'].to(device, dtype))
    return [out.detach().cpu()] + [g.detach().cpu() for g in grads]


def _device_run(P, dev, index_dtype=torch.int64, need=(True, True, True), strided=False):
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import MixtureConvFunction
    x = (_column_block(P['x'], dev) if strided else P['x'].to(dev)).detach().requires_grad_(need[0])
    coef = P['coef'].to(dev).detach().requires_grad_(need[1])
    w = P['w'].to(dev).detach().requires_grad_(need[2])
    graph = P.get('graph')
    if graph is None or graph.edge_index.dtype != index_dtype:
        graph = as_edge_index(P['ei'].to(dev).to(index_dtype), P['n_src'], P['n_dst'])
    out = MixtureConvFunction.apply(x, coef, w, graph, P['n_dst'])
    leaves = [t for t in (x, coef, w) if t.requires_grad]
    grads = dict(zip([id(t) for t in leaves], torch.autograd.grad(out, leaves, P['go'].to(dev))))
    return [out.detach()] + [grads.get(id(t)) for t in (x, coef, w)], graph


def _check(got, want, what, floor=None):
    """at the project's bound, or at ``floor[name]`` (an absolute error) where that is larger"""
    for name, g, w in zip(NAMES, got, want):
        assert g is not None, f'{what}: {name} is missing'
        g, w = g.detach().cpu(), w.float()
        assert g.shape == w.shape, f'{what} {name}: shape'
        err = float((g - w).abs().max()) if g.numel() else 0.0
        scale = max(float(w.abs().max()), 1.0) if w.numel() else 1.0
        bound = max(TOL * scale, (floor or {}).get(name, 0.0))
        print(f'{what} {name}: max abs err {err:.3e}, scale {scale:.3e}, bound {bound:.3e}')
        assert bool(torch.isfinite(g).all()) and err <= bound, \
            f'{what} {name}: max abs err {err:.3e} vs bound {bound:.3e}'


_FUNCTION = {}


def _function_case(F, K, M):
    """problem, float64 results and the floor of the bound: 4 x the error of the SAME restatement
    run in float32 on the host against float64 (the device's products sum in another order)"""
    if (F, K, M) not in _FUNCTION:
        P = _problem(2000, 2000, T._uniform_graph(), F, K, M, 700 + F + 5 * K + M)
        P['want'] = _reference(P)
        host32 = _reference(P, torch.float32, 'cpu')
        P['floor'] = {n: 4 * float((a.double() - b).abs().max())
                      for n, a, b in zip(NAMES, host32, P['want'])}
        _FUNCTION[(F, K, M)] = P
    return _FUNCTION[(F, K, M)]


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('F,K,M', [(64, 8, 48), (100, 3, 24), (16, 25, 64), (64, 65, 32),
                                   (132, 2, 200)])
def test_function_matches_float64(dev, F, K, M, index_dtype):
    """Forward and the three gradients with ``M != F``.  The bound is the project's 2e-5 of the
    tensor's largest magnitude, or 4 x the error of the float32 restatement on the host where
    that is larger.  Measured on the host (float32 restatement against float64, max abs error /
    largest magnitude) at (64, 8, 48): out 3.5e-6 / 19.2, grad_x 6.7e-6 / 15.5, grad_coef 2.7e-6
    / 13.6, grad_weight 2.4e-4 / 808; at (64, 65, 32), the longest reduction (K F = 4160): out
    3.6e-6 / 16.1, grad_x 4.5e-6 / 13.6, grad_coef 8.8e-7 / 4.0, grad_weight 3.0e-4 / 734; the
    other three shapes lie between.  Four times these errors is below 2e-5 of the scale for every
    tensor, so at these shapes the bound in force is the project's."""
    P = _function_case(F, K, M)
    got, graph = _device_run(P, dev, index_dtype=index_dtype)
    P['graph'] = graph
    _check(got, P['want'], f'({F}, {K}, {M})', P['floor'])
    got, _ = _device_run(P, dev, index_dtype=index_dtype, strided=True)
    _check(got, P['want'], f'({F}, {K}, {M}) strided', P['floor'])


# ---- structure -----------------------------------------------------------------------------------------
def test_destinations_a_prefix_empty_rows_duplicates_and_no_edges(dev):
    """300 destinations, a prefix of 900 sources; destinations without slots get exact zeros and
    sources without slots zero gradients; every edge of a block listed twice; no edges at all."""
    ei = random_graph(900, 300, 5000, 43)
    ei = ei[:, (ei[1] % 7 != 0) & (ei[0] % 5 != 0)]
    ei = torch.cat([ei, ei[:, :700]], dim=1)                      # duplicate edges
    P = _problem(900, 300, ei, 24, 5, 40, 11)
    want = _reference(P)
    for strided in (False, True):
        got, _ = _device_run(P, dev, strided=strided)
        _check(got, want, 'prefix')
        assert got[0].shape == (300, 40) and got[1].shape == (900, 24)
        empty_dst = torch.bincount(ei[1], minlength=300) == 0
        empty_src = torch.bincount(ei[0], minlength=900) == 0
        assert int(empty_dst.sum()) >= 40 and int(empty_src.sum()) >= 180
        assert float(got[0].cpu()[empty_dst].abs().max()) == 0.0      # exact zeros
        assert float(got[1].cpu()[empty_src].abs().max()) == 0.0
    Z = _problem(50, 40, torch.zeros(2, 0, dtype=torch.int64), 24, 5, 40, 12)
    got, _ = _device_run(Z, dev)
    assert got[0].shape == (40, 40) and float(got[0].abs().max()) == 0.0
    assert got[1].shape == (50, 24) and float(got[1].abs().max()) == 0.0
    assert got[2].shape == (0, 5)
    assert got[3].shape == (5, 24, 40) and float(got[3].abs().max()) == 0.0


_LONG = {}


def _long_case():
    """the graph of test_gpu_transformer._long_problem (a 6000-slot destination, one of threshold +
    1 slots, a 2000-slot source) at F = 64, K = 5, M = 24"""
    if not _LONG:
        P = _problem(3000, 3000, T._long_problem()['ei'], 64, 5, 24, 57)
        P['want'] = _reference(P)
        host32 = _reference(P, torch.float32, 'cpu')
        P['floor'] = {n: 4 * float((a.double() - b).abs().max())
                      for n, a, b in zip(NAMES, host32, P['want'])}
        _LONG['P'] = P
    return _LONG['P']


def test_long_rows_match_float64_and_are_chunked(dev, monkeypatch):
    """The floor of the bound (4 x the float32 restatement's own error) matters here: the long
    rows' wide planes are sums of 6000 terms."""
    from pytorch_geometric_amd import _native
    P = _long_case()
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    got, graph = _device_run(P, dev)
    torch.cuda.synchronize()
    monkeypatch.undo()
    P['graph'] = graph
    ptr = graph.by_dst().ptr
    assert int(ptr[6] - ptr[5]) == 6000 and int(ptr[12] - ptr[11]) == _native.HUB_THRESHOLD + 1
    _check(got, P['want'], 'long rows', P['floor'])
    recs = [i for i, _, _ in sink if i.get('kind') == 'mixture']
    assert [r['op'] for r in recs] == ['expand', 'expand', 'coef_grad', 'expand']
    chunk = _native.HUB_CHUNK
    want = -(-6000 // chunk) + -(-(_native.HUB_THRESHOLD + 1) // chunk)
    for r in recs[:3]:                                      # the by-destination handle
        assert r['n_hub'] == 2 and r['n_chunks'] == want and r['F'] == 64 and r['K'] == 5
    assert recs[3]['n_hub'] == 1 and recs[3]['n_chunks'] >= -(-2000 // chunk)   # source 7
    assert recs[3]['F'] == 24


def test_two_runs_are_bitwise_identical(dev):
    """No float atomics and grids that depend on the problem only: every output and gradient
    repeats bit for bit, long rows included."""
    for P in (_long_case(), _function_case(64, 8, 48), _function_case(16, 25, 64)):
        a, graph = _device_run(P, dev)
        P['graph'] = graph
        b, _ = _device_run(P, dev)
        for name, x, y in zip(NAMES, a, b):
            assert torch.equal(x, y), f'{name} differs between two runs'


# ---- nothing of size E x K M ---------------------------------------------------------------------------
def test_keeps_nothing_of_edge_times_width(dev):
    """GMMConv at N = 2000, E = 200000, F = M = 64, K = 8: the fused layer's peak above the inputs
    over forward + backward stays below ONE [E, K * M] float32 tensor (390.6 MiB); the generic
    route, which forms that tensor, does not."""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd.nn import GMMConv
    N, E, F, K = 2000, 200000, 64, 8
    torch.manual_seed(3)
    conv = GMMConv(F, F, dim=2, kernel_size=K).to(dev)
    conv.sigma.data.uniform_(0.5, 1.5)
    graph = as_edge_index(random_graph(N, N, E, 71).to(dev), N, N)
    graph.fill_cache_()
    g = gen(72)
    x = torch.randn(N, F, generator=g).to(dev).requires_grad_(True)
    ea = torch.randn(E, 2, generator=g).to(dev).requires_grad_(True)
    params = list(conv.parameters())
    one = E * K * F * 4
    peaks = {}
    for fuse in (True, False):
        conv.fuse = fuse
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = conv(x, graph, ea)
        grads = torch.autograd.grad(out.sum(), [x, ea] + params)
        torch.cuda.synchronize()
        peaks[fuse] = torch.cuda.max_memory_allocated() - before
        assert all(bool(torch.isfinite(t).all()) for t in grads)
        del out, grads
    print(f'peak above the inputs: fused {peaks[True] / 2 ** 20:.1f} MiB, generic '
          f'{peaks[False] / 2 ** 20:.1f} MiB; one [E, K * M] is {one / 2 ** 20:.1f} MiB')
    assert peaks[True] < one <= peaks[False]


# ---- the recorded cases and routing -----------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_the_device(dev, monkeypatch, name, index_dtype):
    """A fused case: one expand forward; the recompute, the transposed expand and one coef_grad
    backward; nothing else that walks the edges.  ``separate_gaussians``, ``max`` and an edge
    network that ends in ReLU: the generic route, no mixture call."""
    c = _counted(monkeypatch, lambda: R.check_class_case(R.load_golden(), name, dev,
                                                         index_dtype=index_dtype))
    if name in R.FUSED_CASES:
        assert _mixture_calls(c) == (3, 1), c.calls
        _no_other_edge_pass(c)
    else:
        assert _mixture_calls(c) == (0, 0), c.calls


@pytest.mark.parametrize('name', ['gmm_defaults', 'nn_mlp'])
def test_forward_and_backward_launches(dev, monkeypatch, name):
    G = R.load_golden()
    case = G['cases'][name]
    layer = R.make_layer(case).to(dev)
    xs, ei, ea = R.case_inputs(G, case, dev)
    state = {}
    c = _counted(monkeypatch, lambda: state.update(out=layer(xs[0], ei, edge_attr=ea)))
    assert _mixture_calls(c) == (1, 0), c.calls
    _no_other_edge_pass(c)
    c = _counted(monkeypatch, lambda: state['out'].sum().backward())
    assert _mixture_calls(c) == (2, 1), c.calls
    _no_other_edge_pass(c)


def _widen_edge_network(layer):
    """the same function of ``edge_attr`` with a hidden width of 70: K' = 71 breaks the byte rule
    on this graph (71 * 48 > 400 * 8)"""
    old0, old2 = layer.nn[0], layer.nn[2]
    new0 = torch.nn.Linear(3, 70).to(old0.weight.device)
    new2 = torch.nn.Linear(70, old2.out_features).to(old0.weight.device)
    with torch.no_grad():
        new0.weight[:10], new0.bias[:10] = old0.weight, old0.bias
        new2.weight.zero_()
        new2.weight[:, :10], new2.bias[:] = old2.weight, old2.bias
    layer.nn[0], layer.nn[2] = new0, new2


@pytest.mark.parametrize('name,what', [
    ('gmm_defaults', 'fuse = False'), ('gmm_defaults', 'message hook'), ('nn_mlp', 'fuse = False'),
    ('nn_mlp', 'message hook'), ('nn_mlp', 'byte rule')])
def test_generic_routes_match_the_fixture(dev, monkeypatch, name, what):
    """``fuse = False``, a message hook (which sees the messages) and, for NNConv, an edge network
    too wide for the byte rule: no mixture call, and the recorded outputs and gradients"""
    G = R.load_golden()
    case = G['cases'][name]
    seen = []
    if what == 'byte rule':
        layer = R.make_layer(case).to(dev)
        _widen_edge_network(layer)
        assert not layer._fusable_shapes(48, 48, 400)
        xs, ei, ea = R.case_inputs(G, case, dev)
        state = {}

        def step():
            state['out'] = layer(xs[0], ei, edge_attr=ea)
            state['grads'] = torch.autograd.grad(state['out'], [xs[0], ea],
                                                 case['grad_out'].to(dev))

        c = _counted(monkeypatch, step)
        assert _mixture_calls(c) == (0, 0), c.calls
        assert_close(state['out'], case['out'], what='byte rule out')
        assert_close(state['grads'][0], case['grad_x'][0], what='byte rule grad_x')
        assert_close(state['grads'][1], case['grad_edge_attr'], atol=5e-5, rtol=5e-5,
                     what='byte rule grad_edge_attr')
        return

    def prepare(layer):
        if what == 'message hook':
            layer.register_message_forward_hook(lambda mod, args, out: seen.append(out.shape))

    c = _counted(monkeypatch, lambda: R.check_class_case(G, name, dev, fuse=what != 'fuse = False',
                                                         prepare=prepare))
    assert _mixture_calls(c) == (0, 0), c.calls
    if what == 'message hook':
        assert seen == [(400, case['out_channels'])], seen


def test_shapes_outside_the_envelope(dev, monkeypatch):
    """``kernel_size = 257`` takes the generic route, 3 the fused one; both match the float64
    restatement.  (``flow='target_to_source'`` is refused by the predicate and not run: the
    reference's own forward gathers the untransformed side there and fails in ``message``.)"""
    from pytorch_geometric_amd.nn import GMMConv
    ei = random_graph(300, 300, 3000, 91)
    from pytorch_geometric_amd.nn.conv.gmm_conv import stock_flow
    flipped = GMMConv(20, 12, dim=2, kernel_size=3, flow='target_to_source').to(dev)
    flipped.fuse = True
    assert stock_flow(flipped, GMMConv)
    assert not flipped._fusable(torch.zeros(4, 20, device=dev), None, torch.zeros(5, 2, device=dev))
    for what, K, kw in (('K = 257', 257, {}), ('supported', 3, {})):
        torch.manual_seed(9)
        conv = GMMConv(20, 12, dim=2, kernel_size=K, **kw).to(dev)
        conv.sigma.data.uniform_(0.5, 1.5)
        conv.fuse = True
        g = gen(92)
        x0, a0 = torch.randn(300, 20, generator=g), torch.randn(3000, 2, generator=g)
        x, a = x0.to(dev).requires_grad_(True), a0.to(dev).requires_grad_(True)
        state = {}

        def step():
            state['out'] = conv(x, ei.to(dev), a)
            state['grad'] = torch.autograd.grad(state['out'].sum(), [x, a])

        c = _counted(monkeypatch, step)
        assert _mixture_calls(c) == ((3, 1) if what == 'supported' else (0, 0)), (what, c.calls)
        st = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
        x64, a64 = x0.double().requires_grad_(True), a0.double().requires_grad_(True)
        want = R.gmm_layer(st, x64, x64, a64, ei, K)
        assert_close_scaled(state['out'], want.detach().float(), tol=TOL, what=f'{what} out')
        for n, got, w in zip(('grad_x', 'grad_edge_attr'), state['grad'],
                             torch.autograd.grad(want.sum(), [x64, a64])):
            assert_close_scaled(got, w.float(), tol=TOL, what=f'{what} {n}')


def test_needs_input_grad_prunes_the_backward(dev, monkeypatch):
    """``x`` without a gradient: no transposed expand; coefficients without one: no coef_grad;
    the weight without one: no recompute of the wide plane"""
    P = _function_case(64, 8, 48)
    full, graph = _device_run(P, dev)
    P['graph'] = graph
    for need, calls in (((False, True, True), (2, 1)), ((True, False, True), (3, 0)),
                        ((True, True, False), (2, 1)), ((True, False, False), (2, 0)),
                        ((False, False, True), (2, 0)), ((False, True, False), (1, 1))):
        state = {}
        c = _counted(monkeypatch, lambda: state.update(got=_device_run(P, dev, need=need)[0]))
        assert _mixture_calls(c) == calls, (need, c.calls)
        for name, wanted, x, y in zip(NAMES[1:], need, state['got'][1:], full[1:]):
            assert (x is not None) == wanted, (need, name)
            if wanted:
                assert torch.equal(x, y), f'{need}: {name} differs from the full backward'


def test_half_inputs_are_widened(dev, monkeypatch):
    """float16 and bfloat16 layers take the fused route, compute in float32 and hand the result
    back in their dtype: against the float32 layer whose parameters and inputs hold the SAME
    rounded values, the only difference is the last rounding to the low dtype, one unit in the
    last place of 2^-11 (float16) or 2^-8 (bfloat16) relative to each entry."""
    import copy
    from pytorch_geometric_amd.nn import GMMConv, NNConv
    x = torch.randn(300, 16, generator=gen(94)).to(dev)
    ei = random_graph(300, 300, 3000, 95).to(dev)
    torch.manual_seed(4)
    gmm = GMMConv(16, 16, dim=2, kernel_size=3)
    gmm.sigma.data.uniform_(0.5, 1.5)
    net = torch.nn.Sequential(torch.nn.Linear(3, 6), torch.nn.ReLU(), torch.nn.Linear(6, 256))
    for conv, width in ((gmm, 2), (NNConv(16, 16, net, aggr='mean'), 3)):
        conv = conv.to(dev)
        conv.fuse = True
        conv.bias.data.normal_(0, 0.3)
        ea = torch.randn(3000, width, generator=gen(98)).to(dev)
        for low, ulp in ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)):
            half = copy.deepcopy(conv).to(low)
            wide = copy.deepcopy(half).float()              # the rounded parameters, in float32
            xl, el = x.to(low), ea.to(low)
            if isinstance(conv, NNConv):
                # the head of the edge network is run as the user's module in its own dtype; hand
                # both routes the float32 value of what it returns
                el = el.float()
                half.nn = wide.nn
            want = wide(xl.float(), ei, el.float())
            state = {}
            c = _counted(monkeypatch, lambda: state.update(out=half(xl, ei, el)))
            assert _mixture_calls(c) == (1, 0), (low, c.calls)
            got = state['out']
            assert got.dtype == low
            assert_close(got.float(), want, rtol=ulp, atol=1e-6, what=f'{type(conv).__name__} {low}')
            xg = xl.clone().requires_grad_(True)            # the backward takes the fused route too
            c = _counted(monkeypatch, lambda: half(xg, ei, el).float().sum().backward())
            assert c.calls.get(COEF) == 1, (low, c.calls)
            assert xg.grad.dtype == low and bool(torch.isfinite(xg.grad).all())


# ---- the registered operators -----------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'mixture_conv' in ops.OPS and 'mixture_conv_backward' in ops.OPS
    op = torch.ops.pyg_amd.mixture_conv
    with FakeTensorMode():
        x = torch.empty(50, 24, device='cuda', requires_grad=True)
        coef = torch.empty(400, 5, device='cuda', requires_grad=True)
        w = torch.empty(5, 24, 7, device='cuda', requires_grad=True)
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        eid = torch.empty(400, dtype=torch.int32, device='cuda')
        for e in (eid, None):
            out = op(x, coef, w, ptr, col, e)
            assert out.shape == (12, 7) and out.requires_grad
            assert out.device.type == 'cuda' and out.dtype == torch.float32
        grads = torch.ops.pyg_amd.mixture_conv_backward(out, x, coef, w, ptr, col, eid, True,
                                                        False, True)
        assert [tuple(g.shape) for g in grads] == [(50, 24), (0, ), (5, 24, 7)]

    P = _function_case(64, 8, 48)
    want = P['want']
    order = torch.argsort(P['ei'][1], stable=True)
    col = P['ei'][0][order].to(dev)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], 2000).to(dev)
    eid = order.to(dev)                 # slot -> the caller's edge: coef stays in COO order
    go = P['go'].to(dev)

    def fn(x, coef, w):
        return (op(x * 1.0, coef, w, ptr, col, eid) * go).sum()

    def leaves():
        return [P[n].to(dev).requires_grad_(True) for n in ('x', 'coef', 'w')]

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        y = f(*ls)
        results.append([y.detach()] + list(torch.autograd.grad(y, ls)))
    for a, b in zip(*results):
        assert_close(b, a, what='compiled vs eager')
    ls = [t.detach() for t in leaves()]
    out = op(*ls, ptr, col, eid)
    _check([out] + results[0][1:], want, 'operator', P['floor'])
    # edge_id = None: coef follows the slots of col
    assert torch.equal(op(ls[0], ls[1][eid], ls[2], ptr, col, None), out)
    # a gradient that is not needed is not computed
    ls = leaves()
    ls[0] = ls[0].detach()
    y = fn(*ls)
    g_c, g_w = torch.autograd.grad(y, ls[1:])
    assert torch.equal(g_c, results[0][2]) and torch.equal(g_w, results[0][3])
    small = _problem(60, 40, random_graph(60, 40, 500, 5), 8, 3, 6, 13)
    order = torch.argsort(small['ei'][1], stable=True)
    s_col = small['ei'][0][order].to(dev)
    s_ptr = torch._convert_indices_from_coo_to_csr(small['ei'][1][order], 40).to(dev)
    args = [small[n].to(dev).requires_grad_(True) for n in ('x', 'coef', 'w')]
    torch.library.opcheck(op, (*args, s_ptr, s_col, order.to(dev)))
    torch.library.opcheck(op, (*args, s_ptr, s_col, None))
