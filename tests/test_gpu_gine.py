"""nn.GINConv / nn.GINEConv on the device: the recorded reference cases with their launch counts,
the kernel pair of csrc/gine.hip against the float64 restatement of the node (tests/_gin_ref.py)
on inputs that make every sum EXACT in float32 (so ``torch.equal`` is the check and no ReLU mask
can flip), long rows through the chunked schedule, bitwise repeatability, the memory promise,
routing, half inputs, HeteroConv and the registered operator.  Nothing here reads the reference
tree.

Exact inputs (a dyadic grid): ``x``, ``grad_out`` = randint(-16, 17) / 8; ``eps`` = 0.25; wide
``edge_attr`` = randint(-16, 17) / 8 + 1/16; linear ``edge_attr`` and ``W`` = randint(-4, 5) / 4,
``b`` = randint(-8, 9) / 8 + 1/16.  Every product and partial sum is then a multiple of 1/32 (1/64
for ``grad_eps``) that float32 holds exactly as long as it stays below 2^24 units; ``_dyadic``
asserts that from the problem's sizes and these ranges."""
import pytest
import torch

import _gin_ref as R
import test_gpu_transformer as T
from _util import assert_close, assert_close_scaled, gen, random_graph

pytestmark = pytest.mark.gpu

NAMES = ('out', 'grad_x_src', 'grad_x_root', 'grad_eps', 'grad_edge_attr', 'grad_W', 'grad_b')


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_the_fused_route(dev, monkeypatch, name, index_dtype):
    """GINEConv: ONE forward and ONE backward launch of the new pair and nothing else that touches
    the edges.  GINConv: the CSR sum SpMM (its forward first, over the destinations), no gine
    call."""
    sink = []
    c = T._counted(monkeypatch, lambda: R.check_class_case(R.load_golden(), name, dev,
                                                           index_dtype=index_dtype), sink=sink)
    if name.startswith('gine'):
        assert c.calls.get('pygamd_gine_forward') == 1, c.calls
        assert c.calls.get('pygamd_gine_backward') == 1, c.calls
        assert not [n for n in c.calls if 'spmm' in n or 'scatter' in n or 'sddmm' in n
                    or 'softmax' in n], c.calls
        assert not [i for i, _, _ in sink if 'reduce' in i], sink
    else:
        assert not [n for n in c.calls if 'gine' in n], c.calls
        spmm = [i for i, _, _ in sink if 'reduce' in i]
        n_dst = R.load_golden()['cases'][name]['out'].size(0)
        # the forward over the destinations, then the same kernel on the transposed handle
        assert [i['reduce'] for i in spmm] == ['sum', 'sum'], spmm
        assert spmm[0]['n_rows'] == n_dst and spmm[0]['F'] == 16 and not spmm[0]['weighted']


# ---- problems ---------------------------------------------------------------------------------------
def _grid(g, lo, hi, shape, div, shift=0.0):
    return torch.randint(lo, hi, shape, generator=g).float() / div + shift


def _dyadic(n_src, n_dst, ei, F, De, seed, root_rows=None):
    """A problem on the dyadic grid of the module docstring, with the exactness of every result
    asserted from its sizes: the largest value a sum can reach over its granularity < 2^24."""
    g = gen(seed)
    E = ei.size(1)
    P = {'x': _grid(g, -16, 17, (n_src, F), 8), 'go': _grid(g, -16, 17, (n_dst, F), 8),
         'xr': _grid(g, -16, 17, (root_rows or n_dst, F), 8), 'eps': torch.tensor([0.25]),
         'ei': ei, 'n_dst': n_dst, 'F': F, 'De': De}
    if De == 0:
        P['a'] = _grid(g, -16, 17, (E, F), 8, 1 / 16)
        P['W'] = P['b'] = None
        e_max = 2 + 1 / 16
        # x is a multiple of 2/16, the edge term of 2/16 plus 1/16: never zero
        assert bool(((P['x'][ei[0]] + P['a']) * 16 % 2 == 1).all())
    else:
        P['a'] = _grid(g, -4, 5, (E, De), 4)
        P['W'] = _grid(g, -4, 5, (F, De), 4)
        P['b'] = _grid(g, -8, 9, (F, ), 8, 1 / 16)
        e_max = De * 1.0 + 1 + 1 / 16                 # |W a + b|, a multiple of 1/16
    in_deg = int(torch.bincount(ei[1], minlength=n_dst).max()) if E else 0
    out_deg = int(torch.bincount(ei[0], minlength=n_src).max()) if E else 0
    limit = 2 ** 24
    assert (in_deg * (2 + e_max) + 1.25 * 2) * 32 < limit        # out: multiples of 1/32
    assert out_deg * 2 * 8 < limit                               # grad_x_src: of 1/8
    assert F * 2 * 1 * 32 < limit                                # grad_edge_attr (linear): of 1/32
    assert E * 2 * 1 * 32 < limit                                # grad_W: of 1/32; grad_b: of 1/8
    assert F * 2 * 2 * 64 < limit                                # a row of <grad_out, x_root>: 1/64
    return P


def _random(n_src, n_dst, ei, F, De, seed):
    g = gen(seed)
    E = ei.size(1)
    P = {'x': torch.randn(n_src, F, generator=g), 'go': torch.randn(n_dst, F, generator=g),
         'xr': torch.randn(n_dst, F, generator=g), 'eps': torch.tensor([0.25]), 'ei': ei,
         'n_dst': n_dst, 'F': F, 'De': De, 'W': None, 'b': None}
    if De == 0:
        P['a'] = torch.randn(E, F, generator=g)
    else:
        P['a'] = torch.randn(E, De, generator=g)
        P['W'] = torch.randn(F, De, generator=g) / De ** 0.5
        P['b'] = torch.randn(F, generator=g)
    return P


def _reference(P, root=True, dtype=torch.float64):
    """the seven of NAMES from the restatement (None where an input is absent), as float32"""
    x, a = [P[n].to(dtype).requires_grad_(True) for n in ('x', 'a')]
    xr, eps = [P[n].to(dtype).requires_grad_(True) if root else None for n in ('xr', 'eps')]
    W, b = [None if P[n] is None else P[n].to(dtype).requires_grad_(True) for n in ('W', 'b')]
    out = R.gine_aggregate(x, xr, eps, a, W, b, P['ei'], P['n_dst'])
    leaves = [t for t in (x, xr, eps, a, W, b) if t is not None]
    grads = dict(zip([id(t) for t in leaves],
                     torch.autograd.grad(out, leaves, P['go'].to(dtype), allow_unused=True)))
    res = [out.detach()] + [None if t is None else grads[id(t)] for t in (x, xr, eps, a, W, b)]
    if E0(P):  # no edge: autograd leaves the unused edge inputs without a gradient
        res = [r if r is not None or t is None else torch.zeros_like(t)
               for r, t in zip(res, (out, x, xr, eps, a, W, b))]
    return [None if r is None else r.detach().float() for r in res]


def E0(P):
    return P['ei'].size(1) == 0


def _device_run(P, dev, index_dtype=torch.int64, root=True, edge_grad=True, strided=False):
    """the same seven through the autograd node, and the handle"""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import GineAggregateFunction
    F = P['F']
    if strided:   # the right half of a [n, 2 F] tensor, read in place
        wide = torch.zeros(P['x'].size(0), 2 * F)
        wide[:, F:] = P['x']
        x = wide.to(dev)[:, F:].detach().requires_grad_(True)
        assert x.stride(0) == 2 * F
    else:
        x = P['x'].to(dev).requires_grad_(True)
    a = P['a'].to(dev).requires_grad_(edge_grad)
    xr, eps = [P[n].to(dev).requires_grad_(True) if root else None for n in ('xr', 'eps')]
    W, b = [None if P[n] is None else P[n].to(dev).requires_grad_(True) for n in ('W', 'b')]
    graph = P.get('graph')
    if graph is None or graph.edge_index.dtype != index_dtype:
        graph = as_edge_index(P['ei'].to(dev).to(index_dtype), P['x'].size(0), P['n_dst'])
    out = GineAggregateFunction.apply(x, xr, eps, a, W, b, graph, P['n_dst'])
    leaves = [t for t in (x, xr, eps, a, W, b) if t is not None and t.requires_grad]
    grads = dict(zip([id(t) for t in leaves], torch.autograd.grad(out, leaves, P['go'].to(dev))))
    return [out.detach()] + [grads.get(id(t)) for t in (x, xr, eps, a, W, b)], graph


def _assert_exact(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, f'{what}: {name} should be absent'
            continue
        assert g is not None and g.shape == w.shape, f'{what}: {name} shape'
        assert torch.equal(g.cpu(), w), \
            f'{what}: {name} is not exact (max abs err {float((g.cpu() - w).abs().max()):.3e})'


# ---- the kernels are exact ------------------------------------------------------------------------
_UNIFORM = {}


def _uniform_case(F, De):
    """problem and float64 results at one shape, computed once for both index dtypes"""
    if (F, De) not in _UNIFORM:
        P = _dyadic(2000, 2000, T._uniform_graph(), F, De, 300 + F + 7 * De)
        _UNIFORM[(F, De)] = (P, _reference(P, root=True), _reference(P, root=False))
    return _UNIFORM[(F, De)]


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('F,De', [(1, 0), (5, 0), (24, 0), (64, 0), (100, 0), (128, 0), (512, 0),
                                  (8, 1), (24, 3), (64, 7), (100, 4), (128, 32), (256, 16),
                                  (512, 8)])
def test_kernels_are_exact(dev, F, De, index_dtype):
    """Wide F below one lane group, odd, the float4 widths and the limit; linear (F, De) through
    every register capacity for De and both limits (F * De = 4096 three ways); with and without
    the self term; x_src as a column block of a wider tensor (row stride 2 F)."""
    P, want_root, want_bare = _uniform_case(F, De)
    got, graph = _device_run(P, dev, index_dtype)
    P['graph'] = graph
    _assert_exact(got, want_root, f'({F}, {De})')
    got, _ = _device_run(P, dev, index_dtype, root=False)
    _assert_exact(got, want_bare, f'({F}, {De}) without x_root')
    got, _ = _device_run(P, dev, index_dtype, strided=True)
    _assert_exact(got, want_root, f'({F}, {De}) strided x_src')


@pytest.mark.parametrize('F,De', [(24, 0), (24, 3)])
def test_destinations_a_prefix_empty_rows_and_no_edges(dev, F, De):
    ei = random_graph(900, 300, 5000, 43)
    ei = ei[:, (ei[1] % 7 != 0) & (ei[0] % 5 != 0)]
    P = _dyadic(900, 300, ei, F, De, 11, root_rows=900)      # x_root longer than the destinations
    got, _ = _device_run(P, dev)
    _assert_exact(got, _reference(P), f'prefix ({F}, {De})')
    assert got[0].shape == (300, F) and got[2].shape == (900, F)
    assert float(got[2][300:].abs().max()) == 0.0
    empty_dst = torch.bincount(ei[1], minlength=300) == 0
    empty_src = torch.bincount(ei[0], minlength=900) == 0
    assert int(empty_dst.sum()) >= 40 and int(empty_src.sum()) >= 180
    # a destination without a slot is exactly its self term, a source without one gets exact zeros
    assert torch.equal(got[0].cpu()[empty_dst], (1.25 * P['xr'][:300])[empty_dst])
    assert float(got[1].cpu()[empty_src].abs().max()) == 0.0
    # no edges at all
    Z = _dyadic(50, 40, torch.zeros(2, 0, dtype=torch.int64), F, De, 12)
    got, _ = _device_run(Z, dev)
    _assert_exact(got, _reference(Z), f'no edges ({F}, {De})')
    assert torch.equal(got[0].cpu(), 1.25 * Z['xr'])
    assert got[1].shape == (50, F) and float(got[1].abs().max()) == 0.0
    assert got[4].shape == (0, De or F)
    if De:
        assert float(got[5].abs().max()) == 0.0 and float(got[6].abs().max()) == 0.0


# ---- long rows ------------------------------------------------------------------------------------
_LONG = {}


def _long_case(De, exact=True):
    """the graph of test_gpu_transformer._long_problem (a 6000-slot destination, one of threshold +
    1 slots, a 2000-slot source) at F = 64"""
    key = (De, exact)
    if key not in _LONG:
        ei = T._long_problem()['ei']
        P = (_dyadic if exact else _random)(3000, 3000, ei, 64, De, 57 + De)
        P['want'] = _reference(P)
        _LONG[key] = P
    return _LONG[key]


@pytest.mark.parametrize('De', [0, 6])
def test_long_rows_are_exact_and_chunked(dev, monkeypatch, De):
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
    _assert_exact(got, P['want'], f'long rows De = {De}')
    info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'gine'}
    assert set(info) == {'forward', 'backward'}
    chunk = _native.HUB_CHUNK
    want = -(-6000 // chunk) + -(-(_native.HUB_THRESHOLD + 1) // chunk)
    assert info['forward']['n_hub'] == 2 and info['forward']['n_chunks'] == want
    assert info['backward']['n_hub'] == 1                       # source 7
    for rec in info.values():
        assert rec['F'] == 64 and rec['De'] == De
    assert info['backward']['grad_edge_attr'] is True


@pytest.mark.parametrize('De', [0, 6])
def test_two_runs_are_bitwise_identical(dev, De):
    """No float atomics anywhere and a grid that depends on the problem only: every output and
    gradient, grad_W and grad_b from the per-workgroup partials included, repeats bit for bit on
    random inputs, long rows included."""
    P = _long_case(De, exact=False)
    a, graph = _device_run(P, dev)
    P['graph'] = graph
    b, _ = _device_run(P, dev)
    for name, x, y in zip(NAMES, a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y), f'De = {De}: {name} differs between two runs'


def test_random_inputs_forward_matches_float64(dev):
    cases = [_random(2000, 2000, T._uniform_graph(), 64, 0, 71),
             _random(2000, 2000, T._uniform_graph(), 100, 4, 72),
             _long_case(0, exact=False), _long_case(6, exact=False)]
    for P in cases:
        want = P['want'][0] if 'want' in P else _reference(P)[0]
        from pytorch_geometric_amd import as_edge_index
        from pytorch_geometric_amd._functions import GineAggregateFunction
        graph = as_edge_index(P['ei'].to(dev), P['x'].size(0), P['n_dst'])
        t = {n: (None if P[n] is None else P[n].to(dev)) for n in ('x', 'xr', 'eps', 'a', 'W', 'b')}
        out = GineAggregateFunction.apply(t['x'], t['xr'], t['eps'], t['a'], t['W'], t['b'], graph,
                                          P['n_dst'])
        assert_close_scaled(out, want, tol=2e-5, what=f"random ({P['F']}, {P['De']}) out")


def test_without_a_gradient_for_edge_attr(dev, monkeypatch):
    """``edge_attr.requires_grad == False``: the kernel is told not to compute grad_edge_attr and
    the other gradients are bitwise those of the run that does compute it."""
    from pytorch_geometric_amd import _native
    for P in (_uniform_case(24, 0)[0], _uniform_case(64, 7)[0], _long_case(6)):
        full, _ = _device_run(P, dev)
        sink = []
        monkeypatch.setattr(_native, 'timing_sink', sink)
        lean, _ = _device_run(P, dev, edge_grad=False)
        torch.cuda.synchronize()
        monkeypatch.undo()
        rec = [i for i, _, _ in sink if i.get('kind') == 'gine' and i['op'] == 'backward']
        assert len(rec) == 1 and rec[0]['grad_edge_attr'] is False
        assert lean[4] is None and full[4] is not None
        for name, x, y in zip(NAMES, lean, full):
            if name != 'grad_edge_attr' and y is not None:
                assert torch.equal(x, y), f'{name} differs without grad_edge_attr'
    # through the node itself: None comes back for edge_attr
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import GineAggregateFunction
    P = _uniform_case(64, 7)[0]
    graph = as_edge_index(P['ei'].to(dev), 2000, 2000)
    x, W = P['x'].to(dev).requires_grad_(True), P['W'].to(dev).requires_grad_(True)
    a = P['a'].to(dev)
    GineAggregateFunction.apply(x, None, None, a, W, None, graph, 2000).sum().backward()
    assert a.grad is None and x.grad is not None and W.grad is not None


# ---- nothing of size E x F --------------------------------------------------------------------------
def test_linear_mode_keeps_nothing_of_edge_times_width(dev):
    """Expected above the inputs: out (2 MiB) + grad_x (2 MiB) + grad_edge_attr (8 MiB) + the
    per-workgroup partials of (grad_W, grad_b) (a few MiB) — far below ONE [E, F] tensor."""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import GineAggregateFunction
    N, E, F, De = 4096, 262144, 128, 8
    graph = as_edge_index(random_graph(N, N, E, 71).to(dev), N, N)
    graph.fill_cache_()
    g = gen(72)
    x = torch.randn(N, F, generator=g).to(dev).requires_grad_(True)
    a = torch.randn(E, De, generator=g).to(dev).requires_grad_(True)
    W = torch.randn(F, De, generator=g).to(dev).requires_grad_(True)
    b = torch.randn(F, generator=g).to(dev).requires_grad_(True)
    eps = torch.tensor([0.1]).to(dev).requires_grad_(True)
    go = torch.randn(N, F, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = GineAggregateFunction.apply(x, x, eps, a, W, b, graph, N)
    grads = torch.autograd.grad(out, [x, eps, a, W, b], go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'peak above the inputs: {extra / 2 ** 20:.1f} MiB')
    assert extra < E * F * 4 // 2                              # 64 MiB; one [E, F] is 128 MiB
    assert all(bool(torch.isfinite(t).all()) for t in grads)


# ---- routing --------------------------------------------------------------------------------------------
def _layer_problem(F, De, device, seed, **kw):
    """a GINEConv over nn = Sequential(Linear(F, 12), ReLU, Linear(12, 8)) whose edge transform is
    dyadic like the inputs (the mask of the message is then the same in float32 and float64)"""
    from pytorch_geometric_amd.nn import GINEConv
    torch.manual_seed(seed)
    nn = torch.nn.Sequential(torch.nn.Linear(F, 12), torch.nn.ReLU(), torch.nn.Linear(12, 8))
    conv = GINEConv(nn, eps=0.25, train_eps=True, edge_dim=De or None, **kw)
    P = _dyadic(300, 300, random_graph(300, 300, 3000, 91), F, De, seed + 1)
    if De:
        conv.lin.weight.data.copy_(P['W'])
        conv.lin.bias.data.copy_(P['b'])
    return conv.to(device), P


def test_routing(dev, monkeypatch):
    """Layouts outside the envelope, target_to_source, another aggregation, ``fuse = False`` and
    host tensors take the generic or the host route and match float64; the supported layer takes
    the new route; the width mismatch raises on the device too."""
    from pytorch_geometric_amd.nn import GINEConv
    for what, F, De, kw, device in (
            ('F * De = 8192', 512, 16, {}, dev),
            ('F = 1024', 1024, 0, {}, dev),
            ('target_to_source', 24, 3, dict(flow='target_to_source'), dev),
            ('mean', 24, 3, dict(aggr='mean'), dev),
            ('fuse = False', 24, 3, {}, dev),
            ('host tensors', 24, 3, {}, 'cpu'),
            ('supported', 24, 3, {}, dev),
            ('supported wide', 24, 0, {}, dev)):
        conv, P = _layer_problem(F, De, device, 9, **kw)
        if what == 'fuse = False':
            conv.fuse = False
        ei = P['ei']
        x = P['x'].to(device).requires_grad_(True)
        a = P['a'].to(device).requires_grad_(True)
        state = {}

        def step():
            state['out'] = conv(x, ei.to(device), edge_attr=a)
            state['grad'] = torch.autograd.grad(state['out'].sum(), [x, a])

        c = T._counted(monkeypatch, step)
        fused = sorted(n for n in c.calls if n in ('pygamd_gine_forward', 'pygamd_gine_backward'))
        if what.startswith('supported'):
            assert fused == ['pygamd_gine_backward', 'pygamd_gine_forward'], (what, c.calls)
        else:
            assert not fused, (what, c.calls)
        p = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
        x64, a64 = P['x'].double().requires_grad_(True), P['a'].double().requires_grad_(True)
        flipped = kw.get('flow') == 'target_to_source'     # the roles of the two rows swap
        want = R.gine_layer(x64, x64, a64, ei.flip(0) if flipped else ei, p, 300,
                            aggr=kw.get('aggr', 'sum'))
        assert_close_scaled(state['out'], want.detach().float(), tol=2e-5, what=f'{what} out')
        for n, g, w in zip(('grad_x', 'grad_edge_attr'), state['grad'],
                           torch.autograd.grad(want.sum(), [x64, a64])):
            assert_close_scaled(g, w.float(), tol=2e-5, what=f'{what} {n}')
    conv = GINEConv(R.make_nn()).to(dev)
    with pytest.raises(ValueError, match='dimensionalities do not match'):
        conv(torch.randn(10, 16, device=dev), torch.randint(0, 10, (2, 30), device=dev),
             edge_attr=torch.randn(30, 5, device=dev))


def test_half_inputs_are_widened(dev):
    from pytorch_geometric_amd.nn import GINEConv
    for edge_dim in (None, 4):
        torch.manual_seed(4)
        conv = GINEConv(R.make_nn(), eps=0.1, edge_dim=edge_dim).to(dev)
        x = torch.randn(300, 16, generator=gen(94)).to(dev)
        ei = random_graph(300, 300, 3000, 95).to(dev)
        ea = torch.randn(3000, edge_dim or 16, generator=gen(98)).to(dev)
        want = conv(x, ei, ea)
        got = conv.half()(x.half(), ei, ea.half())
        assert got.dtype == torch.float16
        assert_close_scaled(got.float(), want, tol=2e-2, what=f'half edge_dim = {edge_dim}')


def test_inside_hetero_conv_with_edge_attr_dict(dev, monkeypatch):
    from pytorch_geometric_amd.nn import GINEConv, HeteroConv
    torch.manual_seed(6)
    layer = GINEConv(R.make_nn(), eps=0.25, train_eps=True, edge_dim=3)
    hetero = HeteroConv({('a', 'to', 'b'): layer}).to(dev)
    ei = random_graph(400, 150, 2500, 97)
    P = _dyadic(400, 150, ei, 16, 3, 96)
    layer.lin.weight.data.copy_(P['W'])
    layer.lin.bias.data.copy_(P['b'])
    xa, xb = P['x'].to(dev).requires_grad_(True), P['xr'].to(dev).requires_grad_(True)
    ead = P['a'].to(dev).requires_grad_(True)
    state = {}

    def step():
        state['out'] = hetero({'a': xa, 'b': xb}, {('a', 'to', 'b'): ei.to(dev)},
                              edge_attr_dict={('a', 'to', 'b'): ead})

    c = T._counted(monkeypatch, step)
    assert c.calls.get('pygamd_gine_forward') == 1, c.calls
    out = state['out']
    assert set(out) == {'b'} and out['b'].shape == (150, 8)
    grads = torch.autograd.grad(out['b'].sum(), [xa, xb, ead])
    p = {k: v.detach().cpu().double() for k, v in layer.state_dict().items()}
    leaves = [P[n].double().requires_grad_(True) for n in ('x', 'xr', 'a')]
    want = R.gine_layer(leaves[0], leaves[1], leaves[2], ei, p, 150)
    assert_close_scaled(out['b'], want.detach().float(), tol=2e-5, what='hetero out')
    for name, got, ref in zip(('grad a', 'grad b', 'grad edge_attr'), grads,
                              torch.autograd.grad(want.sum(), leaves)):
        assert_close_scaled(got, ref.float(), tol=2e-5, what=f'hetero {name}')


# ---- the registered operator ------------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'gine_aggregate' in ops.OPS and 'gine_aggregate_backward' in ops.OPS
    op = torch.ops.pyg_amd.gine_aggregate
    with FakeTensorMode():
        x = torch.empty(50, 24, device='cuda', requires_grad=True)
        xr = torch.empty(12, 24, device='cuda')
        eps = torch.empty(1, device='cuda')
        a = torch.empty(400, 5, device='cuda')
        W = torch.empty(24, 5, device='cuda')
        b = torch.empty(24, device='cuda')
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        eid = torch.empty(400, dtype=torch.int32, device='cuda')
        for args in ((x, xr, eps, a, W, b, ptr, col, eid), (x, None, None, a, W, None, ptr, col,
                                                            None)):
            out = op(*args)
            assert out.shape == (12, 24) and out.requires_grad
            assert out.device.type == 'cuda' and out.dtype == torch.float32

    P, want, _ = _uniform_case(64, 7)
    order = torch.argsort(P['ei'][1], stable=True)
    col = P['ei'][0][order].to(dev)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], 2000).to(dev)
    eid = order.to(dev)                 # slot -> the caller's edge: edge_attr stays in COO order
    go = P['go'].to(dev)

    def fn(x, xr, eps, a, W, b):
        return (op(x * 1.0, xr, eps, a, W, b, ptr, col, eid) * go).sum()

    def leaves():
        return [P[n].to(dev).requires_grad_(True) for n in ('x', 'xr', 'eps', 'a', 'W', 'b')]

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        y = f(*ls)
        results.append([y.detach()] + list(torch.autograd.grad(y, ls)))
    for x, y in zip(*results):
        assert_close(y, x, what='compiled vs eager')
    for name, g, w in zip(NAMES[1:], results[0][1:], want[1:]):
        assert torch.equal(g.cpu(), w), f'operator {name} is not exact'
    out = op(*[t.detach() for t in leaves()], ptr, col, eid)
    assert torch.equal(out.cpu(), want[0])
    # edge_id = None: edge_attr follows the slots of col
    ls = [t.detach() for t in leaves()]
    ls[3] = ls[3][eid]
    assert torch.equal(op(*ls, ptr, col, None).cpu(), want[0])
    torch.library.opcheck(op, (*leaves(), ptr, col, eid))
