"""nn.PNAConv / nn.aggr.DegreeScalerAggregation on the device: the recorded reference cases with
their launch counts, the kernel pair of csrc/pna.hip against the float64 restatement of the node
(tests/_pna_ref.py), empty rows, long rows through the chunked schedule, bitwise repeatability, the
accuracy of the variance, the memory promise, routing, half inputs and the registered operator.
Nothing here reads the reference tree.

The grid of the kernel tests: ``p_src``, ``p_dst`` = randint(-32, 33) / 2, ``Wc`` = randint(-2, 3),
``edge_attr`` = randint(-4, 5) / 2, so every ``u = p_src[j] + Wc a`` is a multiple of g = 1/2 and
ties in min and max are plentiful.  The variance of n such values is 0 or at least g^2 (n - 1) /
n^2 >= g^2 / n^2, which ``_dyadic`` asserts to be >= 2e-5 from the largest in-degree: no std sits
near its threshold.  Gradients are 60 * randint(-2, 3): an extremum's gradient split among up to six
tied slots stays an integer, so a run with ``min`` or ``max`` alone is exact in float32
(``torch.equal``); the number of ties is asserted from the float64 side."""
import pytest
import torch

import _pna_ref as R
import test_gpu_transformer as T
from _util import assert_close, assert_close_scaled, gen, random_graph

pytestmark = pytest.mark.gpu

FOUR = ('mean', 'min', 'max', 'std')
SETS = (('mean', ), ('min', ), ('max', ), ('std', ), FOUR)
GRADS = ('grad_p_src', 'grad_p_dst', 'grad_edge_attr', 'grad_Wc')


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_the_device(dev, monkeypatch, name, index_dtype):
    """Fused cases: ONE forward and ONE backward launch of the pair and nothing else that touches
    the edges.  The two generic cases: no pna call."""
    sink = []
    c = T._counted(monkeypatch, lambda: R.check_class_case(R.load_golden(), name, dev,
                                                           index_dtype=index_dtype), sink=sink)
    if name in R.GENERIC_CASES:
        assert not [n for n in c.calls if 'pna_forward' in n or 'pna_backward' in n], c.calls
    else:
        assert c.calls.get('pygamd_pna_forward') == 1, c.calls
        assert c.calls.get('pygamd_pna_backward') == 1, c.calls
        assert not [n for n in c.calls if 'spmm' in n or 'scatter' in n or 'sddmm' in n
                    or 'softmax' in n], c.calls
        assert not [i for i, _, _ in sink if 'reduce' in i], sink


# ---- problems ---------------------------------------------------------------------------------------
def _grid(g, lo, hi, shape, div=1.0):
    return torch.randint(lo, hi, shape, generator=g).float() / div


def _dyadic(n_src, n_dst, ei, W, De, seed, dst_rows=None):
    """A problem on the grid of the module docstring, with its two promises asserted from the
    problem's sizes"""
    g = gen(seed)
    E = ei.size(1)
    P = {'ps': _grid(g, -32, 33, (n_src, W), 2), 'pd': _grid(g, -32, 33, (dst_rows or n_dst, W), 2),
         'go': [60 * _grid(g, -2, 3, (n_dst, W)) for _ in FOUR], 'ei': ei, 'n_dst': n_dst, 'W': W,
         'De': De, 'a': None, 'Wc': None}
    if De:
        P['a'] = _grid(g, -4, 5, (E, De), 2)
        P['Wc'] = _grid(g, -2, 3, (W, De))
    n = int(torch.bincount(ei[1], minlength=n_dst).max()) if E else 1
    gran = 0.5
    assert gran ** 2 / n ** 2 >= 2e-5, f'in-degree {n}: a variance could sit near the threshold'
    # a single extremum statistic: |grad_u| <= 120, integers; grad_Wc in halves over <= n_dst
    # tied groups per column, grad_edge_attr integers over W columns
    assert n_dst * 120 * 2 * 2 < 2 ** 24 and W * 120 * 2 < 2 ** 24
    return P


def _random(n_src, n_dst, ei, W, De, seed):
    g = gen(seed)
    E = ei.size(1)
    P = {'ps': torch.randn(n_src, W, generator=g), 'pd': torch.randn(n_dst, W, generator=g),
         'go': [torch.randn(n_dst, W, generator=g) for _ in FOUR], 'ei': ei, 'n_dst': n_dst,
         'W': W, 'De': De, 'a': None, 'Wc': None}
    if De:
        P['a'] = torch.randn(E, De, generator=g)
        P['Wc'] = torch.randn(W, De, generator=g) / De ** 0.5
    return P


def _gos(P, stats):
    return [P['go'][FOUR.index(s)] for s in stats]


def _reference(P, stats, dtype=torch.float64):
    """{'out': [per statistic], the four of GRADS (None where an input is absent)} in float32"""
    ps, pd = [P[n].to(dtype).requires_grad_(True) for n in ('ps', 'pd')]
    a, Wc = [None if P[n] is None else P[n].to(dtype).requires_grad_(True) for n in ('a', 'Wc')]
    outs = R.pna_aggregate(ps, pd, a, Wc, P['ei'], P['n_dst'], stats)
    leaves = [t for t in (ps, pd, a, Wc) if t is not None]
    if P['ei'].size(1) == 0:
        grads = [torch.zeros_like(t) for t in leaves]
    else:
        grads = torch.autograd.grad(outs, leaves, [g.to(dtype) for g in _gos(P, stats)],
                                    allow_unused=True)
        grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    by = dict(zip([id(t) for t in leaves], grads))
    res = {'out': [o.detach().float() for o in outs]}
    for name, t in zip(GRADS, (ps, pd, a, Wc)):
        res[name] = None if t is None else by[id(t)].detach().float()
    return res


def _max_ties(P):
    """the largest number of slots of a (destination, column) that attain its min or its max"""
    u = P['ps'].double()[P['ei'][0]]
    if P['De']:
        u = u + P['a'].double() @ P['Wc'].double().t()
    dst, n = P['ei'][1], P['n_dst']
    worst = 0
    for how in ('min', 'max'):
        ext = R.aggregate(u, dst, n, [how])[0]
        cnt = torch.zeros(n, u.size(1)).index_add_(0, dst, (u == ext[dst]).float())
        worst = max(worst, int(cnt.max()))
    return worst


def _device_run(P, dev, stats=FOUR, index_dtype=torch.int64, edge_grad=True, strided=False):
    """the same through the autograd node, and the handle"""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import PnaAggregateFunction
    W = P['W']
    if strided:   # the left half of a [n, 2 W] tensor, read in place
        wide = torch.zeros(P['ps'].size(0), 2 * W)
        wide[:, :W] = P['ps']
        ps = wide.to(dev)[:, :W].detach().requires_grad_(True)
        assert ps.stride(0) == 2 * W
    else:
        ps = P['ps'].to(dev).requires_grad_(True)
    pd = P['pd'].to(dev).requires_grad_(True)
    a = None if P['a'] is None else P['a'].to(dev).requires_grad_(edge_grad)
    Wc = None if P['Wc'] is None else P['Wc'].to(dev).requires_grad_(True)
    graph = P.get('graph')
    if graph is None or graph.edge_index.dtype != index_dtype:
        graph = as_edge_index(P['ei'].to(dev).to(index_dtype), P['ps'].size(0), P['n_dst'])
    outs = PnaAggregateFunction.apply(ps, pd, a, Wc, graph, P['n_dst'], stats)
    assert isinstance(outs, tuple) and len(outs) == len(stats)
    leaves = [t for t in (ps, pd, a, Wc) if t is not None and t.requires_grad]
    grads = dict(zip([id(t) for t in leaves],
                     torch.autograd.grad(outs, leaves, [g.to(dev) for g in _gos(P, stats)])))
    res = {'out': [o.detach() for o in outs]}
    for name, t in zip(GRADS, (ps, pd, a, Wc)):
        res[name] = None if t is None else grads.get(id(t))
    return res, graph


def _check(got, want, stats, what, exact_grads=False):
    for s, g, w in zip(stats, got['out'], want['out']):
        assert g.shape == w.shape, f'{what}: {s} shape'
        if s in ('min', 'max'):
            assert torch.equal(g.cpu(), w), f'{what}: {s} is not exact'
        else:
            assert_close_scaled(g, w, tol=2e-5, what=f'{what} {s}')
    for name in GRADS:
        g, w = got[name], want[name]
        if w is None:
            assert g is None, f'{what}: {name} should be absent'
        elif exact_grads:
            assert g is not None and torch.equal(g.cpu(), w), \
                f'{what}: {name} is not exact (max abs err {float((g.cpu() - w).abs().max()):.3e})'
        else:
            assert g is not None
            assert_close_scaled(g, w, tol=2e-5, what=f'{what} {name}')


# ---- the kernels against float64 -------------------------------------------------------------------
_UNIFORM = {}


def _uniform_case(W, De):
    """problem and float64 results of every statistic set at one shape, computed once"""
    if (W, De) not in _UNIFORM:
        P = _dyadic(2000, 2000, T._uniform_graph(), W, De, 400 + W + 7 * De)
        assert _max_ties(P) <= 6           # 60 / ties is an integer: an even split is exact
        _UNIFORM[(W, De)] = (P, {stats: _reference(P, stats) for stats in SETS})
    return _UNIFORM[(W, De)]


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('W,De', [(1, 0), (5, 0), (24, 0), (64, 0), (100, 0), (128, 0), (512, 0),
                                  (8, 1), (24, 3), (64, 7), (100, 4), (128, 32), (256, 16),
                                  (512, 8)])
def test_kernels_match_float64(dev, W, De, index_dtype):
    """W below one lane group, odd, the float4 widths and the limit; (W, De) through every
    register capacity for De and both limits; every statistic alone and all four; min, max and
    the gradients of a run with one of them alone are exact; p_src as a column block."""
    P, want = _uniform_case(W, De)
    for stats in SETS:
        got, graph = _device_run(P, dev, stats, index_dtype)
        P['graph'] = graph
        _check(got, want[stats], stats, f'({W}, {De}) {stats}',
               exact_grads=stats in (('min', ), ('max', )))
    got, _ = _device_run(P, dev, FOUR, index_dtype, strided=True)
    _check(got, want[FOUR], FOUR, f'({W}, {De}) strided p_src')


@pytest.mark.parametrize('W,De', [(24, 0), (24, 3)])
def test_destinations_a_prefix_empty_rows_and_no_edges(dev, W, De):
    ei = random_graph(900, 300, 5000, 43)
    ei = ei[:, (ei[1] % 7 != 0) & (ei[0] % 5 != 0)]
    P = _dyadic(900, 300, ei, W, De, 11, dst_rows=900)        # p_dst longer than the destinations
    got, _ = _device_run(P, dev)
    _check(got, _reference(P, FOUR), FOUR, f'prefix ({W}, {De})')
    assert got['out'][0].shape == (300, W) and got['grad_p_dst'].shape == (900, W)
    assert float(got['grad_p_dst'][300:].abs().max()) == 0.0
    empty_dst = torch.bincount(ei[1], minlength=300) == 0
    empty_src = torch.bincount(ei[0], minlength=900) == 0
    assert int(empty_dst.sum()) >= 40 and int(empty_src.sum()) >= 180
    assert bool((P['pd'][:300][empty_dst] != 0).any())
    # every statistic of a destination without a slot is exactly 0 although p_dst is not, it takes
    # no gradient, and a source without a slot gets exact zeros
    for s, o in zip(FOUR, got['out']):
        assert float(o.cpu()[empty_dst].abs().max()) == 0.0, s
    assert float(got['grad_p_dst'].cpu()[:300][empty_dst].abs().max()) == 0.0
    assert float(got['grad_p_src'].cpu()[empty_src].abs().max()) == 0.0
    # no edges at all
    Z = _dyadic(50, 40, torch.zeros(2, 0, dtype=torch.int64), W, De, 12)
    got, _ = _device_run(Z, dev)
    _check(got, _reference(Z, FOUR), FOUR, f'no edges ({W}, {De})')
    for o in got['out']:
        assert o.shape == (40, W) and float(o.abs().max()) == 0.0
    assert got['grad_p_src'].shape == (50, W) and float(got['grad_p_src'].abs().max()) == 0.0
    if De:
        assert got['grad_edge_attr'].shape == (0, De)
        assert float(got['grad_Wc'].abs().max()) == 0.0


# ---- long rows ------------------------------------------------------------------------------------
_LONG = {}


def _long_case(De):
    """the graph of test_gpu_transformer._long_problem (a 6000-slot destination, one of threshold +
    1 slots, a 2000-slot source) at W = 64, random normal inputs"""
    if De not in _LONG:
        P = _random(3000, 3000, T._long_problem()['ei'], 64, De, 57 + De)
        P['want'] = _reference(P, FOUR)
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
    for s, g, w in zip(FOUR, got['out'], P['want']['out']):
        assert_close_scaled(g, w, tol=2e-5, what=f'long rows De = {De} {s}')
        if s in ('min', 'max'):    # an extremum is one of the u: p_dst + u is one rounding
            assert_close(g, w, rtol=1e-6, atol=1e-6, what=f'long rows De = {De} {s}')
    for name in GRADS:
        if P['want'][name] is not None:
            assert_close_scaled(got[name], P['want'][name], tol=2e-5,
                                what=f'long rows De = {De} {name}')
    info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'pna'}
    assert set(info) == {'forward', 'backward'}
    chunk = _native.HUB_CHUNK
    want = -(-6000 // chunk) + -(-(_native.HUB_THRESHOLD + 1) // chunk)
    assert info['forward']['n_hub'] == 2 and info['forward']['n_chunks'] == want
    assert info['backward']['n_hub'] == 1                       # source 7
    for rec in info.values():
        assert rec['W'] == 64 and rec['De'] == De and rec['stats'] == 15
    assert info['backward']['grad_edge_attr'] is (De > 0)


@pytest.mark.parametrize('De', [0, 6])
def test_two_runs_are_bitwise_identical(dev, De):
    """No float atomics anywhere and a grid that depends on the problem only: every output and
    gradient, grad_Wc from the per-workgroup partials and grad_edge_attr included, repeats bit for
    bit on random inputs, long rows included."""
    P = _long_case(De)
    a, graph = _device_run(P, dev)
    P['graph'] = graph
    b, _ = _device_run(P, dev)
    for s, x, y in zip(FOUR, a['out'], b['out']):
        assert torch.equal(x, y), f'De = {De}: {s} differs between two runs'
    for name in GRADS:
        assert (a[name] is None) == (b[name] is None)
        if a[name] is not None:
            assert torch.equal(a[name], b[name]), f'De = {De}: {name} differs between two runs'
    assert (a['grad_Wc'] is not None) == (De > 0) and (a['grad_edge_attr'] is not None) == (De > 0)


# ---- the variance ---------------------------------------------------------------------------------
def test_variance_is_no_worse_than_the_reference_formula(dev):
    """Messages with mean 100 and standard deviation 0.1 per column, degrees 2-64.  The kernel's
    var (its std, squared) against float64 must be within max(2e-5 * max|var|, 2 * err_ref), where
    err_ref is the error of the reference's ``mean(x^2) - mean(x)^2`` evaluated in float32 on the
    CPU for the same inputs."""
    n, W = 630, 64
    deg = 2 + torch.arange(n) % 63
    dst = torch.repeat_interleave(torch.arange(n), deg)
    g = gen(77)
    src = torch.randint(0, n, (dst.numel(), ), generator=g)
    P = {'ps': 100 + 0.1 * torch.randn(n, W, generator=g), 'pd': torch.zeros(n, W),
         'go': [torch.zeros(n, W) for _ in FOUR], 'ei': torch.stack([src, dst]), 'n_dst': n,
         'W': W, 'De': 0, 'a': None, 'Wc': None}
    assert int(deg.min()) == 2 and int(deg.max()) == 64
    u64 = P['ps'].double()[src]
    cnt = deg.double().view(-1, 1)
    mean64 = torch.zeros(n, W, dtype=torch.float64).index_add_(0, dst, u64) / cnt
    var64 = torch.zeros(n, W, dtype=torch.float64).index_add_(0, dst, (u64 - mean64[dst]) ** 2) / cnt
    u32 = P['ps'][src]
    c32 = deg.float().view(-1, 1)
    mean32 = torch.zeros(n, W).index_add_(0, dst, u32) / c32
    var32 = torch.zeros(n, W).index_add_(0, dst, u32 * u32) / c32 - mean32 * mean32
    err_ref = float((var32.double() - var64).abs().max())
    got, _ = _device_run(P, dev, ('std', ))
    var = got['out'][0].cpu().double() ** 2
    err = float((var - var64).abs().max())
    bound = max(2e-5 * float(var64.abs().max()), 2 * err_ref)
    print(f'var error: kernel {err:.3e}, reference formula in float32 {err_ref:.3e}, '
          f'bound {bound:.3e}, max var {float(var64.max()):.3e}')
    assert err <= bound


# ---- without a gradient for edge_attr -----------------------------------------------------------------
def test_without_a_gradient_for_edge_attr(dev, monkeypatch):
    """``edge_attr.requires_grad == False``: the kernel is told not to compute grad_edge_attr and
    the other gradients are bitwise those of the run that does compute it."""
    from pytorch_geometric_amd import _native
    for P in (_uniform_case(64, 7)[0], _long_case(6)):
        full, _ = _device_run(P, dev)
        sink = []
        monkeypatch.setattr(_native, 'timing_sink', sink)
        lean, _ = _device_run(P, dev, edge_grad=False)
        torch.cuda.synchronize()
        monkeypatch.undo()
        rec = [i for i, _, _ in sink if i.get('kind') == 'pna' and i['op'] == 'backward']
        assert len(rec) == 1 and rec[0]['grad_edge_attr'] is False
        assert lean['grad_edge_attr'] is None and full['grad_edge_attr'] is not None
        for name in ('grad_p_src', 'grad_p_dst', 'grad_Wc'):
            assert torch.equal(lean[name], full[name]), f'{name} differs without grad_edge_attr'


# ---- nothing of size E x W --------------------------------------------------------------------------
def test_keeps_nothing_of_edge_times_width(dev):
    """Expected above the inputs: four statistics and six saved planes (2 MiB each), the
    coefficient rows (12 MiB) with the temporaries of the pre-pass, grad_p_src, grad_p_dst,
    grad_edge_attr (8 MiB) and the per-workgroup partials of grad_Wc — below half of ONE [E, W]
    tensor."""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import PnaAggregateFunction
    N, E, W, De = 4096, 262144, 128, 8
    graph = as_edge_index(random_graph(N, N, E, 71).to(dev), N, N)
    graph.fill_cache_()
    g = gen(72)
    ps = torch.randn(N, W, generator=g).to(dev).requires_grad_(True)
    pd = torch.randn(N, W, generator=g).to(dev).requires_grad_(True)
    a = torch.randn(E, De, generator=g).to(dev).requires_grad_(True)
    Wc = torch.randn(W, De, generator=g).to(dev).requires_grad_(True)
    gos = [torch.randn(N, W, generator=g).to(dev) for _ in FOUR]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    outs = PnaAggregateFunction.apply(ps, pd, a, Wc, graph, N, FOUR)
    grads = torch.autograd.grad(outs, [ps, pd, a, Wc], gos)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'peak above the inputs: {extra / 2 ** 20:.1f} MiB')
    assert extra < E * W * 4 // 2                              # 64 MiB; one [E, W] is 128 MiB
    assert all(bool(torch.isfinite(t).all()) for t in grads)


# ---- the aggregation module ----------------------------------------------------------------------------
def test_degree_scaler_aggregation_matches_the_restatement(dev):
    from pytorch_geometric_amd.nn.aggr import DegreeScalerAggregation
    x, index, hist, aggrs, scalers = R.scaler_problem()
    mod = DegreeScalerAggregation(aggrs, scalers, hist).to(dev)
    xd = x.to(dev).requires_grad_(True)
    got = mod(xd, index.to(dev), dim_size=40)
    deg = torch.bincount(index, minlength=40).double()
    x64 = x.double().requires_grad_(True)
    want = R.scale(torch.cat(R.aggregate(x64, index, 40, aggrs), dim=-1), deg.view(-1, 1), scalers,
                   mod.avg_deg_lin.cpu().double(), mod.avg_deg_log.cpu().double())
    assert got.shape == (40, 7 * 6 * 5)
    assert_close_scaled(got, want.detach().float(), tol=2e-5, what='module out')
    assert int((deg == 0).sum()) >= 5 and float(got.detach().cpu()[deg == 0].abs().max()) == 0.0
    go = torch.randn(got.shape, generator=gen(8))
    assert_close_scaled(torch.autograd.grad(got, xd, go.to(dev))[0],
                        torch.autograd.grad(want, x64, go.double())[0].float(), tol=2e-5,
                        what='module grad')


# ---- routing --------------------------------------------------------------------------------------------
def _layer_problem(device, seed, in_channels=16, edge_dim=3, towers=2, aggregators=FOUR, **kw):
    from pytorch_geometric_amd.nn import PNAConv
    ei = random_graph(300, 300, 3000, 91)
    hist = torch.bincount(torch.bincount(ei[1], minlength=300))
    torch.manual_seed(seed)
    args = dict(aggregators=list(aggregators), scalers=['identity', 'amplification', 'attenuation'],
                edge_dim=edge_dim, towers=towers, **kw)
    conv = PNAConv(in_channels, 16, deg=hist, **args)
    g = gen(seed + 1)
    x = torch.randn(300, in_channels, generator=g)
    a = torch.randn(3000, edge_dim, generator=g) if edge_dim else None
    return conv.to(device), args, x, a, ei


def test_routing(dev, monkeypatch):
    """``pre_layers = 2``, a ``sum`` aggregator, target_to_source, a layout outside the envelope,
    ``fuse = False`` and host tensors take the generic or the host route and match float64; the
    supported layer, with and without ``edge_dim``, takes the fused one."""
    for what, kw, device in (
            ('pre_layers = 2', dict(pre_layers=2), dev),
            ('sum', dict(aggregators=('mean', 'sum', 'max')), dev),
            ('target_to_source', dict(flow='target_to_source'), dev),
            ('W * De = 8192', dict(in_channels=256, towers=1, edge_dim=32), dev),
            ('fuse = False', {}, dev),
            ('host tensors', {}, 'cpu'),
            ('supported', {}, dev),
            ('supported towers divide', dict(towers=4, divide_input=True), dev),
            ('supported without edge_dim', dict(edge_dim=None), dev)):
        conv, args, x0, a0, ei = _layer_problem(device, 9, **kw)
        if what == 'fuse = False':
            conv.fuse = False
        x = x0.to(device).requires_grad_(True)
        a = None if a0 is None else a0.to(device).requires_grad_(True)
        leaves = [x] + ([a] if a is not None else [])
        state = {}

        def step():
            state['out'] = conv(x, ei.to(device), a)
            state['grad'] = torch.autograd.grad(state['out'].sum(), leaves)

        c = T._counted(monkeypatch, step)
        fused = sorted(n for n in c.calls if n in ('pygamd_pna_forward', 'pygamd_pna_backward'))
        if what.startswith('supported'):
            assert fused == ['pygamd_pna_backward', 'pygamd_pna_forward'], (what, c.calls)
        else:
            assert not fused, (what, c.calls)
        p = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
        x64 = x0.double().requires_grad_(True)
        a64 = None if a0 is None else a0.double().requires_grad_(True)
        flipped = args.get('flow') == 'target_to_source'     # the roles of the two rows swap
        want = R.pna_layer(x64, a64, ei.flip(0) if flipped else ei, p, args)
        assert_close_scaled(state['out'], want.detach().float(), tol=2e-5, what=f'{what} out')
        refs = torch.autograd.grad(want.sum(), [x64] + ([a64] if a64 is not None else []))
        for n, g, w in zip(('grad_x', 'grad_edge_attr'), state['grad'], refs):
            assert_close_scaled(g, w.float(), tol=2e-5, what=f'{what} {n}')


def test_half_inputs_are_widened(dev):
    for edge_dim in (None, 4):
        conv, _, x, a, ei = _layer_problem(dev, 4, edge_dim=edge_dim)
        x, ei = x.to(dev), ei.to(dev)
        a = None if a is None else a.to(dev)
        want = conv(x, ei, a)
        got = conv.half()(x.half(), ei, None if a is None else a.half())
        assert got.dtype == torch.float16
        assert_close_scaled(got.float(), want, tol=2e-2, what=f'half edge_dim = {edge_dim}')


# ---- the registered operator ------------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'pna_aggregate' in ops.OPS and 'pna_aggregate_backward' in ops.OPS
    op = torch.ops.pyg_amd.pna_aggregate
    with FakeTensorMode():
        ps = torch.empty(50, 24, device='cuda', requires_grad=True)
        pd = torch.empty(12, 24, device='cuda')
        a = torch.empty(400, 5, device='cuda')
        Wc = torch.empty(24, 5, device='cuda')
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        eid = torch.empty(400, dtype=torch.int32, device='cuda')
        for args, n in (((ps, pd, a, Wc, ptr, col, eid, 15), 4),
                        ((ps, pd, None, None, ptr, col, None, 6), 2)):
            out, saved = op(*args)
            assert out.shape == (n, 12, 24) and out.requires_grad and saved.shape == (6, 12, 24)
            assert out.device.type == 'cuda' and out.dtype == torch.float32

    P, want = _uniform_case(64, 7)
    want = want[FOUR]
    order = torch.argsort(P['ei'][1], stable=True)
    col = P['ei'][0][order].to(dev)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], 2000).to(dev)
    eid = order.to(dev)                 # slot -> the caller's edge: edge_attr stays in COO order
    go = torch.stack(P['go']).to(dev)

    def fn(ps, pd, a, Wc):
        return (op(ps * 1.0, pd, a, Wc, ptr, col, eid, 15)[0] * go).sum()

    def leaves():
        return [P[n].to(dev).requires_grad_(True) for n in ('ps', 'pd', 'a', 'Wc')]

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        y = f(*ls)
        results.append([y.detach()] + list(torch.autograd.grad(y, ls)))
    for x, y in zip(*results):
        assert_close(y, x, what='compiled vs eager')
    for name, g in zip(GRADS, results[0][1:]):
        assert_close_scaled(g, want[name], tol=2e-5, what=f'operator {name}')
    out, _ = op(*[t.detach() for t in leaves()], ptr, col, eid, 15)
    for q, s in enumerate(FOUR):
        if s in ('min', 'max'):
            assert torch.equal(out[q].cpu(), want['out'][q]), s
        else:
            assert_close_scaled(out[q], want['out'][q], tol=2e-5, what=f'operator {s}')
    # edge_id = None: edge_attr follows the slots of col
    ls = [t.detach() for t in leaves()]
    ls[2] = ls[2][eid]
    assert torch.equal(op(*ls, ptr, col, None, 15)[0], out)
    torch.library.opcheck(op, (*leaves(), ptr, col, eid, 15))
