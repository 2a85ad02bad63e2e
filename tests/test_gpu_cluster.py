"""The geometric searches on the device (csrc/cluster.hip) against the float64 restatement of
tests/_cluster_ref.py, and the point-cloud layers against tests/golden/golden_point_cloud_v1.pt.

Known shares of decided queries (oracle alone, computed on the CPU for the fixed seeds below): the
L2 cases with F <= 8 and the cosine case (3, 16) leave at most 0.5 % of the queries undecided; at
F >= 64 between 2 and 18 % are undecided and the rank-wise check carries the test."""
import copy
import math
import warnings

import pytest
import torch

import pytorch_geometric_amd.nn as pnn
from tests import _cluster_ref as R
from tests import _util as T

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 17, 63, 64, 65, 130, 300, 0, 257, 1000]
SIZES_Y = [3, 0, 5, 64, 1, 70, 0, 33, 12, 300, 129]      # example 8: queries without candidates
FPS_SIZES = [1, 2, 63, 64, 65, 257, 1000, 2500]
L2_CASES = [(1, 4), (2, 8), (3, 16), (3, 64), (8, 20), (64, 20), (65, 33), (128, 40), (3, 1)]
_CLOUDS = {}


def cloud(sizes, F, seed):
    key = (tuple(sizes), F, seed)
    if key not in _CLOUDS:
        _CLOUDS[key] = torch.randn(sum(sizes), F, generator=torch.Generator().manual_seed(seed))
    return _CLOUDS[key]


def lattice(n, seed):
    return torch.randint(0, 4, (n, 3), generator=torch.Generator().manual_seed(seed)).float()


# ---- knn ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('F,k', L2_CASES)
def test_knn_l2(dev, F, k, index_dtype):
    x = cloud(SIZES, F, 100 + F)
    b = R.batch_of(SIZES, index_dtype).to(dev)
    for loop in (True, False):
        got = pnn.knn_graph(x.to(dev), k, b, loop=loop, flow='target_to_source')
        assert got.dtype == torch.int64 and got.is_cuda
        share = R.check_knn(got, x, x, k, SIZES, SIZES, exclude=not loop)
        print(f'knn F={F} k={k} loop={loop}: decided {share:.4f}')
        if F <= 8:
            assert share >= 0.99


@pytest.mark.parametrize('F,k', [(3, 16), (64, 20)])
def test_knn_cosine(dev, F, k):
    x = cloud(SIZES, F, 200 + F)
    b = R.batch_of(SIZES).to(dev)
    got = pnn.knn(x.to(dev), x.to(dev), k, b, b, cosine=True)
    share = R.check_knn(got, x, x, k, SIZES, SIZES, cosine=True)
    print(f'knn cosine F={F} k={k}: decided {share:.4f}')
    if F <= 8:
        assert share >= 0.99


@pytest.mark.parametrize('F,k', [(3, 16), (64, 20)])
def test_knn_two_sets_and_batch_size(dev, F, k):
    x, y = cloud(SIZES, F, 300 + F), cloud(SIZES_Y, F, 301 + F)
    bx, by = R.batch_of(SIZES).to(dev), R.batch_of(SIZES_Y).to(dev)
    got = pnn.knn(x.to(dev), y.to(dev), k, bx, by)
    R.check_knn(got, x, y, k, SIZES, SIZES_Y)
    again = pnn.knn(x.to(dev), y.to(dev), k, bx, by, batch_size=len(SIZES) + 2)
    assert torch.equal(got, again)
    half = pnn.knn(x.half().to(dev), y.half().to(dev), k, bx, by)      # widened, same kernel
    R.check_knn(half, x.half().float(), y.half().float(), k, SIZES, SIZES_Y)
    near = pnn.nearest(y.to(dev), x.to(dev), by, bx)
    first = R.knn_oracle(x, y, 1, SIZES, SIZES_Y)
    assert int((near >= 0).sum()) == first.size(1)


def test_knn_pitched_rows(dev, monkeypatch):
    """ldx = F + 3: a column block of a wider plane that is NaN outside the block, read in place"""
    F, k = 5, 8
    x = cloud(SIZES, F, 400)
    plane = torch.full((x.size(0), F + 3), float('nan'), device=dev)
    plane[:, 2:2 + F] = x.to(dev)
    block = plane[:, 2:2 + F]
    assert block.stride(0) == F + 3 and block.data_ptr() != plane.data_ptr()
    b = R.batch_of(SIZES).to(dev)
    got = pnn.knn_graph(block, k, b, flow='target_to_source')
    R.check_knn(got, x, x, k, SIZES, SIZES, exclude=True)
    assert torch.equal(got, pnn.knn_graph(x.to(dev), k, b, flow='target_to_source'))
    rad = pnn.radius_graph(block, 1.5, b, flow='target_to_source')
    assert torch.equal(rad, pnn.radius_graph(x.to(dev), 1.5, b, flow='target_to_source'))
    assert torch.equal(pnn.fps(block, b, random_start=False),
                       pnn.fps(x.to(dev), b, random_start=False))


@pytest.mark.parametrize('loop', [True, False])
def test_knn_exact_order_and_ties_on_the_lattice(dev, loop):
    """integer coordinates in [0, 4)^3 with duplicates: every distance is exact in float32, so the
    result is the oracle's bit for bit, the (distance, index) tie order included"""
    x = lattice(200, 11)
    got = pnn.knn_graph(x.to(dev), 10, loop=loop, flow='target_to_source')
    assert torch.equal(got.cpu(), R.knn_oracle(x, x, 10, [200], [200], exclude=not loop))


@pytest.mark.parametrize('descending', [True, False])
def test_knn_insertion_paths(dev, descending):
    """300 points on a line, the query at one end: candidates in descending distance insert in
    every tile, in ascending distance nothing inserts after the first k"""
    line = torch.arange(300.0).view(-1, 1)
    x = line.flip(0).contiguous() if descending else line
    y = torch.zeros(1, 1)
    got = pnn.knn(x.to(dev), y.to(dev), 20)
    assert torch.equal(got.cpu(), R.knn_oracle(x, y, 20, [300], [1]))
    want = list(range(299, 279, -1)) if descending else list(range(20))
    assert got[1].tolist() == want


# ---- radius ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', [1, 32, 70])
@pytest.mark.parametrize('F', [1, 3, 5, 64])
def test_radius(dev, F, cap):
    x, y = cloud(SIZES, F, 500 + F), cloud(SIZES_Y, F, 501 + F)
    bx, by = R.batch_of(SIZES).to(dev), R.batch_of(SIZES_Y).to(dev)
    r = math.sqrt(1.6 * F)
    got = pnn.radius(x.to(dev), y.to(dev), r, bx, by, max_num_neighbors=cap)
    capped, empty = R.check_radius(got, x, y, r, SIZES, SIZES_Y, cap)
    print(f'radius F={F} cap={cap}: {capped} capped, {empty} empty of {y.size(0)}')
    assert capped > 0 and empty > 0
    b32 = R.batch_of(SIZES, torch.int32).to(dev)
    g = pnn.radius_graph(x.to(dev), r, b32, max_num_neighbors=cap, flow='target_to_source',
                         batch_size=len(SIZES))
    R.check_radius(g, x, x, r, SIZES, SIZES, cap, exclude=True)


@pytest.mark.parametrize('loop', [True, False])
def test_radius_strict_rule_on_the_lattice(dev, loop):
    r = 5 ** 0.5
    assert float(torch.tensor(r, dtype=torch.float32).square()) == 5.0
    x = lattice(200, 12)
    got = pnn.radius_graph(x.to(dev), r, loop=loop, max_num_neighbors=200,
                           flow='target_to_source').cpu()
    assert torch.equal(got, R.radius_oracle(x, x, r, [200], [200], 200, exclude=not loop))
    d2 = ((x[got[0]] - x[got[1]]) ** 2).sum(-1)
    assert float(d2.max()) == 4.0 or float(d2.max()) < 5.0   # a distance^2 of exactly 5 is out
    capped = pnn.radius_graph(x.to(dev), r, loop=loop, max_num_neighbors=7,
                              flow='target_to_source').cpu()
    assert torch.equal(capped, R.radius_oracle(x, x, r, [200], [200], 7, exclude=not loop))


# ---- fps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ratio', [0.25, 0.5, 0.9, 1.0])
@pytest.mark.parametrize('F', [1, 3, 8])
def test_fps(dev, F, ratio):
    x = cloud(FPS_SIZES, F, 600 + F)
    b = R.batch_of(FPS_SIZES).to(dev)
    got = pnn.fps(x.to(dev), b, ratio=ratio, random_start=False)
    assert got.dtype == torch.int64 and got.is_cuda
    picks = R.fps_picks(FPS_SIZES, ratio)
    assert picks == [math.ceil(ratio * n) for n in FPS_SIZES] and got.numel() == sum(picks)
    exact = R.check_fps(got, x, FPS_SIZES, ratio)
    print(f'fps F={F} ratio={ratio}: {exact} of {sum(p - 1 for p in picks)} steps compared exactly')
    # exact up to the same step as the oracle's own run, whose near-ties are a property of the data
    assert exact == R.check_fps(R.fps_oracle(x, FPS_SIZES, ratio), x, FPS_SIZES, ratio)
    if F == 3:   # these clouds: the oracle meets no near-tie along the whole run
        assert exact == sum(p - 1 for p in picks)


def test_fps_random_start_and_duplicates(dev):
    x = cloud(FPS_SIZES, 3, 603)
    b = R.batch_of(FPS_SIZES, torch.int32).to(dev)
    torch.manual_seed(5)
    got = pnn.fps(x.to(dev), b, ratio=0.5, random_start=True, batch_size=len(FPS_SIZES)).cpu()
    R.check_fps(got, x, FPS_SIZES, 0.5, random_start=True)
    offs = torch.tensor([0] + R.fps_picks(FPS_SIZES, 0.5)).cumsum(0)[:-1].tolist()
    starts = [int(got[o]) for o in offs]
    assert torch.equal(got, R.fps_oracle(x, FPS_SIZES, 0.5, starts))
    assert any(s != p for s, p in zip(starts, torch.tensor([0] + FPS_SIZES).cumsum(0).tolist()))
    # the lattice with duplicates: exact, lowest-index ties, on at distance 0 without a repeat
    lat = lattice(200, 13)
    full = pnn.fps(lat.to(dev), ratio=1.0, random_start=False).cpu()
    assert torch.equal(full, R.fps_oracle(lat, [200], 1.0)) and full.unique().numel() == 200
    # a cloud too large for LDS, one example, no batch vector
    big = cloud([6000], 3, 604)
    one = pnn.fps(big.to(dev), ratio=0.05, random_start=False).cpu()
    assert torch.equal(one, R.fps_oracle(big, [6000], 0.05))


# ---- routes, launches, host reads ---------------------------------------------------------------------
def test_routes_and_launches(dev, monkeypatch):
    x = cloud(SIZES, 3, 700).to(dev)
    b = R.batch_of(SIZES).to(dev)
    for fn, name in ((lambda: pnn.knn(x, x, 8, b, b), 'pygamd_knn'),
                     (lambda: pnn.knn_graph(x, 8, b), 'pygamd_knn'),
                     (lambda: pnn.radius(x, x, 1.0, b, b), 'pygamd_radius'),
                     (lambda: pnn.fps(x, b), 'pygamd_fps')):
        calls = T._call_counts(monkeypatch, fn)
        assert calls.get(name) == 1, calls
        assert sum(v for n, v in calls.items()
                   if n in ('pygamd_knn', 'pygamd_radius', 'pygamd_fps')) == 1, calls
    out = {}
    calls = T._call_counts(monkeypatch, lambda: out.update(e=pnn.knn(x, x, 65, b, b)))
    assert 'pygamd_knn' not in calls, calls
    R.check_knn(out['e'], x.cpu(), x.cpu(), 65, SIZES, SIZES)
    wide = cloud([40, 30], 513, 701).to(dev)
    bw = R.batch_of([40, 30]).to(dev)
    calls = T._call_counts(monkeypatch, lambda: out.update(w=pnn.knn(wide, wide, 4, bw, bw)))
    assert 'pygamd_knn' not in calls, calls
    R.check_knn(out['w'], wide.cpu(), wide.cpu(), 4, [40, 30], [40, 30])
    # repeatability: the same bits, run after run
    for fn in (lambda: pnn.knn_graph(x, 16, b), lambda: pnn.radius_graph(x, 1.0, b),
               lambda: pnn.fps(x, b, random_start=False),
               lambda: pnn.knn(x, x, 16, b, b, cosine=True)):
        assert torch.equal(fn(), fn())
    bad = b.flip(0)
    for fn in (lambda: pnn.knn_graph(x, 4, bad), lambda: pnn.radius_graph(x, 1.0, bad),
               lambda: pnn.fps(x, bad),
               lambda: pnn.radius_graph(x, 1.0, bad, batch_size=len(SIZES)),
               lambda: pnn.knn_graph(x, 4, bad, batch_size=len(SIZES)),
               lambda: pnn.fps(x, bad, batch_size=len(SIZES))):
        with pytest.raises(ValueError):
            fn()


def _host_reads(fn):
    """the synchronising calls torch reports while ``fn`` runs"""
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    return [w for w in seen if 'synchroniz' in str(w.message).lower()]


def test_host_reads(dev):
    x = cloud(SIZES, 3, 700).to(dev)
    b = R.batch_of(SIZES).to(dev)
    nb = len(SIZES)
    pnn.knn_graph(x, 8, b), pnn.fps(x, b), pnn.radius_graph(x, 1.0, b)      # (warm: builds, caches)
    assert len(_host_reads(lambda: x.sum().item())) == 1                    # the probe sees a read
    assert len(_host_reads(lambda: pnn.knn_graph(x, 8))) == 0
    assert len(_host_reads(lambda: pnn.knn(x, x[:100], 8))) == 0
    assert len(_host_reads(lambda: pnn.fps(x, ratio=0.5))) == 0
    assert len(_host_reads(lambda: pnn.knn_graph(x, 8, b))) == 1
    assert len(_host_reads(lambda: pnn.knn_graph(x, 8, b, batch_size=nb))) == 1
    assert len(_host_reads(lambda: pnn.fps(x, b))) == 1
    assert len(_host_reads(lambda: pnn.fps(x, b, batch_size=nb))) == 1
    assert len(_host_reads(lambda: pnn.radius_graph(x, 1.0))) == 1
    assert len(_host_reads(lambda: pnn.radius_graph(x, 1.0, b, batch_size=nb))) == 1
    # a batch vector without batch_size: one more read, for the number of examples
    assert len(_host_reads(lambda: pnn.radius_graph(x, 1.0, b))) == 2


# ---- the layers ----------------------------------------------------------------------------------------
CASES = sorted(R.load_golden()['cases'])


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', CASES)
def test_golden_layers_on_the_device(dev, name, index_dtype):
    R.check_golden_case(name, dev, index_dtype)


@pytest.mark.parametrize('aggr', ['max', 'add', 'mean'])
def test_dynamic_edge_conv_equals_the_edge_conv_golden(dev, monkeypatch, aggr):
    calls = T._call_counts(monkeypatch, lambda: R.check_golden_case(f'edge_conv_{aggr}', dev,
                                                                    dynamic=True))
    assert calls.get('pygamd_knn') == 1, calls


def test_dynamic_edge_conv_pair_input(dev):
    sx, sy = [30, 0, 12, 70], [7, 3, 12, 65]
    xs, xt = cloud(sx, 4, 800), cloud(sy, 4, 801)
    net = R.mlp(8, 16, 5)
    dyn = pnn.DynamicEdgeConv(net, 5, aggr='max')
    static = pnn.EdgeConv(copy.deepcopy(net), aggr='max')
    static.load_state_dict(dyn.state_dict())
    ref = static.double()((xs.double(), xt.double()), R.knn_oracle(xs, xt, 5, sx, sy).flip(0))
    dyn = dyn.to(dev)
    out = dyn((xs.to(dev), xt.to(dev)), (R.batch_of(sx).to(dev), R.batch_of(sy).to(dev)))
    assert out.shape == (sum(sy), 5)
    T.assert_close_scaled(out.double(), ref, what='pair input')


def test_two_stacked_dynamic_edge_convs_backpropagate(dev):
    sizes = [50, 33]
    x = cloud(sizes, 3, 900).to(dev).requires_grad_(True)
    b = R.batch_of(sizes).to(dev)
    l1 = pnn.DynamicEdgeConv(R.mlp(6, 32, 64), 8).to(dev)
    l2 = pnn.DynamicEdgeConv(R.mlp(128, 32, 16), 8, aggr='mean').to(dev)
    out = l2(l1(x, b), b)
    out.square().sum().backward()
    assert out.shape == (83, 16)
    for t in [x] + list(l1.parameters()) + list(l2.parameters()):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all())
    assert float(x.grad.abs().max()) > 0
