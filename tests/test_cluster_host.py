"""The geometric searches and the point-cloud layers without a GPU: the torch fallback of ``fps``,
``knn``, ``knn_graph``, ``radius``, ``radius_graph`` and ``nearest`` on host tensors against the
float64 restatement of tests/_cluster_ref.py, the doc examples of the reference's docstrings, the
output layout, the build and ABI surface, the argument statuses of the C entry points, and
``EdgeConv`` / ``DynamicEdgeConv`` / ``PointNetConv`` against tests/golden/golden_point_cloud_v1.pt."""
import ctypes

import pytest
import torch

import pytorch_geometric_amd.nn as pnn
from tests import _cluster_ref as R

SQUARE = torch.tensor([[-1.0, -1.0], [-1.0, 1.0], [1.0, -1.0], [1.0, 1.0]])
CENTRES = torch.tensor([[-1.0, 0.0], [1.0, 0.0]])
B4, B2 = torch.tensor([0, 0, 0, 0]), torch.tensor([0, 0])
SIZES_X = [1, 2, 17, 0, 64, 65, 130]
SIZES_Y = [3, 0, 17, 5, 10, 65, 1]


def cloud(sizes, F, seed, dtype=torch.float32):
    return torch.randn(sum(sizes), F, generator=torch.Generator().manual_seed(seed)).to(dtype)


def lattice(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 4, (n, 3), generator=g).float()


# ---- the doc examples: the four corners of a square -------------------------------------------------
def test_doc_examples():
    assert pnn.knn(SQUARE, CENTRES, 2, B4, B2).tolist() == [[0, 0, 1, 1], [0, 1, 2, 3]]
    assert pnn.knn_graph(SQUARE, k=2, batch=B4, loop=False).tolist() == [
        [1, 2, 0, 3, 0, 3, 1, 2], [0, 0, 1, 1, 2, 2, 3, 3]]
    assert pnn.radius(SQUARE, CENTRES, 1.5, B4, B2).tolist() == [[0, 0, 1, 1], [0, 1, 2, 3]]
    # the docstring's r = 1.5 is below the side of the square: no edge; 2.5 reaches the two sides
    assert tuple(pnn.radius_graph(SQUARE, r=1.5, batch=B4, loop=False).shape) == (2, 0)
    assert pnn.radius_graph(SQUARE, r=2.5, batch=B4, loop=False).tolist() == [
        [1, 2, 0, 3, 0, 3, 1, 2], [0, 0, 1, 1, 2, 2, 3, 3]]
    assert pnn.radius_graph(SQUARE, r=2.5, batch=B4, loop=True, max_num_neighbors=2).tolist() == [
        [0, 1, 0, 1, 0, 2, 1, 2], [0, 0, 1, 1, 2, 2, 3, 3]]
    assert pnn.fps(SQUARE, B4, ratio=0.5, random_start=False).tolist() == [0, 3]
    assert pnn.nearest(SQUARE, CENTRES, B4, B2).tolist() == [0, 0, 1, 1]
    assert pnn.PointConv is pnn.PointNetConv


def test_strict_radius_and_tie_order_on_the_lattice():
    x = lattice(200, 3)
    got = pnn.radius_graph(x, r=5 ** 0.5, loop=False, max_num_neighbors=1000)
    d2 = ((x[got[0]] - x[got[1]]) ** 2).sum(-1)
    assert float(d2.max()) < 5 and bool((got[0] != got[1]).all())   # distance^2 == 5 is out
    want = R.radius_oracle(x, x, 5 ** 0.5, [200], [200], 1000, exclude=True)
    assert torch.equal(got.flip(0), want)
    for exclude in (False, True):
        got = pnn.knn_graph(x, 10, loop=not exclude, flow='target_to_source')
        assert torch.equal(got, R.knn_oracle(x, x, 10, [200], [200], exclude=exclude))


# ---- the fallback against the restatement ----------------------------------------------------------
@pytest.mark.parametrize('F,k,cosine', [(1, 4, False), (3, 16, False), (3, 16, True),
                                        (8, 70, False), (65, 33, False)])
def test_knn_fallback(F, k, cosine):
    x, y = cloud(SIZES_X, F, 1), cloud(SIZES_Y, F, 2)
    bx, by = R.batch_of(SIZES_X), R.batch_of(SIZES_Y)
    got = pnn.knn(x, y, k, bx, by, cosine=cosine)
    assert got.dtype == torch.int64 and got.size(0) == 2
    R.check_knn(got, x, y, k, SIZES_X, SIZES_Y, cosine=cosine)
    got64 = pnn.knn(x.double(), y.double(), k, bx, by, cosine=cosine, batch_size=9)
    R.check_knn(got64, x, y, k, SIZES_X + [0, 0], SIZES_Y + [0, 0], cosine=cosine)
    if not cosine:
        assert torch.equal(got64, R.knn_oracle(x, y, k, SIZES_X, SIZES_Y))


@pytest.mark.parametrize('loop', [False, True])
def test_knn_graph_fallback_layout_and_flow(loop):
    x = cloud(SIZES_X, 3, 5)
    b = R.batch_of(SIZES_X, torch.int32)
    t2s = pnn.knn_graph(x, 6, b, loop=loop, flow='target_to_source', num_workers=4)
    s2t = pnn.knn_graph(x, 6, b, loop=loop)
    assert torch.equal(t2s.flip(0), s2t)
    assert bool((t2s[0][1:] >= t2s[0][:-1]).all())          # sorted by the query
    assert bool((t2s[0] == t2s[1]).any()) == loop
    R.check_knn(t2s, x, x, 6, SIZES_X, SIZES_X, exclude=not loop)


@pytest.mark.parametrize('F,cap', [(1, 1), (3, 32), (5, 70)])
def test_radius_fallback(F, cap):
    x, y = cloud(SIZES_X, F, 3), cloud(SIZES_Y, F, 4)
    bx, by = R.batch_of(SIZES_X), R.batch_of(SIZES_Y)
    r = 0.9 * F ** 0.5
    got = pnn.radius(x, y, r, bx, by, max_num_neighbors=cap)
    capped, empty = R.check_radius(got, x, y, r, SIZES_X, SIZES_Y, cap)
    assert empty > 0 and (capped > 0 or cap == 70)
    got64 = pnn.radius(x.double(), y.double(), r, bx, by, max_num_neighbors=cap)
    assert torch.equal(got64, R.radius_oracle(x, y, r, SIZES_X, SIZES_Y, cap))
    g = pnn.radius_graph(x, r, bx, loop=False, max_num_neighbors=cap, flow='target_to_source')
    R.check_radius(g, x, x, r, SIZES_X, SIZES_X, cap, exclude=True)
    assert torch.equal(g.flip(0), pnn.radius_graph(x, r, bx, max_num_neighbors=cap))


@pytest.mark.parametrize('ratio', [0.25, 0.5, 1.0])
def test_fps_fallback(ratio):
    sizes = [1, 2, 0, 63, 257]
    x = cloud(sizes, 3, 6)
    b = R.batch_of(sizes)
    got = pnn.fps(x, b, ratio=ratio, random_start=False)
    R.check_fps(got, x, sizes, ratio)
    assert torch.equal(pnn.fps(x.double(), b, ratio=ratio, random_start=False),
                       R.fps_oracle(x, sizes, ratio))
    torch.manual_seed(3)
    rnd = pnn.fps(x, b, ratio=ratio, random_start=True, batch_size=5)
    R.check_fps(rnd, x, sizes, ratio, random_start=True)
    # the rest of a random run is the greedy run from its first pick
    offs = torch.tensor([0] + R.fps_picks(sizes, ratio)).cumsum(0)[:-1].tolist()
    starts = [int(rnd[o]) if n > 0 else 0 for o, n in zip(offs, sizes)]
    assert torch.equal(rnd, R.fps_oracle(x, sizes, ratio, starts))
    # duplicates: the run goes on at distance 0 and never repeats an index
    lat = lattice(200, 7)
    full = pnn.fps(lat, ratio=1.0, random_start=False)
    assert torch.equal(full, R.fps_oracle(lat, [200], 1.0))
    assert full.unique().numel() == 200


def test_nearest_fallback():
    x, y = cloud(SIZES_X, 3, 8), cloud([3, 1, 17, 5, 10, 65, 1], 3, 9)
    sy = [3, 1, 17, 5, 10, 65, 1]
    got = pnn.nearest(y, x, R.batch_of(sy), R.batch_of(SIZES_X))
    want = R.knn_oracle(x, y, 1, SIZES_X, sy)
    ref = torch.full((y.size(0), ), -1, dtype=torch.int64)
    ref[want[0]] = want[1]
    assert torch.equal(got, ref)


def test_batch_rules():
    x = cloud([4, 4], 3, 10)
    bad = torch.tensor([0, 0, 1, 0, 1, 1, 1, 1])
    for call in (lambda: pnn.knn(x, x, 2, bad, bad), lambda: pnn.knn_graph(x, 2, bad),
                 lambda: pnn.radius(x, x, 1.0, bad, bad), lambda: pnn.radius_graph(x, 1.0, bad),
                 lambda: pnn.fps(x, bad), lambda: pnn.nearest(x, x, bad, bad),
                 lambda: pnn.knn_graph(x, 2, torch.tensor([0] * 4 + [1] * 4), batch_size=1)):
        with pytest.raises(ValueError):
            call()
    # half inputs are widened; k > 64 is served by the fallback
    h = pnn.knn(x.half(), x.half(), 70)
    assert h.size(1) == 8 * 8
    R.check_knn(h, x.half().float(), x.half().float(), 70, [8], [8])
    # no batch vector: one example
    assert torch.equal(pnn.knn_graph(x, 3, loop=True), pnn.knn_graph(x, 3, torch.zeros(8).long(),
                                                                      loop=True))


# ---- build and ABI surface -------------------------------------------------------------------------
def test_build_and_abi_surface():
    from pytorch_geometric_amd import _build, _lib
    assert 'cluster.hip' in _build.SOURCES
    assert _lib.ABI_VERSION == 11
    for name in ('pygamd_knn', 'pygamd_radius', 'pygamd_fps', 'pygamd_fps_workspace_size'):
        assert name in _lib.SIGNATURES


def test_argument_validation_without_gpu():
    """The entry points reject bad arguments on the host with status 1 before any device work."""
    from pytorch_geometric_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p

    def knn(k=4, F=3, ldx=3, ldy=3, x=P(16), y=P(16), px=P(16), py=P(16), out=P(16), cnt=P(16),
            idx=1, N=8, M=8, B=1):
        return lib.pygamd_knn(x, ldx, N, y, ldy, M, F, px, py, idx, B, k, 0, 0, out, cnt, None)

    assert knn(k=0) == 1 and knn(k=65) == 1
    assert knn(F=0) == 1 and knn(F=513, ldx=513, ldy=513) == 1
    assert knn(ldx=2) == 1 and knn(ldy=2) == 1
    assert knn(idx=7) == 1 and knn(N=-1) == 1 and knn(B=0) == 1
    for null in ('x', 'y', 'px', 'py', 'out', 'cnt'):
        assert knn(**{null: None}) == 1
    assert knn(M=0, y=None, out=None, cnt=None) == 0      # nothing asked: nothing launched

    def radius(r=1.0, cap=4, F=3, ldx=3, ldy=3, x=P(16), y=P(16), out=P(16), M=8):
        return lib.pygamd_radius(x, ldx, 8, y, ldy, M, F, P(16), P(16), 1, 1, r, cap, 0, out,
                                 P(16), None)

    assert radius(cap=0) == 1 and radius(r=-1.0) == 1 and radius(r=float('nan')) == 1
    assert radius(F=513, ldx=513, ldy=513) == 1 and radius(ldx=2) == 1
    assert radius(x=None) == 1 and radius(out=None) == 1
    assert radius(M=0) == 0

    def fps(F=3, ldx=3, x=P(16), ptr=P(16), out=P(16), ws=P(16), ws_bytes=32, total=4, N=8):
        return lib.pygamd_fps(x, ldx, N, F, ptr, P(16), P(16), 1, 1, total, out, ws, ws_bytes,
                              None)

    assert fps(F=0) == 1 and fps(F=513, ldx=513) == 1 and fps(ldx=2) == 1
    assert fps(x=None) == 1 and fps(ptr=None) == 1 and fps(out=None) == 1
    assert fps(ws_bytes=31) == 3 and fps(ws=None) == 3
    assert fps(total=0, out=None) == 0
    n = ctypes.c_size_t(0)
    assert lib.pygamd_fps_workspace_size(8, ctypes.byref(n)) == 0 and n.value == 32
    assert lib.pygamd_fps_workspace_size(-1, ctypes.byref(n)) == 1


# ---- the layers on host tensors --------------------------------------------------------------------
CASES = sorted(R.load_golden()['cases'])


@pytest.mark.parametrize('name', CASES)
def test_golden_layers_on_host_tensors(name):
    layer = R.check_golden_case(name, 'cpu')
    case = R.load_golden()['cases'][name]
    assert list(layer.state_dict().keys()) == case['keys']
    assert type(layer).__name__ in case['repr']


@pytest.mark.parametrize('aggr', ['max', 'add', 'mean'])
def test_dynamic_edge_conv_is_edge_conv_on_the_knn_graph(aggr):
    layer = R.check_golden_case(f'edge_conv_{aggr}', 'cpu', dynamic=True)
    assert repr(layer).endswith('k=6)')
    with pytest.raises(ValueError):
        layer(torch.zeros(2, 5, 3))


def test_dynamic_edge_conv_pair_input():
    sx, sy = [30, 0, 12], [7, 3, 12]
    xs, xt = cloud(sx, 4, 20), cloud(sy, 4, 21)
    net = R.mlp(8, 16, 5)
    # (a layer re-initialises the network it is given: build both before either runs)
    dyn, static = pnn.DynamicEdgeConv(net, 5, aggr='add'), pnn.EdgeConv(net, aggr='add')
    out = dyn((xs, xt), (R.batch_of(sx), R.batch_of(sy)))
    edges = R.knn_oracle(xs, xt, 5, sx, sy).flip(0)
    want = static((xs, xt), edges)
    assert out.shape == (22, 5) and torch.equal(out, want)
    assert float(out[7:10].abs().max()) == 0      # targets whose example has no source
