"""The "rows given" mode of the one-kernel SAGE layer (csrc/sage_fused.hip, `save_agg =
PYGAMD_AGG_GIVEN`): a launch that reads the aggregated rows back from the buffer a `save_agg = 1`
launch on the same inputs wrote, instead of gathering them.  The mode promises the SAME results bit
for bit — the tiles / term planes receive the same fp32 values and the matrix phase is the same
code — so every comparison here is `torch.equal`, in both arithmetic modes, for both index types,
on graphs with hub rows, empty rows and a partial last tile."""
import pytest
import torch

from tests._util import gen, random_graph

pytestmark = pytest.mark.gpu

N_ROWS = 1037  # 32 full tiles + one of 13 rows


@pytest.fixture(params=['split', 'fp32'])
def gemm_mode(request):
    from pytorch_geometric_amd import _native
    prev = _native.set_gemm_mode(request.param)
    yield request.param
    _native.set_gemm_mode(prev)


def _case(dev, F, Fo, dtype, seed):
    import pytorch_geometric_amd as pga
    g = gen(seed)
    ei = random_graph(N_ROWS, N_ROWS, 30000, seed=seed, skew=True)
    ei[1][ei[1] == 5] = 6  # a row without in-edges
    h = pga.EdgeIndex(ei.to(dtype).to(dev), (N_ROWS, N_ROWS))
    fwd = h.by_dst()
    assert fwd.hub[2] > 0, 'the graph is meant to have rows above the hub threshold'
    assert bool((fwd.degree() == 0).any())
    x = torch.randn(N_ROWS, F, generator=g).to(dev)
    w = (torch.randn(Fo, 2 * F, generator=g) * 0.1).to(dev)
    b = torch.randn(Fo, generator=g).to(dev)
    return fwd, x, w, b, g


def _fresh_bits(Fo, dev):
    return torch.full(((N_ROWS + 31) // 32, (Fo + 31) // 32 + 1, 32), -1, dtype=torch.int32,
                      device=dev)


@pytest.mark.parametrize('F', [4, 100, 128, 256])
@pytest.mark.parametrize('Fo', [32, 47, 256])
@pytest.mark.parametrize('reduce', ['sum', 'mean'])
@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
def test_given_rows_reproduce_the_gathering_launch(dev, gemm_mode, F, Fo, reduce, dtype):
    from pytorch_geometric_amd import _native
    if not _native.sage_layer_forward_supported(F, Fo, reduce):
        pytest.skip(f'the one-kernel layer does not take F={F}, Fo={Fo}')
    fwd, x, w, b, g = _case(dev, F, Fo, dtype, seed=F * 7 + Fo)
    poison = torch.full_like(x, float('nan'))  # the gather source of a given-mode launch: not read

    # ---- the forward's launch shape: bias, ReLU, ReLU bits, the rows stored
    agg = torch.full((N_ROWS, F), 7.0, device=dev)
    y1 = torch.full((N_ROWS, Fo + 8), 3.0, device=dev)
    bits1 = _fresh_bits(Fo, dev)
    _native.sage_layer_forward(fwd.ptr, fwd.idx, x, x, w, b, reduce, True, agg, y1[:, :Fo],
                               hub=fwd.hub, save_agg=True, relu_bits=bits1)
    assert torch.equal(agg, _native.spmm_csr(fwd.ptr, fwd.idx, x, reduce, n_rows=N_ROWS,
                                             hub=fwd.hub))
    kept = agg.clone()
    y2 = torch.full((N_ROWS, Fo + 8), 3.0, device=dev)
    bits2 = _fresh_bits(Fo, dev)
    _native.sage_layer_forward(fwd.ptr, fwd.idx, poison, x, w, b, reduce, True, agg, y2[:, :Fo],
                               hub=fwd.hub, save_agg=_native.AGG_GIVEN, relu_bits=bits2)
    assert not bool(torch.isnan(y2).any())
    assert torch.equal(y2, y1), f'given rows: y differs (max {(y2 - y1).abs().max().item():.3e})'
    assert torch.equal(bits2, bits1)
    assert torch.equal(agg, kept), 'a given-mode launch stores nothing back'

    # ---- the backward's launch shape: no bias / ReLU, mask bits, the row-scaled second output
    mask = _native.pack_relu_bits(torch.randn(N_ROWS, Fo, generator=g).to(dev))
    rs = (torch.rand(N_ROWS, generator=g) + 0.5).to(dev)
    outs = []
    for mode, src in ((True, x), (_native.AGG_GIVEN, poison)):
        y = torch.full((N_ROWS, Fo), 3.0, device=dev)
        ys = torch.full((N_ROWS, Fo), 3.0, device=dev)
        _native.sage_layer_forward(fwd.ptr, fwd.idx, src, x, w, None, reduce, False, agg, y,
                                   hub=fwd.hub, save_agg=mode, mask_bits=mask, row_scale=rs,
                                   out_scaled=ys)
        outs.append((y, ys))
    assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])
    assert torch.equal(agg, kept)


@pytest.mark.parametrize('F,Fo', [(100, 256), (256, 256), (4, 32)])
@pytest.mark.parametrize('variant', [5, 6])
def test_given_rows_through_the_ctypes_route(dev, F, Fo, variant):
    """The ctypes route into the same C entry point (here through the laboratory library's
    production variants: 5 = split kernel, 6 = fp32-instruction kernel whatever the mode) launches
    the same thing as the compiled binding; with the output once more as compressed rows (a ctypes
    only argument, fp32-instruction kernel)."""
    from pytorch_geometric_amd import _native
    fwd, x, w, b, _ = _case(dev, F, Fo, torch.int64, seed=F + Fo + variant)
    poison = torch.full_like(x, float('nan'))
    agg = torch.empty(N_ROWS, F, device=dev)
    res = []
    for mode, src in ((True, x), (_native.AGG_GIVEN, poison)):
        y = torch.full((N_ROWS, Fo), 3.0, device=dev)
        bits = _fresh_bits(Fo, dev)
        _native.sage_layer_forward(fwd.ptr, fwd.idx, src, x, w, b, 'mean', True, agg, y,
                                   hub=fwd.hub, save_agg=mode, relu_bits=bits, variant=variant)
        res.append((y, bits))
    assert torch.equal(res[1][0], res[0][0]) and torch.equal(res[1][1], res[0][1])
    # ... and the compiled binding's launch of the production entry point agrees with both
    prev = _native.set_gemm_mode('split' if variant == 5 else 'fp32')
    try:
        y = torch.full((N_ROWS, Fo), 3.0, device=dev)
        _native.sage_layer_forward(fwd.ptr, fwd.idx, poison, x, w, b, 'mean', True, agg, y,
                                   hub=fwd.hub, save_agg=_native.AGG_GIVEN)
        assert torch.equal(y, res[0][0])
        zs = []
        for mode, src in ((True, x), (_native.AGG_GIVEN, poison)):
            z = torch.zeros(N_ROWS, _native.compressed_pitch(Fo), dtype=torch.int32, device=dev)
            y = torch.full((N_ROWS, Fo), 3.0, device=dev)
            _native.sage_layer_forward(fwd.ptr, fwd.idx, src, x, w, b, 'mean', True, agg, y,
                                       hub=fwd.hub, save_agg=mode, compressed_out=z)
            zs.append((y, z))
        assert torch.equal(zs[1][0], zs[0][0]) and torch.equal(zs[1][1], zs[0][1])
    finally:
        _native.set_gemm_mode(prev)


def test_given_rows_leave_the_saved_buffer_version_alone(dev):
    """The compiled binding takes the given rows as an INPUT: the buffer sits among the saved
    tensors of every forward that used it, and a launch marked in-place would trip the version
    check of an earlier graph."""
    from pytorch_geometric_amd import _native
    fwd, x, w, b, _ = _case(dev, 100, 256, torch.int64, seed=11)
    agg = torch.empty(N_ROWS, 100, device=dev)
    y = torch.empty(N_ROWS, 256, device=dev)
    _native.sage_layer_forward(fwd.ptr, fwd.idx, x, x, w, b, 'mean', True, agg, y, hub=fwd.hub,
                               save_agg=True)
    before = agg._version
    _native.sage_layer_forward(fwd.ptr, fwd.idx, x, x, w, b, 'mean', True, agg, y, hub=fwd.hub,
                               save_agg=_native.AGG_GIVEN)
    assert agg._version == before
