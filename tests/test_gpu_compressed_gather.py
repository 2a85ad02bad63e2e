"""Compressed gather sources (`x_format = PYGAMD_X_COMPRESSED`) with the chunk-per-lane decoder of
csrc/spmm_device.h: lane l of the decoding wave owns columns l, l + 64, l + 128, l + 192; headers
come in through scalar loads, value offsets from mbcnt.  Everything here is compared with
`torch.equal` on the int32 view against the dense gather: same values, same order, same bits."""
import pytest
import torch

from tests._util import decompress_rows, gen

pytestmark = pytest.mark.gpu

U = 8            # source rows in flight per wave in the decoder
N_DST = 1037
N_SRC = 611
HUB = (200, 96)  # (threshold, chunk) of the forced hub plan


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _sources(F, seed):
    """A ReLU-like block (half exact zeros) with the rows the decoder can get wrong."""
    g = gen(seed)
    x = torch.randn(N_SRC, F, generator=g).relu()
    x[0] = 0                                   # all zero
    x[1] = torch.arange(1, F + 1) * 0.25       # all kept
    x[2] = 0
    x[2, 0] = 3.0                              # only column 0
    x[3] = 0
    x[3, F - 1] = -2.0                         # only column F - 1
    x[4] = 0
    x[4, 64:128] = torch.randn(64, generator=g).abs() + 0.5   # only one whole chunk
    x[5, 1] = -0.0                             # kept: the bit pattern is not +0.0
    x[5, 70] = 1e-42                           # a denormal
    x[6, F - 2] = float('inf')
    x[7, 65] = float('-inf')
    x[7, F - 2] = float('-inf')                # (inf + -inf where rows 6 and 7 meet)
    x[8, 3] = float('nan')
    x[9, 64] = 1e-45
    x[9, 63] = -0.0
    return x


def _graph(dtype, seed):
    """CSR by destination with the degrees 0, 1, U - 1, U, U + 1, 63, 64, 65, two staged index
    chunks + 1, a hub row, and random short rows (some empty) behind them."""
    g = gen(seed)
    deg = torch.randint(0, 40, (N_DST, ), generator=g)
    head = [0, 1, U - 1, U, U + 1, 63, 64, 65, 129, 700, 5]
    deg[:len(head)] = torch.tensor(head)
    deg[N_DST - 1] = 0
    ptr = torch.zeros(N_DST + 1, dtype=torch.int64)
    ptr[1:] = deg.cumsum(0)
    col = torch.randint(0, N_SRC, (int(ptr[-1]), ), generator=g)
    # the rows of fixed degree see the special source rows, in the first and the last slots
    col[int(ptr[1])] = 8
    for r in (2, 3, 4, 5, 6, 7, 8, 9):
        s, e = int(ptr[r]), int(ptr[r + 1])
        col[s:s + 5] = torch.tensor([1, 2, 3, 4, 0])
        col[e - 1] = 5
    col[int(ptr[8]) + 64] = 9
    col[int(ptr[9]) + 300] = 6
    col[int(ptr[10]):int(ptr[10]) + 2] = torch.tensor([6, 7])   # inf + -inf
    return ptr.to(dtype), col.to(dtype), deg


def _live_third(ptr, col, deg, seed):
    """(col_live, rowend): a random third of every row's entries moved behind the row's end,
    order kept; hub rows whole (what pygamd_live_lists_build makes)."""
    g = gen(seed)
    col_live, end = col.clone(), ptr[:-1].clone()
    for r in range(N_DST):
        s, e = int(ptr[r]), int(ptr[r + 1])
        if deg[r] > HUB[0]:
            end[r] = e
            continue
        keep = torch.rand(e - s, generator=g) >= 1 / 3
        row = col[s:e]
        col_live[s:e] = torch.cat([row[keep], row[~keep]])
        end[r] = s + int(keep.sum())
    return col_live, end


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('F', [256, 192, 132])
def test_decoder_matches_the_dense_gather_bit_for_bit(dev, dtype, F):
    """`spmm_csr(compressed_width=F)` against the dense launch: last chunk full / absent / partial,
    every degree around the batch and index-chunk sizes, a hub row, special values — and the same
    over live-source lists (`rowend`) that drop a third of each row."""
    from pytorch_geometric_amd import _native
    ptr, col, deg = _graph(dtype, 7 + F)
    x = _sources(F, F)
    col_live, end = _live_third(ptr, col, deg, F + 1)
    ptr, col, col_live, end, x = (t.to(dev) for t in (ptr, col, col_live, end, x))
    hub = _native.hub_plan(ptr, *HUB)
    assert hub.n_hub == 1
    z = _native.rows_compress(x)
    for red in ('sum', 'mean'):
        dense = _native.spmm_csr(ptr, col, x, red, n_rows=N_DST, hub=hub)
        out = _native.spmm_csr(ptr, col, z, red, n_rows=N_DST, hub=hub, compressed_width=F)
        assert torch.equal(_ibits(out), _ibits(dense)), f'{red} F={F}'
    assert bool(torch.isnan(dense[1]).any()) and bool(torch.isnan(dense[10]).any())
    assert not bool(torch.isnan(dense[11:]).all())
    dense = _native.spmm_csr(ptr, col_live, x, 'sum', n_rows=N_DST, hub=hub, rowend=end)
    out = _native.spmm_csr(ptr, col_live, z, 'sum', n_rows=N_DST, hub=hub, rowend=end,
                           compressed_width=F)
    assert torch.equal(_ibits(out), _ibits(dense)), f'rowend F={F}'
    full = _native.spmm_csr(ptr, col, x, 'sum', n_rows=N_DST, hub=hub)
    assert not torch.equal(_ibits(full), _ibits(dense))   # (the lists did drop something)


@pytest.mark.parametrize('reduce', ['mean', 'sum'])
@pytest.mark.parametrize('F,Fo', [(256, 256), (192, 64), (256, 64), (192, 256)])
def test_split_layer_gathers_compressed_rows(dev, request, F, Fo, reduce):
    """The one-kernel layer on the split schedule with a compressed gather source against the same
    launch on dense rows: output, saved aggregated rows, ReLU bits.  A partial last tile (1037 =
    32 * 32 + 13), an empty row, a hub row."""
    from pytorch_geometric_amd import _native
    request.addfinalizer(lambda prev=_native.set_gemm_mode('split'): _native.set_gemm_mode(prev))
    ptr, col, _deg = _graph(torch.int64, F + Fo)
    g = gen(F * 3 + Fo)
    x = torch.randn(N_DST, F, generator=g).relu()   # (square: sources = destinations)
    x[0] = 0
    col = col % N_DST
    w = (torch.randn(Fo, 2 * F, generator=g) * 0.1).to(dev)
    b = torch.randn(Fo, generator=g).to(dev)
    ptr, col, x = ptr.to(dev), col.to(dev), x.to(dev)
    hub = _native.hub_plan(ptr, *HUB)
    assert hub.n_hub == 1
    z = _native.rows_compress(x)
    res = []
    for src, width in ((x, None), (z, F)):
        agg = torch.full((N_DST, F), float('nan'), device=dev)
        out = torch.full((N_DST, Fo), float('nan'), device=dev)
        bits = _native.relu_bits_like(N_DST, Fo, dev).fill_(-1)
        _native.sage_layer_forward(ptr, col, src, x, w, b, reduce, True, agg, out, hub=hub,
                                   save_agg=True, relu_bits=bits, gather_width=width)
        res.append((agg, out, bits))
    for a, c, what in zip(res[0], res[1], ('aggregated rows', 'output', 'ReLU bits')):
        assert torch.equal(_ibits(a), _ibits(c)), f'{what}: compressed gather differs'
    assert not bool(torch.isnan(res[1][1]).any()) and 0 < int((res[1][1] > 0).sum())
    assert bool((res[1][0][0] == 0).all())   # the empty row


@pytest.mark.parametrize('lists', [False, True])
@pytest.mark.parametrize('F,Fo', [(256, 256), (192, 64)])
def test_split_layer_input_gradient_gathers_compressed_rows(dev, request, F, Fo, lists):
    """The input-gradient form of the same launch (transposed graph, `mask_bits`, plain sum, the
    1/deg-scaled rows gathered and the unscaled ones as root operand), with the gathered rows made
    by `rows_compress(row_scale=)`, without and with live-source lists."""
    from pytorch_geometric_amd import _native
    request.addfinalizer(lambda prev=_native.set_gemm_mode('split'): _native.set_gemm_mode(prev))
    ptr, col, deg = _graph(torch.int64, 3 * F + Fo)
    col = col % N_DST
    col_live, end = _live_third(ptr, col, deg, F)
    g = gen(F + 5 * Fo)
    gr = torch.randn(N_DST, F, generator=g) * (torch.rand(N_DST, F, generator=g) < 0.5)
    scale = 1.0 / torch.randint(1, 50, (N_DST, ), generator=g).float()
    act = torch.randn(N_DST, Fo, generator=g)
    w = (torch.randn(Fo, 2 * F, generator=g) * 0.1).to(dev)
    ptr, col, col_live, end, gr, scale = (t.to(dev) for t in (ptr, col, col_live, end, gr, scale))
    mask = _native.pack_relu_bits(act.to(dev))
    hub = _native.hub_plan(ptr, *HUB)
    gs = gr * scale.view(-1, 1)
    z = _native.rows_compress(gr, row_scale=scale)
    kw = {'rowend': end} if lists else {}
    res = []
    for src, width in ((gs, None), (z, F)):
        scratch = torch.full((N_DST, F), float('nan'), device=dev)
        out = torch.full((N_DST, Fo), float('nan'), device=dev)
        _native.sage_layer_forward(ptr, col_live if lists else col, src, gr, w, None, 'sum',
                                   False, scratch, out, hub=hub, save_agg=False, mask_bits=mask,
                                   gather_width=width, **kw)
        res.append(out)
    assert torch.equal(_ibits(res[0]), _ibits(res[1]))
    assert not bool(torch.isnan(res[1]).any()) and bool((res[1] != 0).any())


@pytest.mark.parametrize('F', [256, 132, 36])
def test_rows_compress_with_a_row_scale(dev, F):
    """`rows_compress(row_scale=)` stores `x * scale[:, None]` (one fp32 multiply): the decoded
    block equals that product bit for bit, the header is `bits != +0.0`."""
    from pytorch_geometric_amd import _native
    n = 1037   # (not a multiple of the rows a wave packs)
    g = gen(F)
    x = torch.randn(n, F, generator=g) * (torch.rand(n, F, generator=g) < 0.5)
    x[3] = 0
    x[4, 0] = -0.0
    x[5, F - 1] = float('nan')
    x[6, 1] = 1e-40
    scale = 1.0 / torch.randint(1, 90, (n, ), generator=g).float()
    scale[7] = 0.0                      # x * 0: +0.0 dropped, -0.0 kept
    want = x * scale.view(-1, 1)
    wide = torch.zeros(n, F + 5)
    wide[:, 1:1 + F] = x
    z = _native.rows_compress(wide.to(dev)[:, 1:1 + F], row_scale=scale.to(dev))
    assert z.dtype == torch.int32 and z.shape == (n, _native.compressed_pitch(F))
    got, mask = decompress_rows(z, F)
    assert torch.equal(mask, _ibits(want) != 0)
    assert torch.equal(_ibits(got), _ibits(want))
    plain, _ = decompress_rows(_native.rows_compress(x.to(dev)), F)
    assert torch.equal(_ibits(plain), _ibits(x))
    with pytest.raises(ValueError):
        _native.rows_compress(torch.zeros(4, 260, device=dev), row_scale=torch.ones(4, device=dev))
    with pytest.raises(ValueError):
        _native.rows_compress(x.to(dev), row_scale=scale.to(dev)[:-1])
    with pytest.raises(ValueError):
        _native.rows_compress(x.to(dev), row_scale=scale.double().to(dev))
    with pytest.raises(Exception):
        _native.rows_compress(x.to(dev), row_scale=scale)   # a host tensor
    empty = _native.rows_compress(torch.zeros(0, F, device=dev),
                                  row_scale=torch.zeros(0, device=dev))
    assert empty.shape[0] == 0


def _train_steps(dev, aggr, steps=3):
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd.nn import GraphSAGE
    from pytorch_geometric_amd.nn.models import _fused_sage
    from tests._util import random_graph
    n = 3001
    g = gen(5)
    x = torch.randn(n, 100, generator=g).to(dev)
    y = torch.randint(0, 47, (n, ), generator=g).to(dev)
    train = torch.randperm(n, generator=g)[:n * 8 // 100].to(dev)
    ei = random_graph(n, n, 60_000, seed=3, skew=True).to(dev)
    graph = pga.EdgeIndex(ei, (n, n))
    torch.manual_seed(0)
    model = GraphSAGE(100, 256, num_layers=3, out_channels=47, aggr=aggr).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    _fused_sage.clear_aggregation_cache()
    trace = []
    for _ in range(steps):
        opt.zero_grad()
        out = model(x, graph)
        torch.nn.functional.cross_entropy(out[train], y[train]).backward()
        trace.append([out.detach().clone()] + [p.grad.clone() for p in model.parameters()])
        opt.step()
    return trace


@pytest.mark.parametrize('live', ['1', '0'])
@pytest.mark.parametrize('aggr', ['mean', 'sum'])
def test_stack_is_unchanged_by_the_compressed_gather(dev, monkeypatch, aggr, live):
    """dims (100, 256, 256, 47), loss on an 8 % split, three optimizer steps: output and every
    parameter gradient with PYGAMD_COMPRESS_GATHER on equal the run with it off, bit for bit."""
    from pytorch_geometric_amd import _native
    monkeypatch.setenv('PYGAMD_LIVE_LISTS', live)
    calls = []
    orig = _native.rows_compress
    monkeypatch.setattr(_native, 'rows_compress',
                        lambda *a, **k: (calls.append(k.get('row_scale') is not None),
                                         orig(*a, **k))[1])
    monkeypatch.setenv('PYGAMD_COMPRESS_GATHER', '0')
    off = _train_steps(dev, aggr)
    assert not calls
    monkeypatch.setenv('PYGAMD_COMPRESS_GATHER', '1')
    on = _train_steps(dev, aggr)
    assert calls, 'the switch routes nothing through the compressed gather'
    for step, (a, b) in enumerate(zip(off, on)):
        for i, (ta, tb) in enumerate(zip(a, b)):
            assert torch.equal(_ibits(ta), _ibits(tb)), f'step {step}, tensor {i}'
