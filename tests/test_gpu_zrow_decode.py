"""What a decoder of compressed rows without per-load branches can newly get wrong (csrc/
spmm_device.h, `zrows_batch`: the chunk masks are written into exec by hand and the waits for the
loads are the decoder's own): junk in the words behind the kept values and behind the block,
chunk masks at their edges, kept counts that end on a 128-byte line, special values next to cleared
bits.  Everything is compared on the int32 view with the same launch on dense rows; the shapes are
those of tests/test_gpu_compressed_gather.py."""
import pytest
import torch

from tests._util import gen

pytestmark = pytest.mark.gpu

U = 8            # source rows in flight per wave in the decoder
N = 1037         # destination rows (and the source rows of the square layer launches)
N_SRC = 611      # source rows of the stand-alone aggregation
HUB = (200, 96)  # (threshold, chunk) of the forced hub plan
NAN_WORDS = 4096  # words of NaN bits behind the block
FILLS = [0xFFFFFFFF, 0x7FC00000]
LAST = ['all kept', 'all zero', 'only column F - 1']
EDGE0 = 20       # first of the rows with a chunk mask at its edges
DEG189 = (40, 41, 42)  # destination rows of degree 1, 8, 9 that gather the last source row


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _i32(word):
    return word - (1 << 32) if word >= (1 << 31) else word


def _chunk_patterns(width):
    """The six masks of one chunk of `width` <= 64 columns (lane 63, the upper half: where the
    chunk has them)."""
    lane = torch.arange(width)
    return [lane == 0, lane == 63, lane < 32, lane >= 32, lane >= 0, lane < 0]


def _sources(n, F, last, seed):
    """Half exact zeros, then: every chunk in turn with its mask at an edge (rows EDGE0 ...), kept
    counts that end on a line boundary, special values between cleared bits, the last row."""
    g = gen(seed)
    x = torch.randn(n, F, generator=g).relu()
    r = EDGE0
    for k in range((F + 63) // 64):
        lo, hi = 64 * k, min(64 * k + 64, F)
        for keep in _chunk_patterns(hi - lo):
            x[r, lo:hi] = torch.where(keep, torch.rand(hi - lo, generator=g) + 0.5,
                                      torch.zeros(hi - lo))
            r += 1
    assert r <= EDGE0 + 24
    # 8 + kept = 32 behind chunk 0 (and = 64 in the next row); = 96 behind chunk 2 (24 + 32 + 32)
    x[1] = 0
    x[1, torch.randperm(64, generator=g)[:24]] = 1.5
    x[1, 64:F] = torch.randn(F - 64, generator=g).relu()
    x[2] = 0
    x[2, torch.randperm(64, generator=g)[:56]] = -2.5
    x[2, 64:F] = torch.randn(F - 64, generator=g).relu()
    x[3] = 0
    for k, cnt in enumerate((24, 32, 32)):
        lo, hi = 64 * k, min(64 * k + 64, F)
        if hi - lo >= cnt:
            x[3, lo + torch.randperm(hi - lo, generator=g)[:cnt]] = 0.75
    x[3, 192:] = 1.0
    # kept special values, the columns around them cleared
    x[4] = 0
    x[4, 5] = -0.0
    x[4, 63] = -0.0
    x[4, 70] = 1e-42
    x[4, 130] = float('inf')
    x[5] = 0
    x[5, 64] = 1e-45
    x[5, 127] = -1e-40
    x[5, F - 1] = float('-inf')
    x[6, 9:12] = torch.tensor([0.0, -0.0, 0.0])
    x[n - 1] = 0
    if last == 'all kept':
        x[n - 1] = torch.arange(1, F + 1) * 0.25
    elif last == 'only column F - 1':
        x[n - 1, F - 1] = 3.0
    return x


def _graph(n_src, seed):
    """CSR by destination: the degrees around the batch and index-chunk sizes, a hub row, the
    special source rows in short rows of their own, and rows of degree 1, 8, 9 whose first and
    last slot gather the last source row."""
    g = gen(seed)
    deg = torch.randint(0, 40, (N, ), generator=g)
    head = [0, 1, U - 1, U, U + 1, 63, 64, 65, 129, 700, 5]
    deg[:len(head)] = torch.tensor(head)
    deg[EDGE0:EDGE0 + 12] = 3
    deg[list(DEG189)] = torch.tensor([1, U, U + 1])
    deg[N - 1] = 0
    ptr = torch.zeros(N + 1, dtype=torch.int64)
    ptr[1:] = deg.cumsum(0)
    col = torch.randint(0, n_src, (int(ptr[-1]), ), generator=g)
    for r in (2, 3, 4, 5, 6, 7, 8):   # the line-boundary and special-value rows, first slots
        col[int(ptr[r]):int(ptr[r]) + 6] = torch.arange(1, 7)
    edge = torch.arange(EDGE0, EDGE0 + 24)  # 4 chunks x 6 masks, two to a row (+ a random one)
    for i in range(12):
        s = int(ptr[EDGE0 + i])
        col[s], col[s + 2] = edge[2 * i], edge[2 * i + 1]
    for r in DEG189:
        col[int(ptr[r])] = n_src - 1
        col[int(ptr[r + 1]) - 1] = n_src - 1
    return ptr, col, deg


def _live_third(ptr, col, deg, seed):
    """(col_live, rowend): a random third of every row's entries moved behind the row's end,
    order kept; hub rows whole."""
    g = gen(seed)
    col_live, end = col.clone(), ptr[:-1].clone()
    for r in range(N):
        s, e = int(ptr[r]), int(ptr[r + 1])
        if deg[r] > HUB[0]:
            end[r] = e
            continue
        keep = torch.rand(e - s, generator=g) >= 1 / 3
        row = col[s:e]
        col_live[s:e] = torch.cat([row[keep], row[~keep]])
        end[r] = s + int(keep.sum())
    return col_live, end


def _compress_into_junk(x, F, pitch, fill):
    """`rows_compress` into a block of n x pitch words that was filled with `fill` and that lies in
    front of NAN_WORDS words of NaN bits: a word read behind a row's kept values, or behind the
    block, is a NaN in a sum and never a fault."""
    from pytorch_geometric_amd import _native
    n = x.size(0)
    buf = torch.full((n * pitch + NAN_WORDS, ), _i32(fill), dtype=torch.int32, device=x.device)
    z = buf[:n * pitch].view(n, pitch)
    _native.rows_compress(x, out=z)
    assert bool((buf[n * pitch:] == _i32(fill)).all())
    return z


def _pitch(F, kind):
    from pytorch_geometric_amd import _native
    return F + 12 if kind == 'min' else _native.compressed_pitch(F)


@pytest.mark.parametrize('fill', FILLS, ids=['ones', 'qnan'])
@pytest.mark.parametrize('pitch', ['min', 'line'])
@pytest.mark.parametrize('F', [256, 192, 132])
def test_aggregation_reads_no_word_it_does_not_own(dev, F, pitch, fill):
    """`spmm_csr(compressed_width=F)`, sum / mean / over `rowend` lists, for each kind of last source
    row: equal to the dense launch, and no NaN anywhere (no source holds one)."""
    from pytorch_geometric_amd import _native
    ptr, col, deg = _graph(N_SRC, 11 + F)
    col_live, end = _live_third(ptr, col, deg, F + 2)
    ptr, col, col_live, end = (t.to(dev) for t in (ptr, col, col_live, end))
    hub = _native.hub_plan(ptr, *HUB)
    assert hub.n_hub == 1
    for last in LAST:
        x = _sources(N_SRC, F, last, F).to(dev)
        z = _compress_into_junk(x, F, _pitch(F, pitch), fill)
        for red in ('sum', 'mean'):
            dense = _native.spmm_csr(ptr, col, x, red, n_rows=N, hub=hub)
            out = _native.spmm_csr(ptr, col, z, red, n_rows=N, hub=hub, compressed_width=F)
            assert not bool(torch.isnan(out).any()), f'{red}, last row {last}: NaN'
            assert torch.equal(_ibits(out), _ibits(dense)), f'{red}, last row {last}'
        dense = _native.spmm_csr(ptr, col_live, x, 'sum', n_rows=N, hub=hub, rowend=end)
        out = _native.spmm_csr(ptr, col_live, z, 'sum', n_rows=N, hub=hub, rowend=end,
                               compressed_width=F)
        assert not bool(torch.isnan(out).any()), f'rowend, last row {last}: NaN'
        assert torch.equal(_ibits(out), _ibits(dense)), f'rowend, last row {last}'
        assert bool(torch.isinf(dense).any())   # (the special values are gathered)


def _layer_launches(dev, F, Fo, pitch, fill, last):
    """The layer-forward form (mean, saved aggregated rows, ReLU bits) and the input-gradient form
    (sum, `mask_bits`, `rowend` lists) of the one-kernel layer, each on dense rows and on the same
    rows compressed into junk."""
    from pytorch_geometric_amd import _native
    ptr, col, deg = _graph(N, 3 * F + Fo)
    col_live, end = _live_third(ptr, col, deg, F)
    g = gen(F + 7 * Fo)
    x = _sources(N, F, last, F + 1).to(dev)
    w = (torch.randn(Fo, 2 * F, generator=g) * 0.1).to(dev)
    b = torch.randn(Fo, generator=g).to(dev)
    mask = _native.pack_relu_bits(torch.randn(N, Fo, generator=g).to(dev))
    ptr, col, col_live, end = (t.to(dev) for t in (ptr, col, col_live, end))
    hub = _native.hub_plan(ptr, *HUB)
    assert hub.n_hub == 1
    z = _compress_into_junk(x, F, _pitch(F, pitch), fill)
    fwd, bwd = [], []
    for src, width in ((x, None), (z, F)):
        agg = torch.full((N, F), float('nan'), device=dev)
        out = torch.full((N, Fo), float('nan'), device=dev)
        bits = _native.relu_bits_like(N, Fo, dev).fill_(-1)
        _native.sage_layer_forward(ptr, col, src, x, w, b, 'mean', True, agg, out, hub=hub,
                                   save_agg=True, relu_bits=bits, gather_width=width)
        fwd.append((agg, out, bits))
        scratch = torch.full((N, F), float('nan'), device=dev)
        gout = torch.full((N, Fo), float('nan'), device=dev)
        _native.sage_layer_forward(ptr, col_live, src, x, w, None, 'sum', False, scratch, gout,
                                   hub=hub, save_agg=False, mask_bits=mask, gather_width=width,
                                   rowend=end)
        bwd.append(gout)
    return fwd, bwd


def _check_layer(fwd, bwd, what):
    for a, c, name in zip(fwd[0], fwd[1], ('aggregated rows', 'output', 'ReLU bits')):
        assert torch.equal(_ibits(a), _ibits(c)), f'{what}: forward {name} differ'
    assert not bool(torch.isnan(fwd[1][0]).any()), f'{what}: NaN in the aggregated rows'
    assert torch.equal(_ibits(bwd[0]), _ibits(bwd[1])), f'{what}: input gradient differs'
    assert bool((fwd[1][0][0] == 0).all())   # the empty row


@pytest.mark.parametrize('fill', FILLS, ids=['ones', 'qnan'])
@pytest.mark.parametrize('pitch', ['min', 'line'])
@pytest.mark.parametrize('F,Fo', [(256, 256), (192, 64)])
def test_split_layer_reads_no_word_it_does_not_own(dev, request, F, Fo, pitch, fill):
    """Both forms of the split launch, for each kind of last source row."""
    from pytorch_geometric_amd import _native
    request.addfinalizer(lambda prev=_native.set_gemm_mode('split'): _native.set_gemm_mode(prev))
    for last in LAST:
        fwd, bwd = _layer_launches(dev, F, Fo, pitch, fill, last)
        _check_layer(fwd, bwd, f'last row {last}')


def test_fp32_schedule_reads_no_word_it_does_not_own(dev, request):
    """The same source block through the fp32 schedule with a compressed source."""
    from pytorch_geometric_amd import _native
    request.addfinalizer(lambda prev=_native.set_gemm_mode('fp32'): _native.set_gemm_mode(prev))
    fwd, bwd = _layer_launches(dev, 256, 64, 'min', FILLS[0], LAST[0])
    _check_layer(fwd, bwd, 'fp32 schedule')
