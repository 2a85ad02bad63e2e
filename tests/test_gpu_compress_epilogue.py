"""Compressed rows written by the one-kernel layer's epilogue (`compressed_out`,
csrc/sage_fused_device.h `fused_compress_tile`): each row is put together in LDS and stored as whole
128-byte lines, on the split schedule (gathering and rows-given launches of a dense source) and on
the fp32 schedule.  The block is held, `torch.equal`, to what the stand-alone pass
(`_native.rows_compress`) makes of the same launch's dense output: the 8 header words and the first
popcount(header) value words of every row.  The slack behind them is unspecified, but bounded: a
row is written up to the end of the 128-byte line that holds its last kept value and no further,
the last row of the block up to the end of those 16 bytes."""
import pytest
import torch

from tests._util import gen, random_graph

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _case(n, Fi, Fo, seed):
    """Inputs whose ReLU output has the rows the writer can get wrong.  Column 0 / 1 of the root
    rows are switches (the neighbour weight of both is zero): +-1e4 on column 0 drives a whole
    output row positive / negative, 1e4 on column 1 keeps only the columns at the ends of the mask
    words (31 | 32, 63 | 64, ..., Fo - 1)."""
    g = gen(seed)
    x = torch.randn(n, Fi, generator=g)
    x[:, :2] = 0
    w = torch.randn(Fo, 2 * Fi, generator=g) * 0.1
    w[:, 0] = w[:, 1] = 0          # W_l: the switches do not travel along edges
    w[:, Fi] = 1.0                 # W_r column 0
    edge = torch.full((Fo, ), -1.0)
    for c in (0, 31, 32, 63, 64, Fo - 1):
        if c < Fo:
            edge[c] = 1.0
    w[:, Fi + 1] = edge
    rows = {}
    for name, r in (('zero', 0), ('full', 2), ('edges', 3), ('nan', 5), ('zero_last', n - 1)):
        if r < n and r not in rows.values():
            rows[name] = r
    if n == 1:
        rows = {'edges': 0}
    for name, r in rows.items():
        if name.startswith('zero'):
            x[r, 0] = -1e4
        elif name == 'full':
            x[r, 0] = 1e4
        elif name == 'edges':
            x[r, 1] = 1e4
        elif name == 'nan':
            x[r, 2] = float('nan')
    ei = random_graph(n, n, 8 * n, seed=seed + 1, skew=True)
    if n > 7:
        ei = ei[:, ei[1] != 7]                    # a node without in-edges
    if 'nan' in rows:
        ei = ei[:, ei[0] != rows['nan']]          # (the NaN stays in its own row)
    return x, w, torch.randn(Fo, generator=g), ei, rows


def _check_block(z, guard, out, what):
    """`z` ([n, pitch] view of a sentinel-filled block with one guard row behind it) against the
    stand-alone pass over `out`."""
    from pytorch_geometric_amd import _native
    n, pitch = z.shape
    ref = torch.full_like(z, SENTINEL)
    _native.rows_compress(out, out=ref)
    kept = (_ibits(out) != 0).sum(1).view(-1, 1)
    idx = torch.arange(pitch, device=z.device).view(1, -1)
    assert torch.equal(z[:, :8], ref[:, :8]), f'{what}: header words'
    vals = (idx >= 8) & (idx < 8 + kept)
    assert torch.equal(z[vals], ref[vals]), f'{what}: kept values'
    end = (8 + kept + 31) // 32 * 32               # whole lines ...
    end[n - 1] = (8 + kept[n - 1] + 3) // 4 * 4    # ... the last row: whole 16-byte pieces
    assert bool((z[idx >= end] == SENTINEL).all()), f'{what}: a row is written past its last line'
    assert bool((guard == SENTINEL).all()), f'{what}: written past the block'


@pytest.mark.parametrize('n', [1, 33, 75, 257])
@pytest.mark.parametrize('Fi,Fo', [(100, 256), (16, 160), (256, 256)])
def test_epilogue_block_equals_the_stand_alone_pass(dev, request, n, Fi, Fo):
    """mean / sum, int32 / int64 indices, with / without bias, both schedules; the gathering launch
    and then the rows-given launch on the rows it saved."""
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd import _native
    request.addfinalizer(lambda prev=_native.get_gemm_mode(): _native.set_gemm_mode(prev))
    x, w, b, ei, rows = _case(n, Fi, Fo, 7 * n + Fi + Fo)
    x, w, b = x.to(dev), w.to(dev), b.to(dev)
    pitch = _native.compressed_pitch(Fo)
    seen = set()
    for mode in ('split', 'fp32'):
        _native.set_gemm_mode(mode)
        for dtype in (torch.int64, torch.int32):
            fwd = pga.EdgeIndex(ei.to(dtype).to(dev), (n, n)).by_dst()
            for reduce in ('mean', 'sum'):
                for bias in (b, None):
                    agg = torch.full((n, Fi), float('nan'), device=dev)
                    dense = None
                    for given in (False, True):
                        what = f'{mode} {dtype} {reduce} bias={bias is not None} given={given}'
                        out = torch.full((n, Fo), float('nan'), device=dev)
                        bits = _native.relu_bits_like(n, Fo, dev).fill_(-1)
                        block = torch.full((n + 1, pitch), SENTINEL, dtype=torch.int32,
                                           device=dev)
                        _native.sage_layer_forward(
                            fwd.ptr, fwd.idx, x, x, w, bias, reduce, True, agg, out, hub=fwd.hub,
                            save_agg=_native.AGG_GIVEN if given else True, relu_bits=bits,
                            compressed_out=block[:n])
                        _check_block(block[:n], block[n], out, what)
                        if given:  # the same launch without the writer: nothing else moved
                            assert torch.equal(_ibits(out), _ibits(dense[0])), what
                            assert torch.equal(bits, dense[1]), what
                        else:
                            plain = torch.full((n, Fo), float('nan'), device=dev)
                            pbits = _native.relu_bits_like(n, Fo, dev).fill_(-1)
                            pagg = torch.full((n, Fi), float('nan'), device=dev)
                            _native.sage_layer_forward(
                                fwd.ptr, fwd.idx, x, x, w, bias, reduce, True, pagg, plain,
                                hub=fwd.hub, save_agg=True, relu_bits=pbits)
                            assert torch.equal(_ibits(out), _ibits(plain)), what
                            assert torch.equal(bits, pbits), what
                            assert torch.equal(_ibits(agg), _ibits(pagg)), what
                            dense = (out, bits)
                    # the rows this case is about are there
                    o = out.cpu()
                    for name, r in rows.items():
                        if name.startswith('zero'):
                            assert bool((_ibits(o[r]) == 0).all())
                        elif name == 'full':
                            assert bool((o[r] > 0).all())
                        elif name == 'edges':
                            on = [c for c in (0, 31, 32, 63, 64, Fo - 1) if c < Fo]
                            assert bool((o[r, on] > 0).all()) and int((o[r] != 0).sum()) == len(on)
                        elif name == 'nan':
                            assert bool(o[r].isnan().all())
                        seen.add(name)
    assert seen >= set(rows)


def _train_steps(dev, n, steps=3):
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd.nn import GraphSAGE
    from pytorch_geometric_amd.nn.models import _fused_sage
    g = gen(n)
    x = torch.randn(n, 100, generator=g).to(dev)
    y = torch.randint(0, 47, (n, ), generator=g).to(dev)
    train = torch.randperm(n, generator=g)[:max(n // 5, 4)].to(dev)
    ei = random_graph(n, n, 10 * n, seed=n + 3, skew=True)
    ei = ei[:, ei[1] != 8].to(dev)   # a node without in-edges
    graph = pga.EdgeIndex(ei, (n, n))
    torch.manual_seed(0)
    model = GraphSAGE(100, 256, num_layers=3, out_channels=47).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    _fused_sage.clear_aggregation_cache()
    trace = []
    for _ in range(steps):   # (step 1 gathers and stores the first layer's rows, 2 and 3 read them)
        opt.zero_grad()
        out = model(x, graph)
        torch.nn.functional.cross_entropy(out[train], y[train]).backward()
        trace.append([out.detach().clone()] + [p.grad.clone() for p in model.parameters()])
        opt.step()
    return trace


@pytest.mark.parametrize('n', [75, 257])
def test_stack_is_unchanged_by_the_epilogue_writer(dev, request, monkeypatch, n):
    """dims (100, 256, 256, 47), three optimizer steps: output and every parameter gradient of the
    default route (layer 1 writes layer 2's compressed gather source, no forward pass runs) equal
    those with COMPRESS_ROWS off (the stand-alone pass) and with PYGAMD_COMPRESS_GATHER=0 (dense
    gathers), bit for bit."""
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn.models import _fused_sage
    request.addfinalizer(lambda prev=_native.set_gemm_mode('split'): _native.set_gemm_mode(prev))
    passes, writers = [], []
    compress, layer = _native.rows_compress, _native.sage_layer_forward
    monkeypatch.setattr(_native, 'rows_compress',
                        lambda *a, **k: (passes.append(k.get('row_scale') is not None),
                                         compress(*a, **k))[1])
    monkeypatch.setattr(_native, 'sage_layer_forward',
                        lambda *a, **k: (writers.append(k.get('compressed_out') is not None),
                                         layer(*a, **k))[1])
    monkeypatch.setenv('PYGAMD_COMPRESS_GATHER', '1')
    monkeypatch.setattr(_fused_sage, 'COMPRESS_ROWS', None)
    unset = _train_steps(dev, n)
    assert passes.count(False) == 0, 'the default route still runs the forward compress pass'
    assert writers.count(True) == 3, 'layer 1 writes the compressed block once per step'
    del passes[:], writers[:]
    monkeypatch.setattr(_fused_sage, 'COMPRESS_ROWS', False)
    off = _train_steps(dev, n)
    assert passes.count(False) == 3 and writers.count(True) == 0
    monkeypatch.setattr(_fused_sage, 'COMPRESS_ROWS', None)
    monkeypatch.setenv('PYGAMD_COMPRESS_GATHER', '0')
    dense = _train_steps(dev, n)
    for other, name in ((off, 'COMPRESS_ROWS=0'), (dense, 'PYGAMD_COMPRESS_GATHER=0')):
        for step, (a, b) in enumerate(zip(unset, other)):
            for i, (ta, tb) in enumerate(zip(a, b)):
                assert torch.equal(_ibits(ta), _ibits(tb)), f'{name}: step {step}, tensor {i}'
