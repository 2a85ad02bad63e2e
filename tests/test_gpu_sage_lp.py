"""The one-kernel SAGE layer on float16 / bfloat16 storage (csrc/sage_fused_lp.hip,
``pygamd_sage_layer_lp``) against float64.

Small graph: 70 nodes (two full tiles of 32 rows and one of 6) with an empty row, a row of degree
1, one of degree 65 (more than one staged batch of 64 slots) and self-loops.  Hub graph: 1,100
nodes, one destination of in-degree 1,030 (above the hub threshold of 1,024: five chunks); and
2,400 nodes with one of in-degree 2,300 (nine chunks: one batch of eight partial loads and a tail).

``agg`` must equal ``utils.spmm(h, x, reduce)`` bit for bit (the same accumulation code in the same
order).  ``out`` is bounded elementwise against ``ref = agg W_l^T + x W_r^T + b`` in float64 on the
widened 16-bit values, ``agg`` being that verified 16-bit aggregation, by
``u |ref| + (2 F + 3) 2^-24 (|agg| |W_l|^T + |x| |W_r|^T + |b|)``: the one final rounding (u = 2^-8
bfloat16, 2^-11 float16) plus the float32 accumulation of 2 F exactly representable products and
the bias.  Inputs are small integers over a power of two, so every float16 operand is normal."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
IDX = {'i32': torch.int32, 'i64': torch.int64}
# F: 8 columns per lane, LPR = 1, 2, 4, 8, 16, 32, 32, 64; 8, 24, 72, 136: K tails (F % 16 != 0);
# Fo: 1 and 40 masked columns, 264 a second column pass
CASES = [(8, 1, 'mean', 'i32'), (16, 40, 'sum', 'i64'), (24, 40, 'mean', 'i64'),
         (64, 33, 'sum', 'i32'), (72, 264, 'sum', 'i32'), (136, 40, 'mean', 'i64'),
         (256, 264, 'mean', 'i32'), (512, 8, 'sum', 'i64')]


@functools.lru_cache(None)
def _edges(kind):
    src, dst = [], []
    if kind == 'small':
        n = 70
        for r in range(n):
            deg = {0: 0, 1: 1, 2: 65}.get(r, r % 5 + 1)
            for k in range(deg):
                src.append(r if k == 0 and r > 2 else (7 * k + 3 * r) % n)  # k == 0: a self-loop
                dst.append(r)
    else:
        n, hub_deg = (1100, 1030) if kind == 'hub' else (2400, 2300)
        for r in range(n):
            deg = hub_deg if r == 5 else r % 3
            for k in range(deg):
                src.append((k + r) % n)
                dst.append(r)
    return n, torch.tensor([src, dst])


def _handle(dev, kind, idx):
    import pytorch_geometric_amd as pga
    n, ei = _edges(kind)
    h = pga.EdgeIndex(ei.to(dev).to(IDX[idx]), (n, n)).fill_cache_()
    assert h.by_dst().hub.n_hub == (0 if kind == 'small' else 1)
    return h


@functools.lru_cache(None)
def _inputs(n, F, Fo, dtype):
    g = torch.Generator().manual_seed(1000 * F + Fo)
    x = (torch.randint(-64, 65, (n, F), generator=g) / 32).to(dtype)
    wl = (torch.randint(-32, 33, (Fo, F), generator=g) / 64).to(dtype)
    wr = (torch.randint(-32, 33, (Fo, F), generator=g) / 64).to(dtype)
    b = (torch.randint(-16, 17, (Fo, ), generator=g) / 8).to(dtype)
    return x, wl, wr, b


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check(h, x, wl, wr, b, reduce, out, agg):
    """the two assertions of the module docstring; x, wl, wr, b: the 16-bit device operands"""
    import pytorch_geometric_amd as pga
    dtype, F = x.dtype, x.size(1)
    want_agg = pga.utils.spmm(h, x.contiguous(), reduce)
    if agg is not None:
        assert agg.dtype == dtype and torch.equal(_bits(agg), _bits(want_agg))
    a, x64, wl, wr, b = (t.detach().cpu().double() for t in (want_agg, x, wl, wr, b))
    ref = a @ wl.t() + x64 @ wr.t() + b
    mag = a.abs() @ wl.abs().t() + x64.abs() @ wr.abs().t() + b.abs()
    bound = U[dtype] * ref.abs() + (2 * F + 3) * 2.0 ** -24 * mag
    err = (out.detach().cpu().double() - ref).abs()
    print(f'F={F} Fo={wl.size(0)} worst err / bound = '
          f'{float((err / bound.clamp(min=1e-300)).max()):.3f}')
    assert out.dtype == dtype and bool((err <= bound).all())


@pytest.mark.parametrize('F,Fo,reduce,idx', CASES)
@pytest.mark.parametrize('dtype', DTYPES, ids=['f16', 'bf16'])
def test_small_graph(dev, dtype, F, Fo, reduce, idx):
    from pytorch_geometric_amd import _native
    h = _handle(dev, 'small', idx)
    x, wl, wr, b = (t.to(dev) for t in _inputs(70, F, Fo, dtype))
    fwd = h.by_dst()
    out, agg = _native.sage_layer_lp(fwd.ptr, fwd.idx, x, wl, wr, b, reduce, hub=fwd.hub,
                                     save_agg=True)
    _check(h, x, wl, wr, b, reduce, out, agg)
    assert not bool(agg[0].any()) and bool(out[0].eq(out[0]).all())  # the empty row


@pytest.mark.parametrize('kind,dtype,F,Fo,reduce,idx',
                         [('hub', torch.float16, 72, 40, 'mean', 'i32'),
                          ('hub', torch.bfloat16, 256, 264, 'sum', 'i64'),
                          ('hub9', torch.float16, 136, 33, 'mean', 'i64')],
                         ids=['f16', 'bf16', 'f16-9-chunks'])
def test_hub_row(dev, kind, dtype, F, Fo, reduce, idx):
    from pytorch_geometric_amd import _native
    h = _handle(dev, kind, idx)
    x, wl, wr, b = (t.to(dev) for t in _inputs(_edges(kind)[0], F, Fo, dtype))
    fwd = h.by_dst()
    out, agg = _native.sage_layer_lp(fwd.ptr, fwd.idx, x, wl, wr, b, reduce, hub=fwd.hub,
                                     save_agg=True)
    _check(h, x, wl, wr, b, reduce, out, agg)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f16', 'bf16'])
def test_row_pitches(dev, dtype):
    from pytorch_geometric_amd import _native
    F, Fo = 24, 40
    h = _handle(dev, 'small', 'i64')
    x, wl, wr, b = (t.to(dev) for t in _inputs(70, F, Fo, dtype))
    wide = torch.full((70, F + 16), float('nan'), dtype=dtype, device=dev)
    wide[:, 8:8 + F] = x
    plane = torch.full((70, Fo + 7), 3.0, dtype=dtype, device=dev)
    fwd = h.by_dst()
    out, agg = _native.sage_layer_lp(fwd.ptr, fwd.idx, wide[:, 8:8 + F], wl, wr, None, 'mean',
                                     hub=fwd.hub, out=plane[:, 3:3 + Fo], save_agg=True)
    assert out.data_ptr() == plane[:, 3:3 + Fo].data_ptr()
    _check(h, x, wl, wr, torch.zeros_like(b), 'mean', plane[:, 3:3 + Fo], agg)
    assert bool((plane[:, :3] == 3).all()) and bool((plane[:, 3 + Fo:] == 3).all())


def _count(monkeypatch):
    from pytorch_geometric_amd import _native
    calls, real = [], _native.sage_layer_lp

    def counted(rowptr, col, x, *args, **kwargs):
        calls.append((x.dtype, kwargs['save_agg']))
        return real(rowptr, col, x, *args, **kwargs)

    monkeypatch.setattr(_native, 'sage_layer_lp', counted)
    return calls


def _conv(dev, dtype, F=24, Fo=40, fuse_lp=True, **kwargs):
    import pytorch_geometric_amd as pga
    torch.manual_seed(3)
    conv = pga.nn.SAGEConv(F, Fo, **kwargs).to(dev).to(dtype)
    conv.fuse_lp = fuse_lp
    return conv


def _outcome(conv, *args):
    try:
        return conv(*args)
    except RuntimeError as e:   # (float32 weights on 16-bit rows: torch's linear refuses both ways)
        return type(e)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f16', 'bf16'])
def test_public_route(dev, monkeypatch, dtype):
    import pytorch_geometric_amd as pga
    calls = _count(monkeypatch)
    h = _handle(dev, 'small', 'i64')
    x = _inputs(70, 24, 40, dtype)[0].to(dev)
    conv = _conv(dev, dtype)
    out = conv(x, h)
    assert calls == [(dtype, True)]
    _check(h, x, conv.lin_l.weight, conv.lin_r.weight, conv.lin_l.bias, 'mean', out, None)
    with torch.no_grad():   # inference: the aggregation is neither allocated nor written
        quiet = conv(x, h)
    assert calls[1:] == [(dtype, False)] and torch.equal(_bits(quiet), _bits(out))
    del calls[:]
    x12 = _inputs(70, 16, 40, dtype)[0][:, :12].contiguous().to(dev)
    pair = pga.EdgeIndex(_edges('small')[1][:, :40].to(dev), (70, 70))
    refused = [(_conv(dev, dtype, fuse_lp=False), (x, h)),
               (_conv(dev, dtype, F=12), (x12, h)),
               (_conv(dev, torch.float32), (x, h)),
               (_conv(dev, dtype, aggr='max'), (x, h)),
               (_conv(dev, dtype), ((x, x[:70]), pair))]
    for conv, args in refused:
        got = _outcome(conv, *args)
        conv.fuse_lp = False
        want = _outcome(conv, *args)
        assert calls == []
        if isinstance(want, torch.Tensor):
            assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))
        else:
            assert got is want


@pytest.mark.parametrize('reduce', ['mean', 'sum'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['f16', 'bf16'])
def test_gradients(dev, dtype, reduce):
    h = _handle(dev, 'small', 'i64')
    n, ei = _edges('small')
    A = torch.zeros(n, n, dtype=torch.float64).index_put_(
        (ei[1], ei[0]), torch.ones(ei.size(1), dtype=torch.float64), accumulate=True)
    if reduce == 'mean':
        A = A / A.sum(1, keepdim=True).clamp(min=1)
    x16 = _inputs(n, 24, 40, dtype)[0]
    grads = {}
    for fuse_lp in (True, False):
        conv = _conv(dev, dtype, fuse_lp=fuse_lp, aggr=reduce)
        x = x16.to(dev).requires_grad_(True)
        params = [x, conv.lin_l.weight, conv.lin_r.weight, conv.lin_l.bias]
        grads[fuse_lp] = torch.autograd.grad(conv(x, h).float().square().sum(), params)
    ref_in = [p.detach().cpu().double().requires_grad_(True) for p in params]
    x64, wl, wr, b = ref_in
    ref = torch.autograd.grad(((A @ x64) @ wl.t() + x64 @ wr.t() + b).square().sum(), ref_in)
    for new, old, want in zip(grads[True], grads[False], ref):
        assert new.dtype == dtype
        e_new = float((new.cpu().double() - want).abs().max())
        e_old = float((old.cpu().double() - want).abs().max())
        print(f'max-norm error: new {e_new:.4g}, generic {e_old:.4g}, |ref| {float(want.abs().max()):.4g}')
        assert e_new <= 2 * e_old + U[dtype] * float(want.abs().max())
