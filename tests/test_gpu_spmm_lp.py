"""The CSR aggregation over float16 / bfloat16 storage (csrc/spmm_lp.hip, ``pygamd_spmm_lp``)
against float64 on one small graph: 40 sources, 14 destinations with in-degrees 0, 1, 2, 63, 64,
65, 129, one hub row of ``3 * threshold + 5`` slots (hub plan at (160, 48): 11 chunks) and a source
with more than ``threshold`` out-edges (a hub row of the gradient's by-source walk); sources repeat.

Exact cases hold entries that are small integers / 8, so every float32 and float64 partial sum is
exact and the result must equal ``reference_float64.to(dtype)`` bit for bit.  Every fourth column
is a "tie column": the row ``[2^p, 1, 1, 1]`` (p = 8 bfloat16, 11 float16) — alone as row 8 and
spread over four chunks of the hub row — sums to ``2^p + 3``, a rounding tie that rounding per add
or per chunk gets wrong.  Row 9 sums four times 20480: ``inf`` in float16.

Rounded cases (``randn`` rounded to the dtype, float32 weights) are bounded elementwise by
``u |ref| + (deg + 3) 2^-24 sum_k |m_k x_k|``: the one final rounding (u = 2^-8 bfloat16, 2^-11
float16) plus the float32 accumulation, both terms from the float64 reference."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

PAIR = (160, 48)
N_SRC = 40
DEGS = [0, 1, 2, 63, 64, 65, 129, 3 * PAIR[0] + 5, 4, 4, 3, 0, 7, 5]
HUB, TIE, BIG = 7, 8, 9
WIDTHS = [1, 2, 6, 8, 24, 72, 520]
DTYPES = [torch.float16, torch.bfloat16]
IDX = [torch.int32, torch.int64]
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


@functools.lru_cache(None)
def _edges():
    src, dst = [], []
    for r, deg in enumerate(DEGS):
        for k in range(deg):
            s = (7 * k + 3 * r) % 35
            if r == HUB:
                s = 5 if k % 3 == 0 else s
                s = {0: 36, 100: 37, 200: 38, 300: 39}.get(k, s)
            elif r == TIE:
                s = 36 + k
            elif r == BIG:
                s = 35
            src.append(s)
            dst.append(r)
    return torch.tensor([src, dst])


def _handle(dev, idx, monkeypatch):
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd import _native
    monkeypatch.setattr(_native, 'HUB_THRESHOLD', PAIR[0])
    monkeypatch.setattr(_native, 'HUB_CHUNK', PAIR[1])
    h = pga.EdgeIndex(_edges().to(dev).to(idx), (N_SRC, len(DEGS))).fill_cache_()
    assert h.by_dst().hub.n_hub == 1 and h.by_dst().hub.n_chunks == 11
    assert h.by_src().hub.n_hub >= 1
    return h


@functools.lru_cache(None)
def _exact_x(dtype, F):
    g = torch.Generator().manual_seed(F)
    x = torch.randint(-16, 17, (N_SRC, F), generator=g).double() / 8
    x[:, ::4] = 0
    x[36, ::4] = 2.0 ** (8 if dtype == torch.bfloat16 else 11)
    x[37:40, ::4] = 1
    x[35] = 20480
    go = torch.randint(-16, 17, (len(DEGS), F), generator=g).double() / 8
    return x, go


def _dense(weight=None):
    """A[dst, src] = sum of the weights of the parallel edges (float64), and the same of |w|"""
    ei = _edges()
    w = torch.ones(ei.size(1), dtype=torch.float64) if weight is None else weight.double()
    A = torch.zeros(len(DEGS), N_SRC, dtype=torch.float64)
    return (A.clone().index_put_((ei[1], ei[0]), w, accumulate=True),
            A.index_put_((ei[1], ei[0]), w.abs(), accumulate=True))


def _minmax_reference(h, x, reduce):
    """(out, arg32) by the rule of pygamd_spmm_args.arg32_out over the handle's own slot order"""
    fwd = h.by_dst()
    ptr, col = fwd.ptr.cpu().long(), fwd.idx.cpu().long()
    out = torch.zeros(len(DEGS), x.size(1), dtype=torch.float64)
    arg = torch.full((len(DEGS), x.size(1)), -1, dtype=torch.int32)
    for r in range(len(DEGS)):
        c = col[ptr[r]:ptr[r + 1]]
        if c.numel() == 0:
            continue
        v = x[c]
        best = v.max(0).values if reduce == 'max' else v.min(0).values
        hit = v == best
        ids = c.view(-1, 1).expand_as(v)
        several = ids.masked_fill(~hit, -1).max(0).values != ids.masked_fill(~hit, N_SRC).min(0).values
        first = (hit & (hit.cumsum(0) == 1)).int().argmax(0)
        out[r] = best
        arg[r] = torch.where(several | (best == 0), -2, first).int()
    return out, arg


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize('F,layout', [(F, 'plain') for F in WIDTHS] + [(24, 'block')])
@pytest.mark.parametrize('idx', IDX, ids=['i32', 'i64'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['f16', 'bf16'])
def test_exact_sum_min_max(dev, monkeypatch, dtype, idx, F, layout):
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd import _native
    h = _handle(dev, idx, monkeypatch)
    x64, go64 = _exact_x(dtype, F)
    x = x64.to(dtype).to(dev)
    if layout == 'block':   # pitch 29, first column 3: 2-byte aligned rows, NaN neighbours
        plane = torch.full((N_SRC, F + 5), float('nan'), dtype=dtype, device=dev)
        plane[:, 3:3 + F] = x
        x = plane[:, 3:3 + F]
    x = x.requires_grad_(True)
    A, _ = _dense()
    out = pga.utils.spmm(h, x, 'sum')
    want = (A @ x64).to(dtype)
    assert out.dtype == dtype
    assert torch.equal(_bits(out.detach().cpu()), _bits(want))
    assert float(want[TIE, 0]) == float(want[HUB, 0]) == 2.0 ** (8 if dtype == torch.bfloat16 else 11) + 4
    if dtype == torch.float16:
        assert bool(torch.isinf(out[BIG]).all())
    grad, = torch.autograd.grad(out, [x], go64.to(dtype).to(dev))
    assert grad.dtype == dtype
    assert torch.equal(_bits(grad.cpu()), _bits((A.t() @ go64).to(dtype)))
    fwd = h.by_dst()
    for reduce in ('min', 'max'):
        got, arg = _native.spmm_csr_lp(fwd.ptr, fwd.idx, x.detach(), reduce, n_rows=fwd.n_rows,
                                       hub=fwd.hub, save_arg32=True)
        want, want_arg = _minmax_reference(h, x64, reduce)
        assert torch.equal(_bits(got.cpu()), _bits(want.to(dtype))), reduce
        assert torch.equal(arg.cpu(), want_arg), reduce


@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('idx', IDX, ids=['i32', 'i64'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['f16', 'bf16'])
def test_rounded_mean_and_weighted_sum(dev, monkeypatch, dtype, idx, F):
    import pytorch_geometric_amd as pga
    h = _handle(dev, idx, monkeypatch)
    g = torch.Generator().manual_seed(100 + F)
    x16 = torch.randn(N_SRC, F, generator=g).to(dtype)
    go16 = torch.randn(len(DEGS), F, generator=g).to(dtype)
    w = torch.randn(_edges().size(1), generator=g)
    x64, go64 = x16.double(), go16.double()
    deg = torch.tensor(DEGS, dtype=torch.float64).view(-1, 1)
    outdeg = _dense()[0].sum(0).view(-1, 1)
    for reduce, weight in (('mean', None), ('sum', w)):
        A, Aabs = _dense(weight)
        if reduce == 'mean':
            A, Aabs = A / deg.clamp(min=1), Aabs / deg.clamp(min=1)
        x = x16.to(dev).requires_grad_(True)
        out = pga.utils.spmm(h, x, reduce, None if weight is None else weight.to(dev))
        grad, = torch.autograd.grad(out, [x], go16.to(dev))
        for got, ref, mag, n in ((out, A @ x64, Aabs @ x64.abs(), deg),
                                 (grad, A.t() @ go64, Aabs.t() @ go64.abs(), outdeg)):
            assert got.dtype == dtype
            err = (got.detach().cpu().double() - ref).abs()
            bound = U[dtype] * ref.abs() + (n + 3) * 2.0 ** -24 * mag
            print(f'{reduce} F={F} worst err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}')
            assert bool((err <= bound).all())


@pytest.mark.parametrize('F', [6, 72])
@pytest.mark.parametrize('idx', IDX, ids=['i32', 'i64'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['f16', 'bf16'])
def test_minmax_gradient_is_the_float32_route_narrowed(dev, monkeypatch, dtype, idx, F):
    import pytorch_geometric_amd as pga
    h = _handle(dev, idx, monkeypatch)
    x64, go64 = _exact_x(dtype, F)
    for reduce in ('min', 'max'):
        grads = []
        for t in (dtype, torch.float32):
            x = x64.to(dtype).to(t).to(dev).requires_grad_(True)
            out = pga.utils.spmm(h, x, reduce)
            grads.append(torch.autograd.grad(out, [x], go64.to(t).to(dev))[0])
        assert grads[0].dtype == dtype
        assert torch.equal(_bits(grads[0].cpu()), _bits(grads[1].to(dtype).cpu())), reduce


def _count_lp(monkeypatch):
    from pytorch_geometric_amd import _native
    calls, real = [], _native.spmm_csr_lp

    def counted(rowptr, col, x, *args, **kwargs):
        calls.append(x.dtype)
        return real(rowptr, col, x, *args, **kwargs)

    monkeypatch.setattr(_native, 'spmm_csr_lp', counted)
    return calls


@pytest.mark.parametrize('dtype', DTYPES, ids=['f16', 'bf16'])
def test_routing_and_switch(dev, monkeypatch, dtype):
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd import _functions
    h = _handle(dev, torch.int64, monkeypatch)
    calls = _count_lp(monkeypatch)
    g = torch.Generator().manual_seed(7)
    x16 = torch.randn(N_SRC, 24, generator=g).to(dtype)
    go16 = torch.randn(len(DEGS), 24, generator=g).to(dtype)
    deg = torch.tensor(DEGS, dtype=torch.float64).view(-1, 1)
    A, Aabs = _dense()
    for flag, forward, backward in ((True, 1, 1), (False, 0, 0)):
        monkeypatch.setattr(_functions, 'SPMM_LP', flag)
        for reduce in ('sum', 'mean', 'max'):
            del calls[:]
            x = x16.to(dev).requires_grad_(True)
            out = pga.utils.spmm(h, x, reduce)
            assert len(calls) == forward
            grad, = torch.autograd.grad(out, [x], go16.to(dev))
            assert len(calls) == forward + (backward if reduce != 'max' else 0)
            assert out.dtype == dtype and grad.dtype == dtype
            if reduce != 'max':
                s = deg.clamp(min=1) if reduce == 'mean' else 1.0
                err = (out.detach().cpu().double() - (A / s) @ x16.double()).abs()
                bound = U[dtype] * ((A / s) @ x16.double()).abs() \
                    + (deg + 3) * 2.0 ** -24 * ((Aabs / s) @ x16.double().abs())
                assert bool((err <= bound).all())


def test_graph_conv_bfloat16_and_gcn_autocast(dev, monkeypatch):
    import torch.nn.functional as Fn
    import pytorch_geometric_amd as pga
    calls = _count_lp(monkeypatch)
    g = torch.Generator().manual_seed(11)
    ei = torch.randint(0, N_SRC, (2, 300), generator=g).to(dev)
    h = pga.EdgeIndex(ei, (N_SRC, N_SRC))
    x = torch.randn(N_SRC, 16, generator=g).to(dev)
    torch.manual_seed(0)
    conv = pga.nn.GraphConv(16, 8).to(dev).bfloat16()
    xb = x.bfloat16()
    out = conv(xb, h)
    want = Fn.linear(pga.utils.spmm(h, xb, 'sum'), conv.lin_rel.weight, conv.lin_rel.bias) \
        + Fn.linear(xb, conv.lin_root.weight)
    assert out.dtype == torch.bfloat16 and torch.equal(_bits(out), _bits(want))
    assert calls == [torch.bfloat16] * 2
    del calls[:]
    gcn = pga.nn.GCNConv(16, 8).to(dev)
    xg = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = gcn(xg, ei)
    out.float().sum().backward()
    assert calls and set(calls) == {torch.bfloat16}
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(xg.grad).all())
