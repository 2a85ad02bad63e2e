"""nn.SplineConv on the device: the fused route (csrc/spline.hip) and ``spline_basis`` against the
float64 restatement of tests/_spline_ref.py on one small bipartite graph with an empty destination
and source, a split destination and a split source and pseudo-coordinates at exact 0 and 1;
``grad_pseudo`` per degree, the generic routes, and pseudo-coordinates outside [0, 1].

Bounds as in tests/test_gpu_mixture.py: 2e-5 of the tensor's largest magnitude, or 4 x the error of
the SAME restatement run in float32 on the host where that is larger (the device sums in another
order).  Figures measured on one gfx950 device are in profiles/spline_conv.md."""
import itertools

import pytest
import torch

import _spline_ref as R
from _util import _counted, gen

pytestmark = pytest.mark.gpu

TOL = 2e-5
N_SRC, N_DST, HUB = 37, 23, 700
KS, OPEN = [3, 4, 5], [True, False, True]
WIDTHS = [(1, 4), (8, 33), (65, 64), (130, 16)]
COLLECT, EXPAND, PGRAD = 'pygamd_spline_collect', 'pygamd_spline_expand', 'pygamd_spline_pseudo_grad'
# every (dim, degree) twice; the widths, the aggregation and the index dtype cycle so that each of
# their values meets each dim and each degree
CASES = [(dim, degree, *WIDTHS[(3 * dim + degree + r) % 4], ('add', 'mean')[(dim + degree + r) % 2],
          (torch.int32, torch.int64)[(degree + r) % 2])
         for dim, degree, r in itertools.product((1, 2, 3), (1, 2, 3), (0, 1))]


def _edges():
    """about 300 random edges that leave destination 22 and source 36 alone, 700 more into
    destination 0 and 700 more out of source 1, in arbitrary order"""
    g = gen(11)
    def rand(n, hi): return torch.randint(0, hi, (n, ), generator=g)
    src = torch.cat([rand(300, N_SRC - 1), rand(HUB, N_SRC - 1), torch.ones(HUB, dtype=torch.int64)])
    dst = torch.cat([rand(300, N_DST - 1), torch.zeros(HUB, dtype=torch.int64), rand(HUB, N_DST - 1)])
    return torch.stack([src, dst])[:, torch.randperm(src.numel(), generator=g)]


EI = _edges()
_HANDLES = {}


def _handle(dev, monkeypatch, index_dtype):
    """The graph's handle with its 700-slot rows SPLIT: they exceed ``PYGAMD_HUB_CHUNK`` (256) but
    not the default split threshold (1024), so the plan is made at a threshold of 512; a plan
    carries the threshold it was made for, so the handle stays valid afterwards."""
    from pytorch_geometric_amd import _native, as_edge_index
    if index_dtype not in _HANDLES:
        monkeypatch.setattr(_native, 'HUB_THRESHOLD', 512)
        graph = as_edge_index(EI.to(dev).to(index_dtype), N_SRC, N_DST)
        assert graph.by_dst().hub.n_hub == 1 and graph.by_src().hub.n_hub == 1
        assert graph.by_dst().hub.n_chunks == 3 and graph.by_src().hub.n_chunks == 3
        monkeypatch.undo()
        _HANDLES[index_dtype] = graph
    return _HANDLES[index_dtype]


def _pseudo(dim, degree, seed, off_knots=False, ks=KS):
    """exact 0.0 and 1.0 among uniform draws; ``off_knots``: every ``v = pseudo * span`` at least
    0.05 from an integer instead (the degree-1 derivative jumps at the knots)"""
    g = gen(seed)
    p = torch.rand(EI.size(1), dim, generator=g)
    if off_knots:
        for d in range(dim):
            span = ks[d] - degree * OPEN[d]
            if span > 0:
                whole = torch.randint(0, span, (EI.size(1), ), generator=g)
                p[:, d] = (whole + 0.05 + 0.9 * p[:, d]) / span
    else:
        p[:5], p[5:10], p[10, 0] = 0.0, 1.0, 1.0
    return p


def _layer(dim, degree, F_in, F_out, aggr, kernel_size=None):
    from pytorch_geometric_amd.nn import SplineConv
    torch.manual_seed(7)
    conv = SplineConv((F_in, F_in), F_out, dim=dim, kernel_size=kernel_size or KS[:dim],
                      is_open_spline=OPEN[:dim], degree=degree, aggr=aggr)
    conv.bias.data.normal_()
    return conv


NAMES = ('out', 'x_src', 'x_dst', 'weight', 'lin.weight', 'bias', 'pseudo')


def _restated(conv, xs, xd, pseudo, go, dtype, want_pseudo):
    """output and gradients (in the order of NAMES) of the restatement in ``dtype`` on the host"""
    leaves = [t.detach().to(dtype).requires_grad_(True)
              for t in (xs, xd, conv.weight, conv.lin.weight, conv.bias, pseudo)]
    out = R.layer(leaves[2], leaves[3], leaves[4], leaves[0], leaves[1], leaves[5], EI, N_DST,
                  conv.kernel_size.tolist(), conv.is_open_spline.tolist(), conv.degree, conv.aggr)
    n = 6 if want_pseudo else 5
    return [out.detach()] + list(torch.autograd.grad(out, leaves[:n], go.to(dtype)))


def _device(conv, graph, xs, xd, pseudo, go, dev, want_pseudo):
    conv = conv.to(dev)
    leaves = [t.to(dev).requires_grad_(True) for t in (xs, xd)]
    pd = pseudo.to(dev).requires_grad_(want_pseudo)
    out = conv((leaves[0], leaves[1]), graph, pd)
    leaves += [conv.weight, conv.lin.weight, conv.bias] + ([pd] if want_pseudo else [])
    return [out.detach()] + list(torch.autograd.grad(out, leaves, go.to(dev)))


def _check(got, want64, want32, what):
    for name, g, w, w32 in zip(NAMES, got, want64, want32):
        g = g.detach().cpu().double()
        assert g.shape == w.shape, f'{what} {name}: shape'
        err, scale = float((g - w).abs().max()), max(float(w.abs().max()), 1.0)
        bound = max(TOL * scale, 4 * float((w32.double() - w).abs().max()))
        print(f'{what} {name}: max abs err {err:.3e}, scale {scale:.3e}, bound {bound:.3e}')
        assert bool(torch.isfinite(g).all()) and err <= bound, \
            f'{what} {name}: max abs err {err:.3e} vs bound {bound:.3e}'


def _run(dev, monkeypatch, conv, pseudo, index_dtype, seed, want_pseudo, fused):
    graph = _handle(dev, monkeypatch, index_dtype)
    g = gen(seed)
    F_in, F_out = conv.weight.size(1), conv.out_channels
    xs, xd = torch.randn(N_SRC, F_in, generator=g), torch.randn(N_DST, F_in, generator=g)
    go = torch.randn(N_DST, F_out, generator=g)
    want = [_restated(conv, xs, xd, pseudo, go, t, want_pseudo) for t in (torch.float64, torch.float32)]
    state = {}
    c = _counted(monkeypatch, lambda: state.update(
        got=_device(conv, graph, xs, xd, pseudo, go, dev, want_pseudo)))
    calls = tuple(c.calls.get(n, 0) for n in (COLLECT, EXPAND, PGRAD))
    assert calls == ((1, 1, int(want_pseudo)) if fused else (0, 0, 0)), c.calls
    return state['got'], want


@pytest.mark.parametrize('dim,degree,F_in,F_out,aggr,index_dtype', CASES)
def test_fused_layer_and_basis_match_float64(dev, monkeypatch, dim, degree, F_in, F_out, aggr,
                                             index_dtype):
    """One column per lane and the crossing of 64 and 128 columns on both sides of the weight; the
    bipartite graph of the module docstring (both chunk merges run); output and the gradients of
    x_src, x_dst, weight, lin.weight and bias; ``spline_basis`` on the same pseudo-coordinates."""
    from pytorch_geometric_amd.utils import spline_basis
    conv = _layer(dim, degree, F_in, F_out, aggr)
    pseudo = _pseudo(dim, degree, 20 + 3 * dim + degree)
    got, want = _run(dev, monkeypatch, conv, pseudo, index_dtype, 40 + F_in, False, True)
    _check(got, *want, f'({dim}, {degree}, {F_in}, {F_out}, {aggr})')
    b, wi = spline_basis(pseudo.to(dev), conv.kernel_size, conv.is_open_spline, degree)
    b64, wi64 = R.basis(pseudo, KS[:dim], OPEN[:dim], degree)
    assert b.dtype == torch.float32 and wi.dtype == torch.int64 and torch.equal(wi.cpu(), wi64)
    # a product of `dim` <= 3 cubics in [0, 1] evaluated in float32
    assert float((b.cpu().double() - b64).abs().max()) <= 1e-6


@pytest.mark.parametrize('degree', [1, 2, 3])
def test_pseudo_gradient(dev, monkeypatch, degree):
    """``edge_attr.requires_grad``: one more launch; pseudo-coordinates drawn off the knots"""
    conv = _layer(2, degree, 8, 33, 'mean')
    pseudo = _pseudo(2, degree, 60 + degree, off_knots=True)
    got, want = _run(dev, monkeypatch, conv, pseudo, torch.int64, 61, True, True)
    _check(got, *want, f'pseudo gradient, degree {degree}')


@pytest.mark.parametrize('what', ['outside the envelope', 'max'])
def test_generic_routes_match(dev, monkeypatch, what):
    """K * F_out = 1331 * 16 > 16384 bins, and ``aggr='max'``: no spline launch walks the graph,
    same bounds"""
    if what == 'max':
        conv = _layer(2, 2, 8, 33, 'max')
    else:
        conv = _layer(3, 1, 8, 16, 'mean', kernel_size=[11, 11, 11])
    pseudo = _pseudo(conv.dim, conv.degree, 70, off_knots=True, ks=conv.kernel_size.tolist())
    got, want = _run(dev, monkeypatch, conv, pseudo, torch.int64, 71, True, False)
    _check(got, *want, what)


def test_pseudo_outside_the_unit_interval(dev, monkeypatch):
    """-0.5, 1.5 and NaN on three edges into destination 3: the calls return, and every other
    destination's row is bitwise what it is with those three edges at 0.5"""
    graph = _handle(dev, monkeypatch, torch.int64)
    conv = _layer(2, 2, 8, 33, 'mean').to(dev)
    g = gen(80)
    xs, xd = torch.randn(N_SRC, 8, generator=g).to(dev), torch.randn(N_DST, 8, generator=g).to(dev)
    clean = _pseudo(2, 2, 81)
    into3 = (EI[1] == 3).nonzero().view(-1)[:3]
    clean[into3] = 0.5
    bad = clean.clone()
    bad[into3[0]], bad[into3[1]], bad[into3[2], 0] = -0.5, 1.5, float('nan')
    outs = []
    for p in (clean, bad):
        pd = p.to(dev).requires_grad_(True)
        out = conv((xs, xd), graph, pd)
        out.sum().backward()
        torch.cuda.synchronize()
        outs.append(out.detach().cpu())
    others = torch.arange(N_DST) != 3
    assert torch.equal(outs[0][others], outs[1][others])
    assert bool(torch.isnan(outs[1][3]).any()) and bool(torch.isfinite(outs[0]).all())
