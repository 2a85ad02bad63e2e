"""The propagation step of csrc/hop.hip, the recurrence built on it and the six layers (APPNP,
SGConv, SSGConv, TAGConv, LGConv, GCN2Conv) on the device: the reference's recorded cases with
their launch counts, the step against the float64 restatement on the degree-profile graph at three
hub settings, exact arithmetic through hub rows, aliasing, pitched operands, repeatability, the
recurrence and its backward's launch and pass counts, the layers' routes and width rule, the
registered operator, and sources placed past 2^31 elements."""
import itertools
import os
import sys

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _degree_cases as D  # noqa: E402
import _hops_ref as R  # noqa: E402
import _large_cases as L  # noqa: E402
from _util import _counted, assert_close_scaled  # noqa: E402

pytestmark = pytest.mark.gpu

G = R.load_golden()
WIDTHS = (1, 3, 7, 16, 47, 64, 100, 256, 520)
SETTINGS = D.SETTINGS + (None, )          # None: the package's own threshold and chunk


def _hops(c):
    return c.calls.get('pygamd_hop', 0)


def _none_of(c, *parts):
    return not [n for n in c.calls if any(p in n for p in parts)]


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', sorted(R.FUSED_CASES))
def test_golden_cases_on_the_fused_route(dev, monkeypatch, name, index_dtype):
    """K launches forward and K backward per call, and nothing else that walks the edges"""
    case = G['cases'][name]
    calls = len(case['calls'])
    routes = []
    c = _counted(monkeypatch, lambda: R.check_class_case(
        G, name, dev, index_dtype=index_dtype, tol=2e-5, weight_grad=False, fuse=True,
        routes=routes))
    assert set(routes) == {'fused'}, routes
    K = R.FUSED_CASES[name]
    first = K if calls == 1 else (case['kwargs'].get('K', 1))      # (a cached call: its own K)
    want = 2 * K + (2 * first if calls == 2 else 0)
    if name in ('sg_cached', 'ssg_cached'):                         # the second call reads the cache
        want = 2 * first
    assert _hops(c) == want, c.calls
    assert _none_of(c, 'pygamd_spmm', 'pygamd_scatter'), c.calls


@pytest.mark.parametrize('name', sorted(k for k, v in R.CASES.items() if v is None)
                         + ['appnp_given', 'tag_given', 'lg_given'])
def test_golden_cases_on_the_generic_route(dev, monkeypatch, name):
    """``aggr='mean'`` and edge weights that take a gradient: no launch of the step"""
    routes = []
    c = _counted(monkeypatch, lambda: R.check_class_case(G, name, dev, tol=2e-5, fuse=True,
                                                         routes=routes))
    assert set(routes) == {'generic'}, routes
    assert _hops(c) == 0, c.calls


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
def test_golden_stack(dev, monkeypatch, index_dtype):
    sink = []
    c = _counted(monkeypatch, lambda: R.check_stack(G, dev, index_dtype=index_dtype, tol=2e-5,
                                                    fuse=True), sink=sink)
    assert _hops(c) == 2 * R.STACK_HOPS, c.calls
    assert _none_of(c, 'pygamd_spmm', 'pygamd_scatter'), c.calls
    widths = [i['F'] for i, _, _ in sink if i.get('kind') == 'hop']
    # TAGConv 16 -> 8 in Horner form at 8, SGConv 8 -> 12 at 8, APPNP at 12; the backward in reverse
    assert widths == [8, 8, 8, 8, 12, 12, 12] + [12, 12, 12, 8, 8, 8, 8], widths


# ---- the step on the degree-profile graph ----------------------------------------------------------
_PROBLEMS = {}


def _graph(setting, dev, index_dtype=torch.int64):
    """The profile graph of a setting on the device: both sorted forms with their hub plans at that
    setting, the in- and out-degrees (host) and per-edge weights in COO order"""
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.edge_index import EdgeIndex
    key = (setting, str(dev), index_dtype)
    if key not in _PROBLEMS:
        thr, chunk = setting or D.native_settings()
        ei, n, _ = D.build(0, thr, chunk)
        g = EdgeIndex(ei.to(dev).to(index_dtype), (n, n))
        fwd, bwd = g.by_dst(), g.by_src()
        plans = (_native.hub_plan(fwd.ptr, thr, chunk), _native.hub_plan(bwd.ptr, thr, chunk))
        assert plans[0].n_hub >= 8 and plans[1].n_hub >= 8
        in_deg, out_deg = D.degrees(ei, n)
        w = torch.rand(ei.size(1), generator=torch.Generator().manual_seed(9)) + 0.5
        _PROBLEMS[key] = {'ei': ei.to(dev), 'n': n, 'graph': g, 'forms': (fwd, bwd),
                          'plans': plans, 'deg': (in_deg, out_deg), 'w': w.to(dev)}
    return _PROBLEMS[key]


def _planes(n, F, dev, seed, count=4, misaligned=False):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        t = torch.randn(n, F, generator=g).to(dev)
        if misaligned:               # the base 4 bytes past a 16-byte boundary
            buf = torch.empty(n * F + 1, device=dev)
            buf[1:].copy_(t.reshape(-1))
            t = buf[1:].view(n, F)
            assert t.data_ptr() % 16 == 4
        out.append(t)
    return out


def _run_step(P, side, x, w, use_eid, a, y, b, z, c, s, d, sum_init=False, want_out=True,
              out=None):
    """One launch over the by-destination (side 0) or by-source (side 1) form; ``w`` in COO order,
    read through the form's permutation or, ``use_eid`` false, given in slot order"""
    from pytorch_geometric_amd import _native
    form, plan = P['forms'][side], P['plans'][side]
    eid, ws = form.perm, w
    if w is not None and not use_eid:
        eid, ws = None, w[form.perm.long()].contiguous()
    return _native.hop(form.ptr, form.idx, eid, ws, x, a, y=y, b=b, z=z, c=c, out=out,
                       want_out=want_out, sum=s, d=d, sum_init=sum_init, hub=plan)


def _ref_step(P, side, x, w, a, y, b, z, c, dtype):
    ei = P['ei'] if side == 0 else P['ei'].flip(0)
    cast = lambda t: None if t is None else t.to(dtype)      # noqa: E731
    return R.step(ei, cast(w), x.to(dtype), P['n'], a, cast(y), b, cast(z), c)


@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('setting', SETTINGS)
def test_step_matches_float64_on_the_profile_graph(dev, setting, F):
    """Every subset of {y, z, sum}, with and without weights and the edge map, by destination;
    weights and the edge map by source (the backward's launch); per row at 2e-5 of its scale"""
    P = _graph(setting, dev)
    n = P['n']
    rows = torch.arange(n)
    a, b, c, d = 0.9, 0.1, -0.75, 0.3
    x, y, z, s0 = _planes(n, F, dev, 70 + F)
    for side in (0, 1):
        lengths = P['deg'][side]
        for w in (None, P['w']):
            t64 = _ref_step(P, side, x, w, 1.0, None, 0, None, 0, torch.float64)
            combos = list(itertools.product((False, True), repeat=3)) if side == 0 else \
                [(True, False, False)]
            for use_eid in ((False, True) if w is not None else (True, )):
                for has_y, has_z, has_s in combos:
                    want = a * t64
                    if has_y:
                        want = want + b * y.double()
                    if has_z:
                        want = want + c * z.double()
                    s = s0.clone() if has_s else None
                    got = _run_step(P, side, x, w, use_eid, a, y if has_y else None, b,
                                    z if has_z else None, c, s, d)
                    what = f'setting {setting} F {F} side {side} w {w is not None} eid {use_eid} ' \
                           f'y {has_y} z {has_z} sum {has_s}'
                    D.assert_rows_close(got, want, rows, lengths, what=what + ' out')
                    if has_s:
                        D.assert_rows_close(s, s0.double() + d * want, rows, lengths,
                                            what=what + ' sum')
    if F == 16:      # the same rows from a base that is not 16-byte aligned: the scalar lane shape
        xm, ym, zm, sm = _planes(n, F, dev, 70 + F, misaligned=True)
        om = torch.empty(n * F + 1, device=dev)[1:].view(n, F)
        sm0 = sm.clone()
        _run_step(P, 0, xm, P['w'], True, a, ym, b, zm, c, sm, d, out=om)
        t64 = _ref_step(P, 0, x, P['w'], 1.0, None, 0, None, 0, torch.float64)
        want = a * t64 + b * y.double() + c * z.double()
        D.assert_rows_close(om, want, rows, P['deg'][0], what='misaligned out')
        D.assert_rows_close(sm, sm0.double() + d * want, rows, P['deg'][0], what='misaligned sum')


def _integers(n, F, dev, seed, count=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-8, 9, (n, F), generator=g).float().to(dev) for _ in range(count)]


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('F', [5, 64, 520])
@pytest.mark.parametrize('setting', SETTINGS)
def test_step_is_exact_on_integers(dev, setting, F, index_dtype):
    """Integer planes, power-of-two weights and coefficients: every row sum is representable, so
    the result equals the restatement whatever the order — through ordinary rows, hub rows (the
    chunk merge) and the epilogue, which a hub row must get exactly once"""
    P = _graph(setting, dev, index_dtype)
    n = P['n']
    x, y, z, s0 = _integers(n, F, dev, 90 + F)
    g = torch.Generator().manual_seed(3)
    w = (2.0 ** torch.randint(-1, 2, (P['ei'].size(1), ), generator=g).float()).to(dev)
    a, b, c, d = 0.5, 2.0, -0.25, 4.0
    for side in (0, 1):
        for wt in (None, w):
            want = _ref_step(P, side, x, wt, a, y, b, z, c, torch.float32)
            s = s0.clone()
            got = _run_step(P, side, x, wt, True, a, y, b, z, c, s, d)
            assert torch.equal(got, want), (setting, F, side, wt is not None)
            assert torch.equal(s, s0 + d * want), (setting, F, side, wt is not None, 'sum')
            hubs = P['plans'][side].rows.long()
            assert torch.equal(got[hubs], want[hubs]) and bool(want[hubs].abs().max() > 0)
    # the sum alone, started from zero
    s = torch.full_like(s0, float('nan'))
    assert _run_step(P, 0, x, w, True, a, y, b, None, 0.0, s, d, sum_init=True,
                     want_out=False) is None
    assert torch.equal(s, d * _ref_step(P, 0, x, w, a, y, b, None, 0.0, torch.float32))


def test_rows_without_slots_aliases_and_repeatability(dev):
    P = _graph((64, 48), dev)
    n, F = P['n'], 47
    a, b, c, d = 0.9, 0.1, -0.75, 0.3
    x, y, z, s0 = _planes(n, F, dev, 5)
    empty = torch.nonzero(P['deg'][0] == 0).flatten().to(dev)
    assert empty.numel() >= 1
    s = s0.clone()
    out = _run_step(P, 0, x, P['w'], True, a, y, b, z, c, s, d)
    want_empty = b * y[empty] + c * z[empty]
    assert torch.equal(out[empty], want_empty)                       # b y + c z, exactly
    assert torch.equal(s[empty], s0[empty] + d * want_empty)         # and the sum is still updated
    only_y = _run_step(P, 0, x, None, True, a, y, b, None, 0.0, None, 0.0)
    assert torch.equal(only_y[empty], b * y[empty])
    plain = _run_step(P, 0, x, None, True, a, None, 0.0, None, 0.0, None, 0.0)
    assert not bool(plain[empty].any()) and not bool(torch.signbit(plain[empty]).any())
    # two runs: the same bits
    s2 = s0.clone()
    again = _run_step(P, 0, x, P['w'], True, a, y, b, z, c, s2, d)
    assert torch.equal(out, again) and torch.equal(s, s2)
    # out is y, out is z: the bits of separate buffers
    for alias in ('y', 'z'):
        yy, zz = y.clone(), z.clone()
        target = yy if alias == 'y' else zz
        res = _run_step(P, 0, x, P['w'], True, a, yy, b, zz, c, None, 0.0, out=target)
        assert res.data_ptr() == target.data_ptr()
        assert torch.equal(res, out), alias
    # sum_init against a buffer of zeros
    s_init = torch.full_like(s0, float('nan'))
    _run_step(P, 0, x, P['w'], True, a, y, b, z, c, s_init, d, sum_init=True)
    s_zero = torch.zeros_like(s0)
    _run_step(P, 0, x, P['w'], True, a, y, b, z, c, s_zero, d)
    assert torch.equal(s_init, s_zero)
    # a coefficient of zero is a coefficient: 0 * NaN is NaN
    y_nan = y.clone()
    y_nan[3, 2] = float('nan')
    res = _run_step(P, 0, x, None, True, a, y_nan, 0.0, None, 0.0, None, 0.0)
    assert bool(torch.isnan(res[3, 2])) and int(torch.isnan(res).sum()) == 1


@pytest.mark.parametrize('F', [16, 47])
def test_pitched_operands_are_column_blocks_in_place(dev, F):
    """x, y, z, out and sum are column blocks of wider planes whose other columns hold NaN: the
    result is the compact run's, the neighbours are untouched and none of them was read"""
    P = _graph((64, 48), dev)
    n = P['n']
    a, b, c, d = 0.9, 0.1, -0.75, 0.3
    x, y, z, s0 = _planes(n, F, dev, 6)
    s = s0.clone()
    want = _run_step(P, 0, x, P['w'], True, a, y, b, z, c, s, d)

    def wide(t, left, right):
        plane = torch.full((n, left + F + right), float('nan'), device=dev)
        block = plane[:, left:left + F]
        if t is not None:
            block.copy_(t)
        return plane, block

    pads = {'x': (4, 8), 'y': (8, 4), 'z': (0, 12), 'out': (12, 4), 'sum': (4, 0)}
    if F == 47:
        pads = {'x': (3, 1), 'y': (1, 0), 'z': (0, 5), 'out': (2, 2), 'sum': (7, 3)}
    planes = {k: wide(t, *pads[k]) for k, t in (('x', x), ('y', y), ('z', z), ('out', None),
                                                 ('sum', s0))}
    got = _run_step(P, 0, planes['x'][1], P['w'], True, a, planes['y'][1], b, planes['z'][1], c,
                    planes['sum'][1], d, out=planes['out'][1])
    assert torch.equal(got, want) and torch.equal(planes['sum'][1], s)
    for k, (plane, _) in planes.items():
        left, right = pads[k]
        outside = torch.cat([plane[:, :left], plane[:, left + F:]], dim=1)
        assert bool(torch.isnan(outside).all()), f'{k}: a neighbouring column was written'
    assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(planes['sum'][1]).any())


# ---- the recurrence ----------------------------------------------------------------------------------
def _normalised(dev):
    """The profile graph at the package's setting with self-loops and gcn_norm weights"""
    key = ('normalised', str(dev))
    if key not in _PROBLEMS:
        from pytorch_geometric_amd.edge_index import EdgeIndex
        ei, n, _ = D.build(0)
        ei2, w = R.gcn_norm(ei, None, n, True, torch.float64)
        _PROBLEMS[key] = {'ei': ei2.to(dev), 'w64': w.to(dev), 'w': w.float().to(dev), 'n': n,
                          'graph': EdgeIndex(ei2.to(dev), (n, n))}
    return _PROBLEMS[key]


class _Passes(TorchDispatchMode):
    """The operators that produce a tensor of at least ``numel`` elements, allocations and views
    aside: the elementwise passes over an [N, F] plane"""
    FREE = ('empty', 'empty_like', 'empty_strided', 'new_empty', 'view', '_unsafe_view', 'reshape',
            'alias', 'detach', 'as_strided', 'slice', 'select', 'expand', 't', 'transpose',
            'permute', 'unsqueeze', 'squeeze', 'narrow', 'lift_fresh', '_to_copy')

    def __init__(self, numel):
        super().__init__()
        self.numel, self.ops = numel, []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.overloadpacket.__name__
        if isinstance(out, torch.Tensor) and out.numel() >= self.numel and name not in self.FREE:
            self.ops.append(name)
        return out


@pytest.mark.parametrize('F', [7, 128])
@pytest.mark.parametrize('K', [1, 2, 10])
def test_recurrence_matches_float64(dev, monkeypatch, K, F):
    """x_K, the running sum and the gradients of x and h against float64 at 2e-5 of the scale;
    exactly K launches forward and K backward"""
    from pytorch_geometric_amd._functions import HopsFunction
    P = _normalised(dev)
    n = P['n']
    a, b, d0, d = 0.9, 0.1, 0.2, 0.8 / K
    x0, h0, gx, gs = _planes(n, F, dev, 200 + F + K)
    x64 = x0.double().requires_grad_(True)
    h64 = h0.double().requires_grad_(True)
    xk64, s64 = R.recurrence(P['ei'], P['w64'], x64, h64, K, a, b, d0, d)
    want = torch.autograd.grad([xk64, s64], [x64, h64], [gx.double(), gs.double()])
    res = {}

    def forward():
        x, h = x0.clone().requires_grad_(True), h0.clone().requires_grad_(True)
        res['leaves'] = (x, h)
        res['out'] = HopsFunction.apply(x, h, P['w'], P['graph'], K, a, b, d0, d, True, False)

    def backward():
        res['grads'] = torch.autograd.grad(list(res['out']), list(res['leaves']), [gx, gs])

    P['graph'].fill_cache_()
    assert _hops(_counted(monkeypatch, forward)) == K
    c = _counted(monkeypatch, backward)
    assert _hops(c) == K and _none_of(c, 'pygamd_spmm', 'pygamd_scatter'), c.calls
    assert_close_scaled(res['out'][0], xk64.detach().float(), what='x_K')
    assert_close_scaled(res['out'][1], s64.detach().float(), what='s')
    assert_close_scaled(res['grads'][0], want[0].float(), what='grad_x')
    assert_close_scaled(res['grads'][1], want[1].float(), what='grad_h')
    # APPNP's form: h is x itself, nothing but x_K leaves
    xt = x0.clone().requires_grad_(True)
    out = HopsFunction.apply(xt, None, P['w'], P['graph'], K, a, b, 0.0, 0.0, False, True)
    c = _counted(monkeypatch, lambda: res.update(tied=torch.autograd.grad(out, xt, gx)[0]))
    assert _hops(c) == K
    x64 = x0.double().requires_grad_(True)
    xk64 = R.recurrence(P['ei'], P['w64'], x64, x64, K, a, b)[0]
    assert_close_scaled(out, xk64.detach().float(), what='tied x_K')
    assert_close_scaled(res['tied'], torch.autograd.grad(xk64, x64, gx.double())[0].float(),
                        what='tied grad_x')


@pytest.mark.parametrize('K', [2, 10])
def test_backward_makes_at_most_two_passes_whatever_K(dev, K):
    """Besides its K launches the backward of the recurrence touches an [N, F] plane at most twice
    (one pass joins the two incoming gradients, one finishes grad_h) — and not at all for APPNP"""
    from pytorch_geometric_amd import _onepass
    P = _normalised(dev)
    n, F = P['n'], 7
    gx, gs = _planes(n, F, dev, 300, count=2)
    slots = _onepass.Slots.of_graph(P['graph'])
    slots.by_src().hub
    with _Passes(n * F) as general:
        _onepass.hops_backward(slots, P['w'], K, 0.9, 0.1, 0.2, 0.4, gx, gs, has_h=True,
                               want_x=True, want_h=True)
    assert len(general.ops) <= 2, general.ops
    with _Passes(n * F) as tied:
        _onepass.hops_backward(slots, P['w'], K, 0.9, 0.1, 0.0, 0.0, gx, None, has_h=True,
                               tied=True, want_x=True)
    assert tied.ops == [], tied.ops
    with _Passes(n * F) as summed:       # SSGConv: the running sum alone
        _onepass.hops_backward(slots, P['w'], K, 1.0, 0.0, 0.2, 0.4, None, gs, want_x=True)
    assert len(summed.ops) <= 1, summed.ops


def test_zero_steps_return_the_input(dev):
    from pytorch_geometric_amd.nn import APPNP, SGConv
    P = _normalised(dev)
    x = torch.randn(P['n'], 7, device=dev)
    ei = P['ei'].clone()          # (the handle cache keeps a weak reference: not to a shared tensor)
    layer = APPNP(0, 0.1)
    layer.fuse = True
    assert layer(x, ei) is x
    sg = SGConv(7, 3, K=0).to(dev)
    sg.fuse = True
    assert torch.equal(sg(x, ei), sg.lin(x))


# ---- the layers --------------------------------------------------------------------------------------
def _layer_problem(dev, F, seed=11):
    ei, n, _ = D.build(0, 64, 48)
    g = torch.Generator().manual_seed(seed)
    return ei.to(dev), n, torch.randn(n, F, generator=g).to(dev)


def _run_layer(layer, x0, *args):
    x = x0.clone().requires_grad_(True)
    out = layer(x, *args)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(out.device)
    params = list(layer.parameters())
    grads = torch.autograd.grad(out, [x] + params, go, allow_unused=True)
    return [out.detach()] + [g for g in grads]


def test_appnp_dropout_agrees_with_the_generic_route(dev, monkeypatch):
    """Every step draws its own F.dropout(edge_weight) where the reference does: under one seed
    the two routes see the same masks"""
    from pytorch_geometric_amd.nn import APPNP
    ei, n, x = _layer_problem(dev, 24)
    layer = APPNP(4, 0.1, dropout=0.5)
    layer.train()
    res = {}
    for fuse in (True, False):
        layer.fuse = fuse
        torch.manual_seed(5)
        c = _counted(monkeypatch, lambda: res.update({fuse: _run_layer(layer, x, ei)}))
        assert _hops(c) == (8 if fuse else 0), c.calls
    for got, want in zip(res[True], res[False]):
        assert_close_scaled(got, want, what='dropout')
    layer.eval()
    layer.fuse = True
    assert not torch.equal(_run_layer(layer, x, ei)[0], res[True][0])       # (the masks did bite)


@pytest.mark.parametrize('cls,kw', [('SGConv', dict(K=2)), ('SSGConv', dict(alpha=0.2, K=2)),
                                    ('TAGConv', dict(K=3))])
@pytest.mark.parametrize('fin,fout', [(128, 16), (16, 128)])
def test_layers_propagate_at_the_narrow_width(dev, monkeypatch, cls, kw, fin, fout):
    """out < in: transform first (TAGConv: the Horner form), so every launch runs at the output
    width; out > in: at the input width.  Either way the reference's order gives the same result"""
    from pytorch_geometric_amd import nn
    ei, n, x = _layer_problem(dev, fin)
    torch.manual_seed(2)
    layer = getattr(nn, cls)(fin, fout, **kw).to(dev)
    res, sink = {}, []
    layer.fuse = True
    c = _counted(monkeypatch, lambda: res.update(fused=_run_layer(layer, x, ei)), sink=sink)
    K = kw['K']
    assert _hops(c) == 2 * K, c.calls
    widths = [i['F'] for i, _, _ in sink if i.get('kind') == 'hop']
    assert widths == [min(fin, fout)] * (2 * K), widths
    layer.fuse = False
    c = _counted(monkeypatch, lambda: res.update(generic=_run_layer(layer, x, ei)))
    assert _hops(c) == 0, c.calls
    for got, want in zip(res['fused'], res['generic']):
        assert_close_scaled(got, want, what=f'{cls} {fin} -> {fout}')


def test_routing(dev, monkeypatch):
    from pytorch_geometric_amd.nn import APPNP, GCN2Conv, LGConv
    ei, n, x = _layer_problem(dev, 16)
    w = torch.rand(ei.size(1), device=dev) + 0.5

    def hops(layer, *args):
        return _hops(_counted(monkeypatch, lambda: _run_layer(layer, *args)))

    layer = APPNP(3, 0.1)
    layer.fuse = True
    assert hops(layer, x, ei) == 6 and hops(layer, x, ei, w) == 6
    assert layer.hop_route(x, ei, w) == 'fused'
    wg = w.clone().requires_grad_(True)
    assert layer.hop_route(x, ei, wg) == 'generic' and hops(layer, x, ei, wg) == 0
    layer.fuse = False
    assert layer.hop_route(x, ei) == 'generic' and hops(layer, x, ei) == 0
    mean = APPNP(3, 0.1, aggr='mean')
    mean.fuse = True
    assert mean.hop_route(x, ei) == 'generic' and hops(mean, x, ei) == 0
    layer.fuse = True
    assert layer.hop_route(x.half(), ei) == 'generic'
    assert layer.hop_route(x.cpu(), ei.cpu()) == 'generic'
    c = _counted(monkeypatch, lambda: _run_layer(layer, x.cpu(), ei.cpu()))
    assert _hops(c) == 0
    lg = LGConv()
    lg.fuse = True
    assert hops(lg, x, ei) == 2
    torch.manual_seed(0)
    gcn2 = GCN2Conv(16, 0.1, theta=0.5, layer=2).to(dev)
    gcn2.fuse = True
    x_0 = torch.randn(n + 5, 16, device=dev)
    assert hops(gcn2, x, x_0, ei) == 2
    fused = _run_layer(gcn2, x, x_0, ei)
    gcn2.fuse = False
    assert hops(gcn2, x, x_0, ei) == 0
    for got, want in zip(fused, _run_layer(gcn2, x, x_0, ei)):
        assert_close_scaled(got, want, what='GCN2Conv')


def test_target_to_source_flow(dev, monkeypatch):
    """flow='target_to_source': the handle is built from the flipped list, the degree is the
    receiver's (edge_index[0]); both routes agree and the fused one stays fused"""
    from pytorch_geometric_amd.nn import APPNP, TAGConv
    ei, n, x = _layer_problem(dev, 16)
    torch.manual_seed(3)
    for layer, hops in ((APPNP(3, 0.1, flow='target_to_source'), 6),
                        (TAGConv(16, 4, K=2, flow='target_to_source').to(dev), 4)):
        res = {}
        layer.fuse = True
        c = _counted(monkeypatch, lambda: res.update(fused=_run_layer(layer, x, ei)))
        assert _hops(c) == hops, c.calls
        layer.fuse = False
        res['generic'] = _run_layer(layer, x, ei)
        for got, want in zip(res['fused'], res['generic']):
            assert_close_scaled(got, want, what=f'{type(layer).__name__} target_to_source')
    x64 = x.double()
    ei2, w = R.gcn_norm(ei.flip(0), None, n, True, torch.float64)
    want = R.recurrence(ei2, w, x64, x64, 3, 0.9, 0.1)[0]
    flipped = APPNP(3, 0.1, flow='target_to_source')
    flipped.fuse = True
    assert_close_scaled(flipped(x, ei), want.float(), what='against the flipped restatement')


def test_handle_inputs_normalise_once(dev, monkeypatch):
    from pytorch_geometric_amd.edge_index import EdgeIndex
    from pytorch_geometric_amd.nn import APPNP
    ei, n, x = _layer_problem(dev, 16)
    handle = EdgeIndex(ei, (n, n))
    layer = APPNP(3, 0.1)
    layer.fuse = True
    want = _run_layer(layer, x, ei)
    got = _run_layer(layer, x, handle)
    for g, w in zip(got, want):
        assert_close_scaled(g, w, what='handle')
    c = _counted(monkeypatch, lambda: _run_layer(layer, x, handle))      # the derived graph is kept
    assert _hops(c) == 6 and _none_of(c, 'pygamd_index_sort', 'pygamd_scatter'), c.calls


# ---- the registered operator -------------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops  # noqa: F401 (registers torch.ops.pyg_amd.*)
    op = torch.ops.pyg_amd.hop
    ei, n, x0 = _layer_problem(dev, 24)
    order = torch.argsort(ei[1], stable=True)
    col = ei[0][order].contiguous()
    ptr = torch._convert_indices_from_coo_to_csr(ei[1][order], n)
    eid = order
    g = torch.Generator().manual_seed(4)
    w = (torch.rand(ei.size(1), generator=g) + 0.5).to(dev)
    y0, z0, go = (torch.randn(n, 24, generator=g).to(dev) for _ in range(3))

    def fn(x, y, z):
        return (op(ptr, col, eid, w, x * 1.0, 0.9, y, 0.1, z, -0.5) * go).sum()

    def leaves():
        return [t.clone().requires_grad_(True) for t in (x0, y0, z0)]

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        out = f(*ls)
        results.append([out.detach()] + list(torch.autograd.grad(out, ls)))
    for got, want in zip(*results):
        assert torch.equal(got, want), 'compiled vs eager'
    x64 = x0.double().requires_grad_(True)
    want = R.step(ei, w.double(), x64, n, 0.9, y0.double(), 0.1, z0.double(), -0.5)
    gx = torch.autograd.grad(want, x64, go.double())[0]
    assert_close_scaled(op(ptr, col, eid, w, x0, 0.9, y0, 0.1, z0, -0.5), want.detach().float())
    assert_close_scaled(results[0][1], gx.float(), what='grad_x')
    assert torch.equal(results[0][2], go * 0.1) and torch.equal(results[0][3], go * -0.5)
    # edge_id = None: w follows the slots of col
    assert torch.equal(op(ptr, col, None, w[eid], x0, 0.9, y0, 0.1, z0, -0.5),
                       op(ptr, col, eid, w, x0, 0.9, y0, 0.1, z0, -0.5))
    torch.library.opcheck(op, (ptr, col, eid, w, x0.clone().requires_grad_(True), 0.9,
                               y0.clone().requires_grad_(True), 0.1, None, 0.0))


# ---- past 2^31 elements ------------------------------------------------------------------------------
def test_sources_placed_past_two_to_the_31_elements(dev):
    """The step with y on the profile graph at (64, 48) with its sources spread over R rows, R * F
    just over 2^31 elements, rows on both sides of 2^29, 2^30 and 2^31: the same bits as the
    compact run (a strictly increasing placement keeps every row's slot order and the hub plan);
    the rows nobody reads hold NaN.  Every row offset of csrc/hop.hip is an int64_t."""
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.edge_index import EdgeIndex
    F = 100
    P = _graph(L.SETTING, dev)
    n = P['n']
    x, y = _planes(n, F, dev, 12, count=2)
    want = _run_step(P, 0, x, P['w'], True, 0.9, y, 0.1, None, 0.0, None, 0.0)
    R_rows = L.rows_for(F)
    pl, info = L.place(n, R_rows, [(F, 0)], P['deg'][1], L.SETTING[0])
    assert info['boundary'] and R_rows * F > 2 ** 31
    ei = P['ei'].clone()
    ei[0] = pl.to(dev)[ei[0]]
    big = L.expand(x, R_rows, pl, float('nan'), dev)
    g = EdgeIndex(ei, (R_rows, n))
    fwd = g.by_dst()
    plan = _native.hub_plan(fwd.ptr, *L.SETTING)
    assert plan.n_chunks == P['plans'][0].n_chunks
    got = _native.hop(fwd.ptr, fwd.idx, fwd.perm, P['w'], big, 0.9, y=y, b=0.1, hub=plan)
    assert torch.equal(got, want)
