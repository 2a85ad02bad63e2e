"""RGATConv on the device: the recorded cases of the real reference with counted launches, the
kernels of csrc/rgat.hip through the autograd node against the float64 restatement of
tests/_rgat_ref.py run on the device (the project's 2e-5 through ``assert_close_scaled``), exact
pre-activations, the row shapes of tests/_degree_cases.py, non-finite scores, and the routing of
the layer.

Launch budget (C-ABI calls, ``T._counted``): across-relation one forward; within-relation two (the
scalar launch over the pair rows first); three backward in either mode."""
import os
import subprocess
import sys

import pytest
import torch

import _degree_cases as D
import _rgat_ref as R
import test_gpu_transformer as T
from _util import assert_close, assert_close_scaled, gen, random_graph

pytestmark = pytest.mark.gpu

NAMES = ('out', 'alpha', 'grad_P', 'grad_QI', 'grad_KJ', 'grad_B')
TOL = 2e-5
SLOPE = 0.2


def _rgat_calls(c):
    return {k: v for k, v in c.calls.items() if k.startswith('pygamd_rgat_')}


def _check_launches(c, within, times=1):
    """One forward launch (within-relation: the scalar launch over the pair rows in front of it,
    two in all), three backward launches in either mode, and nothing else that aggregates or
    gathers over the edges"""
    calls = {k: v for k, v in _rgat_calls(c).items()
             if k != 'pygamd_rgat_supported'}
    if within:
        want = {'pygamd_rgat_pair_scalar': 2, 'pygamd_rgat_forward': 1,
                'pygamd_rgat_backward_dst': 1, 'pygamd_rgat_backward_src': 1}
    else:
        want = {'pygamd_rgat_forward': 1, 'pygamd_rgat_backward_dst': 1,
                'pygamd_rgat_backward_src': 2}
    assert calls == {k: v * times for k, v in want.items()}, calls
    assert not [n for n in c.calls if 'spmm' in n or 'scatter' in n or 'gather' in n], c.calls


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_the_device(dev, monkeypatch, name, index_dtype):
    c = T._counted(monkeypatch, lambda: R.check_class_case(R.load_golden(), name, dev,
                                                           index_dtype=index_dtype))
    if name in R.FUSED_CASES:
        _check_launches(c, within=name == 'within')
    else:
        assert not _rgat_calls(c), c.calls


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
def test_golden_stack_on_the_device(dev, monkeypatch, index_dtype):
    """layer 0 across-relation, layer 1 within-relation"""
    c = T._counted(monkeypatch, lambda: R.check_stack(R.load_golden(), dev,
                                                      index_dtype=index_dtype))
    calls = _rgat_calls(c)
    assert calls == {'pygamd_rgat_forward': 2, 'pygamd_rgat_pair_scalar': 2,
                     'pygamd_rgat_backward_dst': 2, 'pygamd_rgat_backward_src': 3}, calls


# ---- problems ---------------------------------------------------------------------------------------
def _grid(shape, g, span=16):
    return torch.randint(-span, span + 1, shape, generator=g).float() / 8


def _problem(n, ei, et, H, C, R_, seed, grid=False):
    """``P [n, R H C]``, ``QI`` / ``KJ [n, R H]``, ``B [E, H]`` and the cotangent; ``grid``: the
    scores' terms from the grid ``k / 8`` (every pre-activation exact, some exactly 0)"""
    g = gen(seed)
    E = ei.size(1)
    draw = (lambda s: _grid(s, g, 8)) if grid else (lambda s: torch.randn(s, generator=g))
    return {'ei': ei, 'et': et, 'n': n, 'H': H, 'C': C, 'R': R_,
            'P': torch.randn(n, R_ * H * C, generator=g), 'QI': draw((n, R_ * H)),
            'KJ': draw((n, R_ * H)), 'B': draw((E, H)),
            'go': torch.randn(n, H * C, generator=g)}


def _reference(Pr, within=False, bias=False, device='cuda'):
    """the six of NAMES from the float64 restatement run on ``device``, as CPU tensors (grad_B
    None without the bias)"""
    names = ('P', 'QI', 'KJ') + (('B', ) if bias else ())
    leaves = [Pr[n].to(device, torch.float64).requires_grad_(True) for n in names]
    ei, et = Pr['ei'].to(device), Pr['et'].to(device)
    out, alpha = R.rgat_attend(leaves[0], leaves[1], leaves[2], leaves[3] if bias else None,
                               ei[0], ei[1], et, Pr['n'], Pr['H'], Pr['C'], SLOPE, within)
    grads = torch.autograd.grad(out, leaves, Pr['go'].to(device, torch.float64))
    res = [out, alpha] + list(grads) + ([] if bias else [None])
    return [None if t is None else t.detach().cpu() for t in res]


def _forms(Pr, dev, index_dtype=torch.int64, sort=True):
    """``sort``: the forms as the layer builds them (relation sort, by-destination sort);
    otherwise a CSR pair of the edges in their own order, relations unsorted within the rows"""
    from pytorch_geometric_amd._onepass import RgatForms
    from pytorch_geometric_amd.edge_index import EdgeIndex
    ei = Pr['ei'].to(dev).to(index_dtype)
    et = Pr['et'].to(dev)
    if sort:
        return RgatForms.of_edges(ei[0].contiguous(), ei[1].contiguous(), et, Pr['n'], Pr['n'],
                                  Pr['R'])
    csr = EdgeIndex(ei, (Pr['n'], Pr['n'])).by_dst()
    perm = csr.perm.to(torch.int64)
    forms = RgatForms.of_csr(csr.ptr, csr.idx, et[perm].to(torch.int32), Pr['n'], Pr['R'])
    forms.perm = perm            # so that the node speaks the caller's edge order
    return forms


def _device_run(Pr, dev, index_dtype=torch.int64, packed=False, within=False, bias=False,
                sort=True):
    """the same six through the autograd node.  ``packed``: P, QI and KJ are the column blocks of
    one plane and the gradient is ONE plane of that shape"""
    from pytorch_geometric_amd._functions import RGATAggregateFunction
    H, C, R_ = Pr['H'], Pr['C'], Pr['R']
    if packed:
        p = torch.cat([Pr['P'], Pr['QI'], Pr['KJ']], dim=1).to(dev).requires_grad_(True)
        qi = kj = None
    else:
        p, qi, kj = [Pr[n].to(dev).requires_grad_(True) for n in ('P', 'QI', 'KJ')]
    b = Pr['B'].to(dev).requires_grad_(True) if bias else None
    key = ('forms', index_dtype, sort)
    if key not in Pr:
        Pr[key] = _forms(Pr, dev, index_dtype, sort)
    out, alpha = RGATAggregateFunction.apply(p, qi, kj, b, Pr[key], H, C, SLOPE, within)
    assert not alpha.requires_grad
    leaves = [t for t in (p, qi, kj, b) if t is not None]
    grads = dict(zip([id(t) for t in leaves], torch.autograd.grad(out, leaves, Pr['go'].to(dev))))
    if packed:
        plane = grads[id(p)]
        w, h = R_ * H * C, R_ * H
        assert plane.shape == (Pr['n'], w + 2 * h) and plane.is_contiguous()
        gs = [plane[:, :w], plane[:, w:w + h], plane[:, w + h:]]
    else:
        gs = [grads[id(t)] for t in (p, qi, kj)]
    return [out.detach(), alpha.detach()] + gs + [None if b is None else grads[id(b)]]


def _check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, f'{what}: {name} should be absent'
            continue
        assert g is not None, f'{what}: {name} is missing'
        assert_close_scaled(g, w.float(), tol=TOL, what=f'{what} {name}')


# ---- the kernels against float64 ------------------------------------------------------------------
_UNIFORM = {}


def _uniform_case(H, C, R_):
    """problem and float64 results at one shape, computed once"""
    key = (H, C, R_)
    if key not in _UNIFORM:
        ei = T._uniform_graph()
        et = torch.randint(0, R_, (ei.size(1), ), generator=gen(300 + R_))
        Pr = _problem(2000, ei, et, H, C, R_, 500 + 11 * H + C + 7 * R_)
        Pr['want'] = {(w, b): _reference(Pr, w, b) for w in (False, True) for b in (False, True)}
        _UNIFORM[key] = Pr
    return _UNIFORM[key]


@pytest.mark.parametrize('R_', [1, 4, 7])
@pytest.mark.parametrize('H,C', [(1, 1), (3, 5), (1, 48), (4, 32), (8, 64)])
def test_kernels_match_float64(dev, H, C, R_):
    """One channel, odd widths below a wave, a float4 width of one head, heads that share a wave
    and the 512 limit, with one, four and seven relations.  Both mechanisms, each with three
    separate tensors and with the column blocks of one plane, with and without the score bias."""
    Pr = _uniform_case(H, C, R_)
    for within in (False, True):
        for packed in (False, True):
            for bias in (False, True):
                got = _device_run(Pr, dev, within=within, packed=packed, bias=bias,
                                  index_dtype=torch.int32 if packed == bias else torch.int64)
                _check(got, Pr['want'][(within, bias)],
                       f'({H}, {C}, {R_}) within {within}, packed {packed}, bias {bias}')


@pytest.mark.parametrize('H,C,R_', [(3, 5, 4), (4, 32, 7)])
def test_the_other_pairings_and_unsorted_relations(dev, H, C, R_):
    """the relations of a row in the edge list's own order (the register reloads at every change
    of relation)"""
    Pr = dict(_uniform_case(H, C, R_))
    for within in (False, True):
        _check(_device_run(Pr, dev, within=within, bias=True, sort=False, packed=True),
               Pr['want'][(within, True)], f'unsorted, within {within}')
    forms = Pr[('forms', torch.int64, False)]
    rel, ptr = forms.rel.cpu().long(), forms.fwd.ptr.cpu().long()
    row = torch.repeat_interleave(torch.arange(ptr.numel() - 1), ptr[1:] - ptr[:-1])
    falls = (rel[1:] < rel[:-1]) & (row[1:] == row[:-1])
    assert int(falls.sum()) > 1000                              # not grouped by relation


@pytest.mark.parametrize('within', [False, True])
@pytest.mark.parametrize('H,C,R_', [(3, 5, 4), (4, 32, 2)])
def test_exact_pre_activations(dev, H, C, R_, within):
    """QI, KJ and B from the grid k / 8: every pre-activation is exact in float32, many are exactly
    0, where the leaky ReLU's derivative is the slope (as torch's).  The mask the kernels used is
    read off grad_B: with d alpha - D != 0, grad_B / (alpha (d alpha - D)) is 1 or the slope."""
    ei = T._uniform_graph()
    et = torch.randint(0, R_, (ei.size(1), ), generator=gen(310 + R_))
    Pr = _problem(2000, ei, et, H, C, R_, 77 + H, grid=True)
    t = R.rgat_scores(Pr['QI'].view(-1, R_, H), Pr['KJ'].view(-1, R_, H), Pr['B'], ei[0], ei[1],
                      et)
    t64 = R.rgat_scores(Pr['QI'].double().view(-1, R_, H), Pr['KJ'].double().view(-1, R_, H),
                        Pr['B'].double(), ei[0], ei[1], et)
    assert torch.equal(t.double(), t64)                       # exact
    zeros = int((t == 0).sum())
    assert zeros > 100, zeros
    want = _reference(Pr, within, True)
    got = _device_run(Pr, dev, within=within, bias=True)
    _check(got, want, f'grid, within {within}')
    # the mask: where the restatement's grad_B is clearly non-zero the two agree in sign and size,
    # on the zeros too (slope 0.2 against 1 is a factor of five)
    gb, wb = got[5].cpu().double(), want[5]
    at_zero = (t64 == 0) & (wb.abs() > 1e-3)
    assert int(at_zero.sum()) > 20
    ratio = gb[at_zero] / wb[at_zero]
    assert float((ratio - 1).abs().max()) < 0.5, float((ratio - 1).abs().max())


# ---- row shapes -------------------------------------------------------------------------------------
def _degree_problem(thr=None, chunk=None):
    ei, n, _ = D.build(0, thr, chunk)
    R_ = 3
    et = torch.randint(0, R_, (ei.size(1), ), generator=gen(900))
    first = int(torch.argmax(torch.bincount(ei[1], minlength=n)))
    et[ei[1] == first] = 1                 # a hub row that holds all of one relation
    return _problem(n, ei, et, 3, 5, R_, 901), first


@pytest.mark.parametrize('setting', [None, *D.SETTINGS])
def test_row_shapes(dev, monkeypatch, setting):
    """The graph of ``_degree_cases.build`` at the package's threshold and chunk and at the small
    pairs: every row length around the lane counts, the threshold and the chunk, judged per row.
    One hub row holds a single relation; in the other hub rows the sorted relations change inside
    chunks; with ``sort=False`` the relations of a row come unsorted."""
    from pytorch_geometric_amd import _native
    if setting is not None:
        monkeypatch.setattr(_native, 'HUB_THRESHOLD', setting[0])
        monkeypatch.setattr(_native, 'HUB_CHUNK', setting[1])
    thr, chunk = D.native_settings()
    Pr, first = _degree_problem(*(setting or (None, None)))
    n, ei, et = Pr['n'], Pr['ei'], Pr['et']
    in_deg, out_deg = D.degrees(ei, n)
    assert int((in_deg > thr).sum()) >= 2 and int(in_deg[first]) > thr
    assert bool((et[ei[1] == first] == 1).all())
    # a hub row whose chunks straddle relation changes: some other hub row holds >= 2 relations
    other = [int(r) for r in torch.nonzero(in_deg > thr).flatten() if int(r) != first]
    assert any(et[ei[1] == r].unique().numel() >= 2 for r in other)
    nodes = torch.arange(n)
    sides = {'out': (nodes, in_deg), 'alpha': (ei[1], in_deg), 'grad_P': (nodes, out_deg),
             'grad_QI': (nodes, in_deg), 'grad_KJ': (nodes, out_deg), 'grad_B': (ei[1], in_deg)}
    for within in (False, True):
        want = _reference(Pr, within, True)
        for sort in (True, False):
            got = _device_run(Pr, dev, within=within, bias=True, sort=sort, packed=sort)
            for name, gt, wt in zip(NAMES, got, want):
                row_of, lengths = sides[name]
                D.assert_rows_close(gt, wt, row_of, lengths, tol=TOL,
                                    what=f'{name} within {within} sort {sort} at {(thr, chunk)}')
    forms = Pr[('forms', torch.int64, True)]
    assert forms.fwd.hub.n_hub == int((in_deg > thr).sum())
    assert (forms.fwd.hub.threshold, forms.fwd.hub.chunk) == (thr, chunk)


# ---- non-finite scores ------------------------------------------------------------------------------
@pytest.mark.parametrize('within', [False, True])
def test_non_finite_scores(dev, within):
    """A -inf in KJ has weight 0; a softmax group whose every score is -inf is NaN in its own
    (row, head) only; an empty row is 0 with gradient 0 — all as the restatement gives them."""
    n, R_, H, C = 60, 2, 2, 6
    g = gen(41)
    src = torch.randint(0, n - 1, (600, ), generator=g)
    dst = torch.randint(0, n - 1, (600, ), generator=g)       # node n - 1: no incoming edge
    src[src == 9] = 10
    src[dst == 5] = 9
    et = torch.randint(0, R_, (600, ), generator=g)
    ei = torch.stack([src, dst])
    Pr = _problem(n, ei, et, H, C, R_, 42)
    kj = Pr['KJ'].view(n, R_, H)
    kj[3, :, 0] = float('-inf')          # source 3, head 0: weight 0 wherever it appears
    kj[9, :, 1] = float('-inf')          # every edge into 5 comes from 9: head 1 of row 5 all -inf
    assert int((dst == 5).sum()) >= 2 and int((src == 3).sum()) >= 2
    want = _reference(Pr, within, False)
    got = _device_run(Pr, dev, within=within)
    out, alpha = got[0].cpu(), got[1].cpu()
    assert_close(out, want[0].float(), rtol=TOL, atol=TOL, what='out')      # NaN where NaN
    assert_close(alpha, want[1].float(), rtol=TOL, atol=TOL, what='alpha')
    from3 = (src == 3) & ~torch.isnan(alpha[:, 0])
    assert int(from3.sum()) >= 1 and bool((alpha[from3, 0] == 0).all())
    assert 5 in torch.isnan(out).any(1).nonzero().flatten().tolist()
    assert bool(torch.isnan(out[5, C:]).all()) and bool(torch.isfinite(out[5, :C]).all())
    assert bool((out[n - 1] == 0).all())
    assert bool((got[3].cpu()[n - 1] == 0).all())             # grad_QI of the empty row
    # the gradients: NaN exactly where the restatement's are (the all -inf groups and what they
    # feed), elsewhere — the zero-weight -inf slots included, where 0 * inf must not appear —
    # within 2e-5 of the tensor's finite scale
    for name, g, w in zip(NAMES[2:5], got[2:5], want[2:5]):
        g, w = g.cpu().double(), w
        nan = torch.isnan(w)
        assert bool(nan.any()) and torch.equal(torch.isnan(g), nan), f'{name}: NaN pattern'
        assert bool(torch.isfinite(g[~nan]).all()), f'{name}: non-finite where finite'
        scale = max(1.0, float(w[~nan].abs().max()))
        err = float((g[~nan] - w[~nan]).abs().max())
        assert err <= TOL * scale, f'{name}: {err:.3e} vs scale {scale:.3e}'
    kj_grad = got[4].cpu().view(n, R_, H)
    assert bool(torch.isfinite(kj_grad[3]).all())             # the -inf entries themselves


# ---- long rows, repeatability, memory -------------------------------------------------------------
def test_two_runs_are_bitwise_identical(dev, monkeypatch):
    from pytorch_geometric_amd import _native
    monkeypatch.setattr(_native, 'HUB_THRESHOLD', 64)
    monkeypatch.setattr(_native, 'HUB_CHUNK', 48)
    Pr, _ = _degree_problem(64, 48)
    for kw in (dict(bias=True), dict(within=True, packed=True, bias=True)):
        a, b = _device_run(Pr, dev, **kw), _device_run(Pr, dev, **kw)
        for name, x, y in zip(NAMES, a, b):
            assert torch.equal(x, y), f'{name} differs between two runs ({kw})'


@pytest.mark.parametrize('within', [False, True])
def test_keeps_nothing_of_edge_times_width(dev, within):
    """N = 2048, E = 131072, H = 2, C = 32, R = 2, so E >> N R.  Above the inputs and the warm
    forms, forward + backward allocate node-sized planes (out 0.5 MiB, the zero-filled gradient
    plane 1.1 MiB, the pair statistics) and [E, H] tensors (alpha, grad_s, the bias in slot order,
    its gradient back in edge order, alpha in edge order: 1 MiB each) — about 8 MiB with the
    allocator's rounding against 32 MiB for ONE [E, H C] float plane.  The bound, half such a
    plane, follows from that count, not from a measurement."""
    from pytorch_geometric_amd._functions import RGATAggregateFunction
    N, E, H, C, R_ = 2048, 131072, 2, 32, 2
    Pr = {'ei': random_graph(N, N, E, 71), 'et': torch.randint(0, R_, (E, ), generator=gen(70)),
          'n': N, 'R': R_}
    forms = _forms(Pr, dev)
    forms.pairs[0].hub, forms.pairs[1].hub, forms.fwd.hub, forms.inv      # (the handles warm)
    g = gen(72)
    plane = torch.randn(N, R_ * (H * C + 2 * H), generator=g).to(dev).requires_grad_(True)
    b = torch.randn(E, H, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(N, H * C, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, alpha = RGATAggregateFunction.apply(plane, None, None, b, forms, H, C, SLOPE, within)
    grads = torch.autograd.grad(out, [plane, b], go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'peak above the inputs: {extra / 2 ** 20:.1f} MiB (one [E, H C]: '
          f'{E * H * C * 4 / 2 ** 20:.0f} MiB)')
    assert extra < E * H * C * 4 / 2
    assert all(bool(torch.isfinite(t).all()) for t in grads)


# ---- routing --------------------------------------------------------------------------------------------
def _layer64(conv, x, ei, et, ea=None):
    state = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
    cfg = dict(heads=conv.heads, out_channels=conv.out_channels, num_relations=conv.num_relations,
               num_bases=conv.num_bases, num_blocks=conv.num_blocks, mod=conv.mod,
               concat=conv.concat, attention_mechanism=conv.attention_mechanism,
               attention_mode=conv.attention_mode, dim=conv.dim,
               negative_slope=conv.negative_slope)
    return R.rgat_layer(state, cfg, x, ei, et, ea)


def _small(dev, seed=5, **kw):
    from pytorch_geometric_amd.nn import RGATConv
    torch.manual_seed(seed)
    conv = RGATConv(16, 8, 3, **kw).to(dev)
    with torch.no_grad():
        for p in conv.parameters():         # (bias, b1, b2 start at zero: give them values)
            if not bool(p.any()):
                p.normal_(0, 0.3)
    conv.fuse = True
    x = torch.randn(300, 16, generator=gen(94)).to(dev)
    ei = random_graph(300, 300, 3000, 95).to(dev)
    et = torch.randint(0, 3, (3000, ), generator=gen(96)).to(dev)
    return conv, x, ei, et


@pytest.mark.parametrize('kw', [dict(heads=2, mod='scaled'), dict(heads=2, mod='f-scaled'),
                                dict(heads=3, concat=False), dict(heads=2, bias=False),
                                dict(heads=2, attention_mechanism='within-relation',
                                     mod='scaled', edge_dim=4)])
def test_node_level_pieces_through_the_layer(dev, monkeypatch, kw):
    """``scaled`` / ``f-scaled`` / ``concat=False`` / the bias are node-level code on the kernel's
    output: the fused layer against the float64 restatement of the whole layer"""
    conv, x, ei, et = _small(dev, **kw)
    ea = torch.randn(3000, 4, generator=gen(97)).to(dev) if 'edge_dim' in kw else None
    xg = x.clone().requires_grad_(True)
    state = {}

    def step():
        out, (_, alpha) = conv(xg, ei, et, ea, return_attention_weights=True)
        state.update(out=out, alpha=alpha, grad=torch.autograd.grad(out.sum(), [xg])[0])

    c = T._counted(monkeypatch, step)
    _check_launches(c, within='attention_mechanism' in kw)
    x64 = x.cpu().double().requires_grad_(True)
    out64, alpha64, _ = _layer64(conv, x64, ei.cpu(), et.cpu(),
                                 None if ea is None else ea.cpu().double())
    g64, = torch.autograd.grad(out64.sum(), [x64])
    assert_close_scaled(state['out'], out64.float(), tol=TOL, what='out')
    assert_close_scaled(state['alpha'], alpha64.float(), tol=TOL, what='alpha')
    assert_close_scaled(state['grad'], g64.float(), tol=TOL, what='grad_x')


def test_routing(dev, monkeypatch):
    """``fuse = False``, the multiplicative mode, ``mod='additive'``, training dropout,
    ``target_to_source``, a message hook and float64 take the generic route: no rgat call."""
    from pytorch_geometric_amd.nn import RGATConv
    conv, x, ei, et = _small(dev, heads=2)
    c = T._counted(monkeypatch, lambda: conv(x, ei, et).sum().backward())
    _check_launches(c, within=False)
    want = conv(x, ei, et)
    conv.fuse = False
    c = T._counted(monkeypatch, lambda: conv(x, ei, et))
    assert not _rgat_calls(c)
    assert_close_scaled(conv(x, ei, et), want, tol=TOL, what='generic against fused')
    conv.fuse = True
    handle = conv.register_message_forward_hook(lambda *a: None)
    assert not _rgat_calls(T._counted(monkeypatch, lambda: conv(x, ei, et)))
    handle.remove()
    assert _rgat_calls(T._counted(monkeypatch, lambda: conv(x, ei, et)))
    state = {}
    c = T._counted(monkeypatch, lambda: state.update(out=conv.double()(x.double(), ei, et)))
    assert not _rgat_calls(c) and state['out'].dtype == torch.float64   # never narrowed
    assert_close(state['out'], _layer64(conv, x.cpu().double(), ei.cpu(), et.cpu())[0],
                 rtol=1e-9, atol=1e-9, what='float64 on the device')
    for kw in (dict(attention_mode='multiplicative-self-attention', dim=2), dict(mod='additive'),
               dict(mod='f-additive'), dict(dropout=0.3), dict(flow='target_to_source')):
        other = RGATConv(16, 8, 3, heads=2, **kw).to(dev)
        other.fuse = True
        c = T._counted(monkeypatch, lambda: other(x, ei, et))
        assert not _rgat_calls(c), (kw, c.calls)
    dropped = RGATConv(16, 8, 3, heads=2, dropout=0.3).to(dev).eval()
    dropped.fuse = True
    assert _rgat_calls(T._counted(monkeypatch, lambda: dropped(x, ei, et)))   # eval: fused
    with pytest.raises(ValueError, match=r"must lie in \[0, 3\)"):
        conv.float()(x, ei, et + 1)
    with pytest.raises(ValueError, match="'edge_type' is required"):
        conv(x, ei)


def test_half_inputs_are_widened(dev, monkeypatch):
    """float16 and bfloat16 layers take the fused route, compute in float32 and hand the result
    back in their dtype: against the float32 layer whose parameters and inputs hold the SAME
    rounded values, the only difference is the last rounding to the low dtype."""
    import copy
    conv, x, ei, et = _small(dev, heads=2)
    for low, ulp in ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)):
        half = copy.deepcopy(conv).to(low)
        wide = copy.deepcopy(half).float()
        xl = x.to(low)
        want = wide(xl.float(), ei, et)
        state = {}
        c = T._counted(monkeypatch, lambda: state.update(out=half(xl, ei, et)))
        assert c.calls.get('pygamd_rgat_forward') == 1, (low, c.calls)
        assert state['out'].dtype == low
        assert_close(state['out'].float(), want, rtol=ulp, atol=1e-6, what=f'{low}')
        xg = xl.clone().requires_grad_(True)
        c = T._counted(monkeypatch, lambda: half(xg, ei, et).float().sum().backward())
        assert c.calls.get('pygamd_rgat_backward_dst') == 1, (low, c.calls)
        assert xg.grad.dtype == low and bool(torch.isfinite(xg.grad).all())


@pytest.mark.parametrize('low,ulp', [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)])
@pytest.mark.parametrize('kw,fuse', [(dict(heads=2, mod='scaled'), True),
                                     (dict(heads=2, mod='scaled', edge_dim=4), False),
                                     (dict(heads=2, mod='additive'), True)])
def test_half_layers_on_both_routes(dev, monkeypatch, kw, fuse, low, ulp):
    """a half / bf16 layer with ``mod='scaled'`` on the fused route (the degree factor meets the
    float32 degrees), with ``fuse = False`` and with ``mod='additive'`` (the generic route: every
    parameter meets widened data): computed in float32, handed back in the layer's dtype, one
    rounding away from the float32 layer that holds the same rounded values"""
    import copy
    conv, x, ei, et = _small(dev, **kw)
    conv.fuse = fuse
    half = copy.deepcopy(conv).to(low)
    wide = copy.deepcopy(half).float()
    xl = x.to(low)
    ea = torch.randn(3000, 4, generator=gen(97)).to(dev).to(low) if 'edge_dim' in kw else None
    want, (_, want_alpha) = wide(xl.float(), ei, et, None if ea is None else ea.float(),
                                 return_attention_weights=True)
    state = {}
    c = T._counted(monkeypatch, lambda: state.update(
        res=half(xl, ei, et, ea, return_attention_weights=True)))
    fused = fuse and kw.get('mod') != 'additive'
    assert bool(_rgat_calls(c)) is fused, c.calls
    got, (_, alpha) = state['res']
    assert got.dtype == low and alpha.dtype == low
    assert_close(got.float(), want, rtol=ulp, atol=1e-6, what=f'{low} out')
    assert_close(alpha.float(), want_alpha, rtol=ulp, atol=1e-6, what=f'{low} alpha')
    xg = xl.clone().requires_grad_(True)
    half(xg, ei, et, ea).float().sum().backward()
    assert xg.grad.dtype == low and bool(torch.isfinite(xg.grad).all())
    assert all(p.grad is None or p.grad.dtype == low for p in half.parameters())


def test_host_index_with_device_features_is_not_fused(dev, monkeypatch):
    """the fused route needs every tensor on the device, the index too: a host ``edge_index``
    never reaches the sorted forms (what the generic route makes of mixed devices is torch's)"""
    from pytorch_geometric_amd.nn.conv import rgat_conv
    conv, x, ei, et = _small(dev, heads=2)
    taken = []
    monkeypatch.setattr(rgat_conv.RGATConv, '_forward_fused',
                        lambda self, *a, **k: taken.append(1) or (None, None))
    try:
        conv(x, ei.cpu(), et)
    except Exception:
        pass
    assert not taken
    conv(x, ei, et)
    assert taken == [1]


def test_the_handles_are_cached_on_the_layer(dev, monkeypatch):
    conv, x, ei, et = _small(dev, heads=2)
    x = x.requires_grad_(True)

    def step():
        conv(x, ei, et).sum().backward()

    first = T._counted(monkeypatch, step)
    assert first.calls.get('pygamd_index_sort', 0) >= 2, first.calls
    forms = conv._rgat_cache[-1]
    again = T._counted(monkeypatch, step)
    assert 'pygamd_index_sort' not in again.calls, again.calls
    assert not [n for n in again.calls if 'hub_plan' in n or 'minmax' in n], again.calls
    _check_launches(again, within=False)
    assert conv._rgat_cache[-1] is forms
    et.add_(0)                                             # an in-place change: a new version
    changed = T._counted(monkeypatch, step)
    assert changed.calls.get('pygamd_index_sort', 0) >= 2 and conv._rgat_cache[-1] is not forms


def test_switch_off_in_a_child_process(dev):
    """``PYGAMD_FUSE_RGAT=0`` is read at import: a layer made in such a process starts with ``fuse
    = False`` and its forward on the device never reaches the rgat kernels; with ``1`` it does."""
    code = (
        "import os, torch\n"
        "from pytorch_geometric_amd import _native\n"
        "from pytorch_geometric_amd.nn import RGATConv\n"
        "seen = []\n"
        "inner = _native.rgat_forward\n"
        "def spy(*a, **k):\n"
        "    seen.append(1)\n"
        "    return inner(*a, **k)\n"
        "_native.rgat_forward = spy\n"
        "conv = RGATConv(8, 6, 2, heads=2).cuda()\n"
        "on = os.environ['PYGAMD_FUSE_RGAT'] == '1'\n"
        "assert conv.fuse is on\n"
        "x = torch.randn(50, 8, device='cuda')\n"
        "ei = torch.randint(0, 50, (2, 400), device='cuda')\n"
        "et = torch.randint(0, 2, (400, ), device='cuda')\n"
        "out = conv(x, ei, et)\n"
        "assert out.shape == (50, 12) and bool(torch.isfinite(out).all())\n"
        "assert bool(seen) is on\n"
        "print('route ok')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value in ('0', '1'):
        env = dict(os.environ, PYGAMD_FUSE_RGAT=value,
                   PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
        res = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True,
                             text=True, timeout=300)
        assert res.returncode == 0 and 'route ok' in res.stdout, res.stderr[-2000:]


# ---- the registered operators -----------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'rgat_aggregate' in ops.OPS and 'rgat_aggregate_backward' in ops.OPS
    op = torch.ops.pyg_amd.rgat_aggregate
    with FakeTensorMode():
        p = torch.empty(50, 4 * 15, device='cuda', requires_grad=True)
        qi = torch.empty(50, 12, device='cuda', requires_grad=True)
        kj = torch.empty(50, 12, device='cuda', requires_grad=True)
        plane = torch.empty(50, 4 * 21, device='cuda', requires_grad=True)
        b = torch.empty(400, 3, device='cuda', requires_grad=True)
        ptr = torch.empty(51, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        rel = torch.empty(400, dtype=torch.int32, device='cuda')
        for args in ((p, qi, kj, b, ptr, col, rel, 4, 3, 0.2, False),
                     (plane, None, None, None, ptr, col, rel, 4, 3, 0.2, True)):
            out, alpha = op(*args)
            assert out.shape == (50, 15) and alpha.shape == (400, 3) and out.requires_grad
            assert out.device.type == 'cuda' and out.dtype == torch.float32

    H, C, R_ = 1, 1, 4                                         # the smallest case
    Pr = _uniform_case(H, C, R_)
    forms = _forms(Pr, dev, sort=False)
    ptr, col, rel = forms.fwd.ptr, forms.fwd.idx, forms.rel
    perm = forms.perm
    b_slot = Pr['B'].to(dev)[perm].contiguous()
    go = Pr['go'].to(dev)
    for within in (False, True):
        want = Pr['want'][(within, True)]

        def fn(p, qi, kj, b):
            return (op(p * 1.0, qi, kj, b, ptr, col, rel, R_, H, SLOPE, within)[0] * go).sum()

        def leaves():
            return ([Pr[n].to(dev).requires_grad_(True) for n in ('P', 'QI', 'KJ')]
                    + [b_slot.clone().requires_grad_(True)])

        results = []
        for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
            ls = leaves()
            y = f(*ls)
            results.append([y.detach()] + list(torch.autograd.grad(y, ls)))
        for x, y in zip(*results):
            assert_close(y, x, what='compiled vs eager')
        out, alpha = op(*[t.detach() for t in leaves()], ptr, col, rel, R_, H, SLOPE, within)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel(), device=perm.device)
        g_p, g_qi, g_kj, g_b = results[0][1:]
        _check([out, alpha[inv], g_p, g_qi, g_kj, g_b[inv]], want, f'operator, within {within}')
    with pytest.raises(ValueError, match='rel'):               # a relation the planes do not hold
        op(*[t.detach() for t in leaves()], ptr, col, rel + 1, R_, H, SLOPE, False)
    torch.library.opcheck(op, (*leaves(), ptr, col, rel, R_, H, SLOPE, False))
    plane = torch.cat([Pr['P'], Pr['QI'], Pr['KJ']], dim=1).to(dev).requires_grad_(True)
    torch.library.opcheck(op, (plane, None, None, None, ptr, col, rel, R_, H, SLOPE, True))
