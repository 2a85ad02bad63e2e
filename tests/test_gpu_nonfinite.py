"""Softmax, logsumexp, extremum and cross-entropy kernels on non-finite inputs: -inf masks, +inf,
NaN, 1e4- and 3e38-magnitude logits, subnormals, signed zeros, empty segments
(tests/_nonfinite_cases.py) — the HIP path against the real reference's recorded answers
(tests/golden/golden_nonfinite_v1.pt) and against the oracle on the CPU.

Rules used throughout:
  * forward: ``assert_close`` at 1e-5 (NaN for NaN, same-signed infinities); the 1e4 / 3e38
    segments are judged against a float64 evaluation as well (``assert_sum_close``);
  * backward: per (segment, column), a reference gradient that is finite everywhere must be
    matched at 1e-5; one that is non-finite anywhere must be non-finite somewhere here; the
    elements inside such a segment are not compared one by one;
  * isolation: whatever is ordinary in the input gives the result of the same call on a copy
    whose special values are replaced by ``randn`` — bit for bit on the routes without float
    atomics, within 1e-5 on the atomic ones.
"""
import pytest
import torch

from oracle import pyg_oracle as O
from tests import _nonfinite_cases as NF
from tests._util import assert_close, assert_close_scaled, assert_sum_close, gen
from tests.test_oracle_golden import nonfinite_calls

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
# routes without float atomics: the result on ordinary data must not depend on its neighbours
BITWISE = ('softmax_ptr', 'lse_dim0', 'lse_dim1', 'segment_sum', 'segment_mean', 'segment_min',
           'segment_max')


@pytest.fixture(scope='module')
def fx():
    return NF.load()


class Lib:
    """The package's calls under the oracle's names."""

    def __init__(self):
        from pytorch_geometric_amd import utils
        self.softmax, self.segment, self.scatter = utils.softmax, utils.segment, utils.scatter
        self.segment_logsumexp = utils.segment_logsumexp


def run_grad(fn, src, grad_out, device=None):
    x = src.clone().to(device or src.device).requires_grad_(True)
    out = fn(x)
    (grad, ) = torch.autograd.grad(out, [x], grad_out.to(out.device))
    return out.detach().cpu(), grad.cpu()


def group_all(flag, index, S):
    """[rows, H] bool -> [S, H]: true where every row of the group is (empty groups: true)."""
    out = torch.ones(S, flag.size(1))
    out.scatter_reduce_(0, index.view(-1, 1).expand_as(flag), flag.float(), 'amin')
    return out.bool()


def check_backward(got, ref, index, S, what):
    """The backward rule of the module docstring; ``index``: the segment of every row."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, what
    index = index.cpu().long()
    seg_ok = group_all(ref.isfinite(), index, S)
    ok = seg_ok[index]
    assert_close(torch.where(ok, got, 0), torch.where(ok, ref, 0), what=f'{what} (finite part)')
    got_ok = group_all(got.isfinite(), index, S)
    missing = ~seg_ok & got_ok
    assert not missing.any(), (f'{what}: {int(missing.sum())} (segment, column) pairs have a '
                               f'non-finite reference gradient and a finite one here: '
                               f'{missing.nonzero()[:4].tolist()}')


def special_mask(I, per_row, rows_index=None):
    """True at the elements the special values can reach: (rows of a special segment | the
    special segment, the special column)."""
    H, S = I['H'], len(I['kinds'])
    seg = torch.tensor([bool(k) for k in I['kinds']])
    index = I['index'] if rows_index is None else rows_index
    rows = seg[index] if per_row else seg
    mask = torch.zeros(rows.numel(), H, dtype=torch.bool)
    mask[:, I['col']] = rows
    return mask


def large_mask(I, per_row, rows_index=None):
    seg = torch.tensor([k in NF.LARGE for k in I['kinds']])
    index = I['index'] if rows_index is None else rows_index
    rows = seg[index] if per_row else seg
    mask = torch.zeros(rows.numel(), I['H'], dtype=torch.bool)
    mask[:, I['col']] = rows
    return mask


def clean_input(I, src):
    out = src.clone()
    out[:, I['col']] = I['clean_col']
    return out


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('H', NF.WIDTHS)
def test_calls_match_the_reference_and_isolate_special_values(dev, fx, H, dtype):
    """Every call of the fixture, forward and backward, under the three rules above."""
    I = fx[f'H{H}']
    NF.check_layout(H, I['kinds'], I['ptr'])
    ref_calls = nonfinite_calls(I, O)
    dev_calls = nonfinite_calls(I, Lib(), to=lambda t: t.to(dtype).to(dev))
    failures = []
    for name, call in dev_calls.items():
        try:  # every call is judged, also behind one that fails
            _check_call(I, name, call, ref_calls[name][0], dtype, dev)
        except AssertionError as exc:
            failures.append(f'{name}: {str(exc)[:300]}')
    assert not failures, f'H={H}: ' + ' || '.join(failures)


def _check_call(I, name, call, ref_fn, dtype, dev):
    H, S, cols, perm = I['H'], len(I['kinds']), I['cols'], I['perm']
    fn, src, go = call
    what = f'H={H} {dtype} {name}'
    shuffled = name == 'softmax_shuffled' or name.startswith('scatter')
    rows_index = I['index'][perm] if shuffled else I['index']
    per_row = name.startswith('softmax')
    out, grad = run_grad(fn, src, go, dev)
    ref, ref_grad = run_grad(ref_fn, src, go)
    # forward: the oracle on every column, the real reference's record on the kept ones
    assert_close(out, ref, what=what)
    assert_close(out[:, cols], I['results'][name]['out'], what=f'{what} (fixture)')
    big = large_mask(I, per_row, rows_index)
    exact = ref_fn(src.double())
    # (scatter 'mul' over +-3e38 overflows in float32 only: -inf there, checked above)
    big &= exact.isfinite() & ref.isfinite()
    assert_sum_close(out[big], ref[big], exact[big], what=f'{what} (1e4 / 3e38 vs fp64)')
    # backward
    check_backward(grad, ref_grad, rows_index, S, f'{what} gradient')
    check_backward(grad[:, cols], I['results'][name]['grad'], rows_index, S,
                   f'{what} gradient (fixture)')
    # isolation
    src_clean = clean_input(I, src if not shuffled else src[perm.argsort()])
    src_clean = src_clean[perm] if shuffled else src_clean
    out_c, grad_c = run_grad(fn, src_clean, go, dev)
    keep_o = ~special_mask(I, per_row, rows_index)
    keep_g = ~special_mask(I, True, rows_index)
    if name in BITWISE:
        assert torch.equal(out[keep_o], out_c[keep_o]), f'{what}: ordinary outputs moved'
        assert torch.equal(grad[keep_g], grad_c[keep_g]), f'{what}: ordinary gradients moved'
    else:
        assert_close(out[keep_o], out_c[keep_o], what=f'{what} isolation')
        assert_close(grad[keep_g], grad_c[keep_g], what=f'{what} gradient isolation')


TABLE = {  # id -> (call, values of the one column, ptr or index, expected)
    'lse [-inf, -inf]': ('lse', [-INF, -INF], [0, 2], [-INF]),
    'lse [-inf]': ('lse', [-INF], [0, 1], [-INF]),
    'lse [1, +inf]': ('lse', [1., INF], [0, 2], [INF]),
    'lse [1, nan]': ('lse', [1., NAN], [0, 2], [NAN]),
    'lse [-inf, nan]': ('lse', [-INF, NAN], [0, 2], [NAN]),
    'lse [+inf, -inf]': ('lse', [INF, -INF], [0, 2], [INF]),
    'softmax ptr [-inf, -inf]': ('softmax_ptr', [-INF, -INF], [0, 2], [0., 0.]),
    'softmax ptr [1, +inf]': ('softmax_ptr', [1., INF], [0, 2], [0., NAN]),
    'segment max': ('segment_max', [-INF, -INF, 1., INF], [0, 2, 4], [0., 0.]),
    'segment min': ('segment_min', [-INF, -INF, 1., INF], [0, 2, 4], [0., 1.]),
    # the index form keeps the index branch's answer for an all -inf group, scatter the plain
    # extremum
    'softmax index [-inf, -inf]': ('softmax_index', [-INF, -INF], [0, 0], [NAN, NAN]),
    'scatter max [-inf, -inf]': ('scatter_max', [-INF, -INF], [0, 0], [-INF]),
    'scatter max [1, +inf]': ('scatter_max', [1., INF], [0, 0], [INF]),
}


@pytest.mark.parametrize('case', list(TABLE))
def test_table_of_reference_answers(dev, case):
    """The five divergences predicted from the kernel source, one case each (the same values are
    asserted of the reference and the oracle in
    ``test_oracle_golden.test_nonfinite_table_of_the_reference``), plus segments with a NaN in
    segment_logsumexp, whose maximum ``fmaxf`` would drop."""
    from pytorch_geometric_amd import utils
    call, values, where, want = TABLE[case]
    src = torch.tensor(values, device=dev).view(-1, 1)
    where = torch.tensor(where, device=dev)
    n_groups = int(where.max()) + 1
    got = {'lse': lambda: utils.segment_logsumexp(src, where, 0),
           'softmax_ptr': lambda: utils.softmax(src, None, where),
           'segment_max': lambda: utils.segment(src, where, 'max'),
           'segment_min': lambda: utils.segment(src, where, 'min'),
           'softmax_index': lambda: utils.softmax(src, where, num_nodes=n_groups),
           'scatter_max': lambda: utils.scatter(src, where, 0, n_groups, 'max')}[call]()
    got, want = got.cpu().view(-1), torch.tensor(want)
    assert torch.equal(got.isnan(), want.isnan()) and \
        torch.equal(got.nan_to_num(nan=0.), want.nan_to_num(nan=0.)), (case, got, want)


def test_segment_extremum_gradient_follows_the_result_the_caller_sees(dev):
    """segment(..., 'max') returns 0 for a segment whose maximum is infinite; nothing of such a
    segment may receive a gradient (the reference's ``where(out.isinf(), 0, out)``), a NaN
    extremum sends the gradient to the NaN element."""
    from pytorch_geometric_amd import utils
    src = torch.tensor([[1., 2.], [INF, 0.], [NAN, 5.], [3., 4.], [-INF, -INF]])
    ptr = torch.tensor([0, 2, 4, 5])
    go = torch.tensor([[1., 2.], [-3., 4.], [5., 6.]])
    for r in ('max', 'min'):
        ref, ref_grad = run_grad(lambda s: O.segment(s, ptr, r), src, go)
        out, grad = run_grad(lambda s: utils.segment(s, ptr.to(dev), r), src, go, dev)
        assert_close(out, ref, rtol=0, atol=0, what=r)
        assert_close(grad, ref_grad, rtol=0, atol=0, what=f'{r} gradient')


# ---- fused GAT edge softmax ------------------------------------------------------------------------
def gat_case(H, seed, slope):
    """Destination rows = the segments of ``layout(H)``; every edge has a source node of its own,
    so ``alpha_src`` sets each logit; after the leaky ReLU the special column of a special
    destination holds that kind's values (negative finite ones are divided by the slope first)."""
    g = gen(seed)
    segs = NF.layout(H)
    kinds = [k for k, _ in segs]
    lens = torch.tensor([n for _, n in segs])
    S, n, c = len(segs), int(lens.sum()), NF.special_col(H)
    dst = torch.arange(S).repeat_interleave(lens)
    a_src = torch.randn(n, H, generator=g) * 2
    a_dst = torch.randn(S, H, generator=g)
    clean = a_src.clone()
    at = 0
    for i, (kind, ln) in enumerate(segs):
        if kind:
            v = torch.tensor(NF.special_values(kind, H))
            a_src[at:at + ln, c] = torch.where((v < 0) & v.isfinite(), v / slope, v)
            a_dst[i, c] = 0.
        at += ln
    order = torch.randperm(n, generator=g)  # edges in no particular order
    ei = torch.stack([torch.arange(n)[order], dst[order]])
    return kinds, ei, a_src, clean, a_dst, c


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('H', [1, 4, 8, 3])
def test_gat_edge_softmax_nonfinite(dev, H, dtype):
    """``GatEdgeSoftmaxFunction`` (logits + leaky ReLU + softmax per destination in one kernel)
    against the unfused composition on the CPU — the oracle's softmax in its INDEX form, which
    is what GATConv calls: an all -inf neighbourhood gives NaN, not 0."""
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd._functions import GatEdgeSoftmaxFunction
    slope = 0.2
    kinds, ei, a_src, a_src_clean, a_dst, c = gat_case(H, 900 + H, slope)
    S, n = len(kinds), a_src.size(0)
    go = torch.randn(n, H, generator=gen(H))
    graph = pga.EdgeIndex(ei.to(dtype).to(dev), (n, S))
    slot = graph.by_dst().perm.long().cpu()  # slot k of the by-destination order = edge slot[k]
    seg_of_src = torch.empty(n, dtype=torch.long)
    seg_of_src[ei[0]] = ei[1]

    def ref_fn(s, d):
        logit = torch.nn.functional.leaky_relu(s[ei[0]] + d[ei[1]], slope)
        return O.softmax(logit, ei[1], num_nodes=S)[slot]

    def dev_fn(s, d):
        return GatEdgeSoftmaxFunction.apply(s, d, graph, slope)

    def both(fn, s, d, device=None):
        s = s.clone().to(device or 'cpu').requires_grad_(True)
        d = d.clone().to(device or 'cpu').requires_grad_(True)
        out = fn(s, d)
        gs, gd = torch.autograd.grad(out, [s, d], go.to(out.device))
        return out.detach().cpu(), gs.cpu(), gd.cpu()

    ref, ref_gs, ref_gd = both(ref_fn, a_src, a_dst)
    out, gs, gd = both(dev_fn, a_src, a_dst, dev)
    what = f'GAT edge softmax H={H} {dtype}'
    assert_close(out, ref, what=what)
    i = kinds.index('neginf_2')
    rows = (ei[1][slot] == i).nonzero().view(-1)
    assert bool(ref[rows, c].isnan().all()) and bool(out[rows, c].isnan().all()), \
        'an all -inf neighbourhood is NaN in the index form'
    dst_slot = ei[1][slot]
    big = torch.zeros(n, H, dtype=torch.bool)
    big[:, c] = torch.tensor([k in NF.LARGE for k in kinds])[dst_slot]
    exact = ref_fn(a_src.double(), a_dst.double())
    assert_sum_close(out[big], ref[big], exact[big], what=f'{what} (1e4 / 3e38 vs fp64)')
    # gradients: alpha_src rows belong to the destination of their one edge; alpha_dst row i and
    # the alpha_src rows of destination i stand or fall together
    joint_ref = torch.cat([ref_gs, ref_gd])
    joint = torch.cat([gs, gd])
    joint_index = torch.cat([seg_of_src, torch.arange(S)])
    check_backward(joint, joint_ref, joint_index, S, f'{what} gradient')
    # isolation
    out_c, gs_c, gd_c = both(dev_fn, a_src_clean, a_dst, dev)
    special = torch.tensor([bool(k) for k in kinds])
    keep = torch.ones(n, H, dtype=torch.bool)
    keep[:, c] = ~special[dst_slot]
    assert torch.equal(out[keep], out_c[keep]), f'{what}: ordinary coefficients moved'
    keep_s = torch.ones(n, H, dtype=torch.bool)
    keep_s[:, c] = ~special[seg_of_src]
    assert_close(gs[keep_s], gs_c[keep_s], what=f'{what} alpha_src gradient isolation')
    keep_d = torch.ones(S, H, dtype=torch.bool)
    keep_d[:, c] = ~special
    assert_close(gd[keep_d], gd_c[keep_d], what=f'{what} alpha_dst gradient isolation')


# ---- SoftmaxAggregation and GATConv end to end -----------------------------------------------------
@pytest.mark.parametrize('use_ptr', [True, False])
def test_softmax_aggregation_with_a_masked_column(dev, fx, use_ptr):
    """``sum_i softmax_i(t x_i) x_i`` with -inf / +inf / NaN entries in one column: against the
    oracle's composition (the masked entries give ``-inf * 0 = NaN`` in the reference as well)."""
    from pytorch_geometric_amd import nn
    I = fx['H8']
    S = len(I['kinds'])
    x = NF.full(I['src'], 8, I['cols'], I['seed'])
    go = torch.randn(S, 8, generator=gen(3))
    where = dict(ptr=I['ptr']) if use_ptr else dict(index=I['index'], dim_size=S)
    aggr = nn.SoftmaxAggregation(t=0.5).to(dev)
    ref, ref_grad = run_grad(lambda s: O.softmax_aggregation(s, t=0.5, **where), x, go)
    out, grad = run_grad(lambda s: aggr(s, **{k: v.to(dev) if torch.is_tensor(v) else v
                                              for k, v in where.items()}), x, go, dev)
    what = f'SoftmaxAggregation ptr={use_ptr}'
    # (atol: the bound test_softmax_and_powermean_aggregation_golden holds this layer to)
    assert_close(out, ref, atol=2e-5, what=what)
    # The gradient holds x_i - out = 1e4 - 9999.73: both float32 evaluations cancel there with
    # an error of an ulp of 1e4 (1e-3) over 0.27, so on the 1e4 / 3e38 segments the kernel is
    # bounded by the reference's own float32 error against float64, elsewhere by 1e-5.
    big = large_mask(I, True)
    (exact, ) = torch.autograd.grad(O.softmax_aggregation(xd := x.double().requires_grad_(True),
                                                          t=0.5, **where), [xd], go.double())
    big &= exact.isfinite() & ref_grad.isfinite()
    assert_sum_close(grad[big], ref_grad[big], exact[big], what=f'{what} gradient vs fp64')
    check_backward(torch.where(big, ref_grad, grad), ref_grad, I['index'], S, f'{what} gradient')
    out_c, grad_c = run_grad(lambda s: aggr(s, **{k: v.to(dev) if torch.is_tensor(v) else v
                                                  for k, v in where.items()}),
                             clean_input(I, x), go, dev)
    keep_o, keep_g = ~special_mask(I, False), ~special_mask(I, True)
    assert_close(out[keep_o], out_c[keep_o], what=f'{what} isolation')
    assert_close(grad[keep_g], grad_c[keep_g], what=f'{what} gradient isolation')


@pytest.mark.parametrize('fuse_node', [True, False])
def test_gat_conv_with_masked_sources(dev, fuse_node):
    """GATConv end to end where head 1's logit of some source nodes is -inf (their projected
    feature times the attention vector overflows): those edges get coefficient exactly 0, every
    output and gradient stays finite and matches the oracle's unfused layer."""
    from pytorch_geometric_amd.nn import GATConv
    g = gen(17)
    n, e, fin, heads, C = 60, 400, 6, 4, 5
    x = torch.randn(n, fin, generator=g)
    x[:, 0] = 0.
    masked = torch.arange(n) % 7 == 3
    x[masked, 0] = 1e10
    ei = torch.randint(1, n, (2, e), generator=g)
    ei = torch.cat([ei, torch.stack([torch.zeros(n - 1, dtype=torch.long),
                                     torch.arange(1, n)])], 1)  # node 0 (unmasked) reaches all
    torch.manual_seed(5)
    conv = GATConv(fin, C, heads=heads)
    with torch.no_grad():
        conv.lin.weight[:, 0] = 0.
        conv.lin.weight[1 * C, :] = 0.
        conv.lin.weight[1 * C, 0] = 1.      # x'[:, head 1, 0] = x[:, 0]
        conv.att_src[0, 1, 0] = -1e30       # 1e10 * -1e30 overflows: a_src[masked, 1] = -inf
        conv.att_dst[0, 1, 0] = 0.
    st = {k: v.detach().clone() for k, v in conv.state_dict().items()}
    names = ['lin.weight', 'att_src', 'att_dst', 'bias']
    leaves = [st[k].clone().requires_grad_(True) for k in names]
    xr = x.clone().requires_grad_(True)
    ref, ref_ei, ref_alpha = O.gat_conv(xr, ei, leaves[0], leaves[1], leaves[2], leaves[3], heads,
                                        C, return_alpha=True)
    go = torch.randn(n, heads * C, generator=g)
    ref_grads = torch.autograd.grad(ref, [xr] + leaves, go)
    src_masked = masked[ref_ei[0]]
    assert bool((ref_alpha[src_masked, 1] == 0).all()) and bool(ref.isfinite().all())
    assert all(bool(t.isfinite().all()) for t in ref_grads)

    conv = conv.to(dev)
    xx = x.to(dev).requires_grad_(True)
    if fuse_node:
        out = conv(xx, ei.to(dev))
    else:
        out, (got_ei, alpha) = conv(xx, ei.to(dev), return_attention_weights=True)
        assert torch.equal(got_ei.cpu(), ref_ei)
        assert_close(alpha, ref_alpha, what='attention weights')
        assert bool((alpha.cpu()[src_masked, 1] == 0).all())
    out.backward(go.to(dev))
    assert_close(out, ref, what='GATConv out')
    # (the gradients that pass through att_src[0, 1, 0] = -1e30 are ~1e29: judged on their own)
    assert_close_scaled(xx.grad[:, 1:], ref_grads[0][:, 1:], what='GATConv grad x')
    assert_close_scaled(xx.grad[:, 0], ref_grads[0][:, 0], what='GATConv grad x[:, 0]')
    params = dict(conv.named_parameters())
    for k, want in zip(names, ref_grads[1:]):
        got = params[k].grad
        if k == 'lin.weight':
            rest = torch.arange(heads * C) != C
            assert_close_scaled(got[C], want[C], what='GATConv grad lin.weight, masking row')
            got, want = got[rest.to(dev)], want[rest]
        assert_close_scaled(got, want, what=f'GATConv grad {k}')


# ---- one-pass cross entropy ------------------------------------------------------------------------
def ce_case(C, seed):
    g = gen(seed)
    B = 14
    logits = torch.randn(B, C, generator=g) * 3
    y = torch.randint(0, C, (B, ), generator=g)
    kinds = [''] * B

    def put(r, kind):
        kinds[r] = kind
        t = int(y[r])
        o = (t + 1) % C
        if kind == 'masked':          # -inf on non-target classes
            logits[r, torch.arange(C) % 2 == (t + 1) % 2] = -INF
        elif kind == 'only_target':   # -inf everywhere but the target
            logits[r] = -INF
            logits[r, t] = 0.75
        elif kind == 'big_pos':
            logits[r, t], logits[r, o] = 1e4 - 1, 1e4
        elif kind == 'big_neg':
            logits[r] = -1e4 - logits[r].abs()
        elif kind == 'target_neginf':
            logits[r, t] = -INF
        elif kind == 'posinf':
            logits[r, o] = INF
        elif kind == 'nan':
            logits[r, o] = NAN
        elif kind == 'below_16':      # the last maximum that still subtracts max + log(sum) ...
            logits[r, o] = 16 - 2.0 ** -20
        elif kind == 'at_16':         # ... and the first that subtracts the maximum alone
            logits[r, o] = 16.

    # rows 0..3 / 4..7 / 8..11 / 12..13 share a wave each: special rows next to ordinary ones
    for r, kind in ((1, 'masked'), (2, 'big_pos'), (4, 'target_neginf'), (6, 'only_target'),
                    (7, 'big_neg'), (9, 'posinf'), (10, 'nan'), (13, 'masked'),
                    (3, 'below_16'), (11, 'at_16')):
        put(r, kind)
    return logits, y, kinds


@pytest.mark.parametrize('C', [3, 172, 700])
def test_cross_entropy_nonfinite(dev, C):
    """``nn.functional.cross_entropy(out, y, index)`` and the raw ``pygamd_cross_entropy_step``
    rows against ``F.cross_entropy`` and its autograd: -inf masks, +-1e4 rows, a -inf target
    (loss +inf, finite gradient), +inf and NaN rows, and a row on either side of the maximum (16)
    from which the kernel subtracts the maximum alone.  C = 3 / 172 take the register route, 700
    the loop route."""
    import torch.nn.functional as F
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn.functional import cross_entropy
    logits, y, kinds = ce_case(C, 40 + C)
    B = logits.size(0)
    finite_rows = [r for r, k in enumerate(kinds) if k not in ('target_neginf', 'posinf', 'nan')]
    subsets = {'finite': finite_rows, 'inf_loss': finite_rows + [kinds.index('target_neginf')],
               'posinf': finite_rows + [kinds.index('posinf')],
               'nan': finite_rows + [kinds.index('nan')], 'all': list(range(B))}
    for name, rows in subsets.items():
        index = torch.tensor(rows)
        xr = logits.clone().requires_grad_(True)
        ref = F.cross_entropy(xr[index], y[index])
        (ref_grad, ) = torch.autograd.grad(ref, [xr])
        xx = logits.to(dev).requires_grad_(True)
        loss = cross_entropy(xx, y.to(dev), index.to(dev))
        (grad, ) = torch.autograd.grad(loss, [xx])
        what = f'cross entropy C={C} rows={name}'
        print(f'{what}: loss {float(loss)} reference {float(ref)}')
        assert bool(loss.isfinite()) == bool(ref.isfinite()), f'{what}: {float(loss)} vs {float(ref)}'
        assert_close(loss, ref, what=f'{what} loss')
        if ref.isfinite():
            ex = F.cross_entropy(logits.double()[index], y[index])
            assert_sum_close(loss.view(1), ref.view(1), ex.view(1), what=f'{what} loss vs fp64')
        check_backward(grad, ref_grad, torch.arange(B), B, f'{what} gradient')
        assert bool(grad.cpu()[finite_rows].isfinite().all())
        # the kernel's own rows (d loss / d logits[index]) and loss
        k_loss, k_grad = _native.cross_entropy_rows(logits.to(dev), y.to(dev), index.to(dev))
        assert bool(k_loss.isfinite()) == bool(ref.isfinite())
        assert_close(k_loss, ref, what=f'{what} kernel loss')
        check_backward(k_grad, ref_grad[index], torch.arange(len(rows)), len(rows),
                       f'{what} kernel gradient')
    # a -inf target: the loss is +inf, the gradient the ordinary softmax minus one-hot
    r = kinds.index('target_neginf')
    index = torch.tensor([r])
    k_loss, k_grad = _native.cross_entropy_rows(logits.to(dev), y.to(dev), index.to(dev))
    assert float(k_loss) == INF
    want = torch.softmax(logits[r].double(), 0)
    want[y[r]] -= 1
    assert_close(k_grad.view(-1), want.float(), what='gradient of the -inf-target row')


# ---- unsorted scatter on both sides of the sorted-route threshold ----------------------------------
@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
def test_large_scatter_nonfinite_takes_the_sorted_route(dev, fx, dtype):
    """The fixture's rows inside an index large enough for the sorted route (a cached radix sort +
    a segment reduction; ``test_large_unsorted_scatter_takes_the_sorted_route``): NaN propagates
    as in ``amax`` / ``amin``, signed infinities are kept, the neighbours are untouched.  The
    small side of the threshold (float atomics) is
    ``test_calls_match_the_reference_and_isolate_special_values``."""
    from pytorch_geometric_amd import _functions
    from pytorch_geometric_amd.utils import scatter
    I = fx['H64']
    H, S, perm = 64, len(I['kinds']), I['perm']
    g = gen(91)
    extra, groups = 140_000, 3000
    src = torch.cat([NF.full(I['src'], H, I['cols'], I['seed'])[perm],
                     torch.randn(extra, H, generator=g)])
    index = torch.cat([I['index'][perm], torch.randint(S, S + groups, (extra, ), generator=g)])
    N = S + groups
    go = torch.randn(N, H, generator=g)
    d_index = index.to(dtype).to(dev)
    _functions._scatter_plans.clear()
    _functions._scatter_seen.clear()
    assert _functions._use_sorted_scatter(src, d_index, 'max')
    scatter(src.to(dev), d_index, 0, N, 'sum')  # first sighting: atomics; sorted from now on
    clean = src.clone()
    clean[:perm.numel(), I['col']] = I['clean_col'][perm]
    keep_o = torch.ones(N, H, dtype=torch.bool)
    keep_o[:S] = ~special_mask(I, False)
    keep_g = torch.ones(src.size(0), H, dtype=torch.bool)
    keep_g[:perm.numel()] = ~special_mask(I, True, I['index'][perm])
    for r in ('sum', 'mean', 'min', 'max'):
        what = f'sorted-route scatter {r} {dtype}'
        ref, ref_grad = run_grad(lambda s: O.scatter(s, index, 0, N, r), src, go)
        out, grad = run_grad(lambda s: scatter(s, d_index, 0, N, r), src, go, dev)
        assert len(_functions._scatter_plans) == 1, 'the sorted route was not taken'
        assert_close(out[:S], ref[:S], what=what)
        ex = O.scatter(src.double(), index, 0, N, r)
        fin = ref.isfinite() & ex.isfinite()
        assert torch.equal(out.isfinite(), ref.isfinite()), what
        assert_sum_close(out[fin], ref[fin], ex[fin], what=f'{what} vs fp64')
        check_backward(grad, ref_grad, index, N, f'{what} gradient')
        out_c, grad_c = run_grad(lambda s: scatter(s, d_index, 0, N, r), clean, go, dev)
        if r in ('min', 'max'):
            assert torch.equal(out[keep_o], out_c[keep_o]), f'{what}: ordinary outputs moved'
            assert torch.equal(grad[keep_g], grad_c[keep_g]), f'{what}: ordinary gradients moved'
        else:
            assert_close(out[keep_o], out_c[keep_o], what=f'{what} isolation')
            assert_close(grad[keep_g], grad_c[keep_g], what=f'{what} gradient isolation')
