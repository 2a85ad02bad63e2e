"""TopKPooling / SAGPooling on the GPU (csrc/pool.hip): the select kernel bit-exact against the
reference's ``topk`` on the CPU copy and against the plain-Python tie rule, the edge filter
bit-exact against the reference's ``filter_adj``, the gather-scale forward bit-exact against the
torch expression and its backward against float64, and every golden layer case on both routes."""
import pytest
import torch

from tests import _pool_ref as R
from tests._norm_ref import scaled_err, tol_of
from tests._util import _call_counts, assert_close_scaled

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BASE_SIZES = [1, 2, 3, 63, 64, 65, 0, 70, 5]
RATIOS = [0.5, 0.7, 1e-9, 1, 3, 100]
_REF = {}


def reference():
    """the real reference's ``topk`` and ``filter_adj`` (the staged copy), imported once"""
    if not _REF:
        from oracle import make_ref
        make_ref.import_reference()
        from torch_geometric.nn.pool.connect.filter_edges import filter_adj
        from torch_geometric.nn.pool.select.topk import topk
        _REF.update(topk=topk, filter_adj=filter_adj)
    return _REF


def threshold_sizes():
    from pytorch_geometric_amd import _native
    sizes = list(BASE_SIZES)
    for t in (_native.TOPK_WAVE_NODES, 256, _native.TOPK_MAX_NODES):   # 256: one key per thread
        sizes += [t - 1, t, t + 1]
    return sizes


def tie_free_scores(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).float() / n


# ---- select ------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
def test_select_matches_the_reference(dtype, monkeypatch):
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn import topk
    sizes = [s for s in threshold_sizes() if s <= _native.TOPK_MAX_NODES]
    batch = R.batch_of(sizes)
    score = tie_free_scores(batch.numel(), 1)
    sd, bd = score.to(DEV), batch.to(device=DEV, dtype=dtype)
    for ratio in RATIOS:
        want = reference()['topk'](score, ratio, batch)
        calls = _call_counts(monkeypatch, lambda: topk(sd, ratio, bd, fuse=True))
        assert calls.get('pygamd_topk_select') == 1, calls
        got = topk(sd, ratio, bd, fuse=True)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), ratio
        assert torch.equal(topk(sd, ratio, bd, fuse=False).cpu(), want), ratio
        ptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), device=DEV, dtype=dtype)
        from pytorch_geometric_amd.nn.pool.select.topk import num_selected
        k = num_selected(ratio, ptr[1:] - ptr[:-1], torch.float32)
        out_ptr = torch.zeros(len(sizes) + 1, dtype=torch.long, device=DEV)
        out_ptr[1:] = torch.minimum(k, (ptr[1:] - ptr[:-1]).long()).cumsum(0)
        perm, weight = _native.topk_select(sd, ptr, k, out_ptr, int(out_ptr[-1]), max(sizes))
        assert torch.equal(perm.cpu(), want) and torch.equal(weight.cpu(), score[want])


def test_select_past_the_envelope_takes_the_generic_route(monkeypatch):
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn import topk
    sizes = [5, _native.TOPK_MAX_NODES + 1, 64]
    batch = R.batch_of(sizes)
    score = tie_free_scores(batch.numel(), 2)
    sd, bd = score.to(DEV), batch.to(DEV)
    for ratio in (0.5, 3):
        calls = _call_counts(monkeypatch, lambda: topk(sd, ratio, bd, fuse=True))
        assert 'pygamd_topk_select' not in calls
        assert torch.equal(topk(sd, ratio, bd, fuse=True).cpu(),
                           reference()['topk'](score, ratio, batch))


def test_select_without_a_batch_vector_and_unsorted():
    from pytorch_geometric_amd.nn import topk
    for n in (1, 64, 65, 700):
        score = tie_free_scores(n, n)
        for ratio in RATIOS:
            want = reference()['topk'](score, ratio, torch.zeros(n, dtype=torch.long))
            assert torch.equal(topk(score.to(DEV), ratio, None, fuse=True).cpu(), want)
    U = R.load_golden()['unsorted']
    for ratio, want in U['perm'].items():
        got = topk(U['score'].to(DEV), ratio, U['batch'].to(DEV), fuse=True)
        assert torch.equal(got.cpu(), want)


def test_select_tie_rule():
    from pytorch_geometric_amd.nn import topk
    sizes = threshold_sizes()[:-1]       # (without the graph past the envelope)
    batch = R.batch_of(sizes).to(DEV)
    n = batch.numel()
    g = torch.Generator().manual_seed(3)
    inf, nan = float('inf'), float('nan')
    scores = {'equal': torch.full((n, ), 0.25),
              'zeros': torch.where(torch.rand(n, generator=g) < 0.5, 0.0, -0.0),
              'inf': torch.tensor([inf, -inf, 1.0, 0.0, -0.0])[torch.randint(0, 5, (n, ),
                                                                             generator=g)]}
    for where in ('first', 'last', 'middle'):
        s = torch.randn(n, generator=g)
        start = 0
        for size in sizes:
            if size > 0:
                s[start + {'first': 0, 'last': size - 1, 'middle': size // 2}[where]] = nan
            start += size
        s[140], s[141] = nan, -nan
        scores['nan ' + where] = s
    for what, s in scores.items():
        for ratio in (0.5, 3, 100):
            want = R.topk_ref(s.tolist(), sizes, ratio)
            assert topk(s.to(DEV), ratio, batch, fuse=True).tolist() == want, (what, ratio)
            assert topk(s.to(DEV), ratio, batch, fuse=False).tolist() == want, (what, ratio)


# ---- edge filter -------------------------------------------------------------------------------
def _edges(E, n, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, E), generator=g)
    if E >= 8:
        ei[1, :E // 8] = ei[0, :E // 8]                       # self loops
        ei[:, E // 4:E // 4 + E // 8] = ei[:, :E // 8]        # duplicates
    return ei.to(dtype)


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
def test_filter_edges_matches_the_reference(dtype):
    from pytorch_geometric_amd.nn import filter_adj
    n = 97
    g = torch.Generator().manual_seed(7)
    keeps = {'none': torch.empty(0, dtype=torch.long), 'all': torch.randperm(n, generator=g),
             'half': torch.randperm(n, generator=g)[:n // 2]}
    for E in (0, 1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5):
        ei = _edges(E, n, E, dtype)
        for what, perm in keeps.items():
            want, _ = reference()['filter_adj'](ei.long(), None, perm, num_nodes=n)
            got, _ = filter_adj(ei.to(DEV), None, perm.to(DEV), num_nodes=n, fuse=True)
            assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), (E, what)
            slow, _ = filter_adj(ei.to(DEV), None, perm.to(DEV), num_nodes=n, fuse=False)
            assert torch.equal(slow.cpu(), want), (E, what)


def test_filter_edges_strided_inputs_and_edge_attr(monkeypatch):
    from pytorch_geometric_amd.nn import filter_adj
    n, E = 50, 4097
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:30]
    ei = _edges(E, n, 5, torch.int64)
    want, _ = reference()['filter_adj'](ei, None, perm, num_nodes=n)
    transposed = ei.t().contiguous().to(DEV).t()              # a transposed [E, 2]
    wide = torch.zeros(2, 3 * E, dtype=torch.long)
    wide[:, ::3] = ei
    sliced = wide.to(DEV)[:, ::3]                             # a column slice of a wider tensor
    for view in (transposed, sliced):
        assert not view.is_contiguous()
        calls = _call_counts(monkeypatch,
                             lambda: filter_adj(view, None, perm.to(DEV), num_nodes=n, fuse=True))
        assert calls.get('pygamd_filter_edges') == 1, calls
        got, _ = filter_adj(view, None, perm.to(DEV), num_nodes=n, fuse=True)
        assert torch.equal(got.cpu(), want)
    for shape in ((E, ), (E, 3)):
        attr = torch.randn(shape, generator=torch.Generator().manual_seed(2))
        a_ref = attr.clone().requires_grad_(True)
        _, want_attr = reference()['filter_adj'](ei, a_ref, perm, num_nodes=n)
        go = torch.randn(want_attr.shape, generator=torch.Generator().manual_seed(3))
        want_attr.backward(go)
        a = attr.to(DEV).requires_grad_(True)
        got, got_attr = filter_adj(ei.to(DEV), a, perm.to(DEV), num_nodes=n, fuse=True)
        got_attr.backward(go.to(DEV))
        assert torch.equal(got.cpu(), want) and torch.equal(got_attr.cpu(), want_attr.detach())
        assert torch.equal(a.grad.cpu(), a_ref.grad)          # (no edge twice: plain copies)


# ---- gather-scale ------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [1, 3, 64, 65, 256, 513])
def test_gather_scale(F):
    from pytorch_geometric_amd._functions import GatherScaleFunction
    N = 150
    g = torch.Generator().manual_seed(F)
    x0 = torch.randn(N, F, generator=g)
    s0 = torch.randn(N, generator=g)
    for M in (0, 1, N):
        for mult in (1.0, 2.5):
            perm = torch.randperm(N, generator=g)[:M]
            go = torch.randn(M, F, generator=g)
            gw = torch.randn(M, generator=g)

            def torch_expr(dtype, device):
                x = x0.to(device=device, dtype=dtype).requires_grad_(True)
                s = s0.to(device=device, dtype=dtype).requires_grad_(True)
                w = s[perm.to(device)]
                out = x[perm.to(device)] * w.view(-1, 1)
                out = mult * out if mult != 1 else out
                (out * go.to(device=device, dtype=dtype)).sum().add(
                    (w * gw.to(device=device, dtype=dtype)).sum()).backward()
                return out.detach(), w.detach(), x.grad, s.grad

            o32, w32, gx32, gs32 = torch_expr(torch.float32, DEV)
            _, _, gx64, gs64 = torch_expr(torch.float64, 'cpu')
            x = x0.to(DEV).requires_grad_(True)
            s = s0.to(DEV).requires_grad_(True)
            out, w = GatherScaleFunction.apply(x, s, perm.to(DEV), mult)
            assert torch.equal(out, o32) and torch.equal(w, w32), (M, mult)   # bit-exact
            ((out * go.to(DEV)).sum() + (w * gw.to(DEV)).sum()).backward()
            for name, got, r32, r64 in (('grad_x', x.grad, gx32, gx64),
                                        ('grad_score', s.grad, gs32, gs64)):
                tol = tol_of(scaled_err(r32, r64))
                print(f'F {F} M {M} mult {mult} {name}: err {scaled_err(got, r64):.2e} '
                      f'tol {tol:.2e}')
                assert_close_scaled(got.double(), r64, tol=tol, what=f'{name} F={F} M={M}')
            dropped = torch.ones(N, dtype=torch.bool)
            dropped[perm] = False
            assert not x.grad.cpu()[dropped].any() and not s.grad.cpu()[dropped].any()


def test_gather_scale_strided_x():
    from pytorch_geometric_amd import _native
    g = torch.Generator().manual_seed(9)
    wide = torch.randn(40, 100, generator=g).to(DEV)
    s = torch.randn(40, generator=g).to(DEV)
    perm = torch.randperm(40, generator=g)[:17].to(DEV)
    x = wide[:, 10:75]
    out, w = _native.gather_scale_forward(x, s, perm, 2.0)
    assert torch.equal(out, 2.0 * (x[perm] * s[perm].view(-1, 1))) and torch.equal(w, s[perm])


# ---- layers ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.load_golden()['cases']))
def test_golden_case_fused_and_generic(name):
    _, fused = R.check_golden_case(name, DEV, True)
    _, slow = R.run_golden_case(name, DEV, False)
    assert torch.equal(fused['perm'], slow['perm'])
    assert torch.equal(fused['edge_index'], slow['edge_index'])


def test_golden_case_int32_batch():
    R.check_golden_case('topk_ratio_0.7_attr_E', DEV, True, index_dtype=torch.int32)


def test_fused_layer_calls_and_cached_handle(monkeypatch):
    import pytorch_geometric_amd.nn as nn
    from pytorch_geometric_amd import _norm
    G = R.load_golden()
    layer = nn.TopKPooling(G['meta']['F'], ratio=0.5).to(DEV)
    layer.fuse = True
    x, ei, batch = G['x'].to(DEV), G['edge_index'].to(DEV), G['batch'].to(DEV)
    calls = _call_counts(monkeypatch, lambda: layer(x, ei, None, batch))
    for fn in ('pygamd_topk_select', 'pygamd_gather_scale_forward', 'pygamd_filter_edges'):
        assert calls.get(fn) == 1, calls
    handle = _norm.batch_handle(batch, None)
    again = _call_counts(monkeypatch, lambda: layer(x, ei, None, batch))
    assert 'pygamd_index2ptr' not in again and _norm.batch_handle(batch, None) is handle
    layer.fuse = False
    off = _call_counts(monkeypatch, lambda: layer(x, ei, None, batch))
    assert not any(fn.startswith(('pygamd_topk', 'pygamd_gather_scale', 'pygamd_filter'))
                   for fn in off), off
