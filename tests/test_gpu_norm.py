"""GraphNorm and LayerNorm(mode='graph') on the device (csrc/graph_norm.hip): the golden cases
with their C-ABI call counts, the shapes at which the kernels change path, exact results on dyadic
data, independence of a graph from the rest of its batch, bitwise repeatability, 64-bit row
offsets, the memory promise, half inputs, torch.compile and the pools.  Every comparison is
against float64 (the golden or the restatement of tests/_norm_ref.py run on the device) with
``assert_close_scaled`` at ``max(2e-5, 2 x the reference arithmetic's own float32 error)``."""
import pytest
import torch

import pytorch_geometric_amd.nn as nn
import pytorch_geometric_amd.ops  # noqa: F401 (registers torch.ops.pyg_amd.*)
from pytorch_geometric_amd import _native, _norm
from tests import _norm_ref as R
from tests import _util as T

pytestmark = pytest.mark.gpu

FWD, BWD = 'pygamd_graph_norm_forward', 'pygamd_graph_norm_backward'
CASES = sorted(R.load_golden()['cases'])
TH, CH = _native.GRAPH_NORM_THRESHOLD, _native.GRAPH_NORM_CHUNK


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows_calls(calls):
    return [n for n in calls if 'scatter' in n or 'gather' in n or 'spmm' in n]


def _layers(F, dev, seed=0, **kw):
    """a GraphNorm and a LayerNorm with non-trivial parameters"""
    g = gen(seed)
    out = []
    for layer in (nn.GraphNorm(F), nn.LayerNorm(F, **kw)):
        with torch.no_grad():
            for p in layer.parameters():
                p.add_(0.3 * torch.randn(p.shape, generator=g))
        out.append(layer.to(dev))
    return out


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', CASES)
def test_golden_cases_on_the_device(dev, monkeypatch, name, index_dtype):
    """one forward and one backward graph-norm call per layer call and no scatter or gather on the
    fused route; node mode is ``F.layer_norm``"""
    c = T._counted(monkeypatch, lambda: R.check_golden_case(name, dev, index_dtype))
    if name == 'layer_norm_node':
        assert FWD not in c.calls and BWD not in c.calls, c.calls
    else:
        assert c.calls.get(FWD) == 1 and c.calls.get(BWD) == 1, c.calls
        assert not _rows_calls(c.calls), c.calls


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('norm', ['graph_norm', 'layer_norm'])
def test_golden_models_on_the_device(dev, monkeypatch, norm, index_dtype):
    c = T._counted(monkeypatch, lambda: R.check_golden_model(norm, dev, index_dtype))
    assert c.calls.get(FWD) == 1 and c.calls.get(BWD) == 1, c.calls


def test_generic_cases_make_no_graph_norm_call(dev, monkeypatch):
    """``fuse=False``, an unsorted batch vector and F = 513 take the reference's scatters"""
    c = T._counted(monkeypatch, lambda: R.check_golden_case('graph_norm_offset', dev, fuse=False))
    assert FWD not in c.calls and BWD not in c.calls and _rows_calls(c.calls), c.calls
    c = T._counted(monkeypatch, lambda: R.check_golden_case('layer_norm_offset', dev, fuse=False))
    assert FWD not in c.calls and BWD not in c.calls and _rows_calls(c.calls), c.calls

    sizes = [5, 9, 1, 20]
    perm = torch.randperm(35, generator=gen(1))
    for F, shuffle in ((12, True), (513, False)):
        x = torch.randn(35, F, generator=gen(2))
        go = torch.randn(35, F, generator=gen(3))
        batch = R.batch_of(sizes)
        for layer, kind in zip(_layers(F, dev), ('graph_norm', 'layer_norm')):
            state = {}

            def step():
                xb = (x[perm] if shuffle else x).to(dev).requires_grad_(True)
                bb = (batch[perm] if shuffle else batch).to(dev)
                out = layer(xb, bb)
                out.backward((go[perm] if shuffle else go).to(dev))
                state.update(out=out, gx=xb.grad)

            c = T._counted(monkeypatch, step)
            assert FWD not in c.calls and BWD not in c.calls, c.calls
            params = {n: p.detach().double() for n, p in layer.named_parameters()}
            want, gx, _ = R.restate_with_grads(kind, x.to(dev), sizes, go.to(dev), params,
                                               torch.float64)
            inv = torch.argsort(perm).to(dev) if shuffle else slice(None)
            T.assert_close_scaled(state['out'][inv].double(), want, what=f'{kind} F={F} out')
            T.assert_close_scaled(state['gx'][inv].double(), gx, what=f'{kind} F={F} grad_x')


# ---- shapes at which the kernels can go wrong ------------------------------------------------------
@pytest.mark.parametrize('F', [1, 3, 20, 64, 256, 512])
def test_widths_and_graph_sizes_across_the_threshold(dev, monkeypatch, F):
    """every lane shape (scalar and float4, one to eight registers per lane) on graphs of 1 node, on
    both sides of a wave's 64 rows and of the plan's threshold, and of three chunks; the threshold
    and the chunk are the ones a plan of this kernel carries"""
    carried = _native.graph_norm_plan(R.ptr_of([1], dev))
    threshold, chunk = carried.threshold, carried.chunk
    SIZES = [1, 2, 63, 64, 65, threshold, threshold + 1, 2 * chunk + 1]
    plan = _native.graph_norm_plan(R.ptr_of(SIZES, dev))
    assert (plan.threshold, plan.chunk) == (threshold, chunk)
    assert plan.n_hub == sum(n > plan.threshold for n in SIZES) == 2
    assert plan.n_chunks == sum(-(-n // plan.chunk) for n in SIZES if n > plan.threshold)
    N = sum(SIZES)
    x = (torch.randn(N, F, generator=gen(F)) * 2 + 5).to(dev)
    go = torch.randn(N, F, generator=gen(F + 1)).to(dev)
    batch = R.batch_of(SIZES, dev)
    for layer, kind in zip(_layers(F, dev, seed=F), ('graph_norm', 'layer_norm')):
        c = T._counted(monkeypatch, lambda: R.check_against_restatement(
            layer, kind, x, SIZES, batch, go, f'{kind} F={F}'))
        assert c.calls.get(FWD) == 1 and c.calls.get(BWD) == 1, c.calls


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
def test_one_hub_graph_and_no_batch_vector(dev, index_dtype):
    """a batch that is ONE long graph, with a batch vector and without: the chunks, the merge and
    the apply launches alone; LayerNorm's two formulas differ as the reference's do"""
    n, F = 5 * CH + 7, 40
    assert n > TH
    x = (torch.randn(n, F, generator=gen(1)) + 30).to(dev)
    go = torch.randn(n, F, generator=gen(2)).to(dev)
    batch = torch.zeros(n, dtype=index_dtype, device=dev)
    gn, ln = _layers(F, dev, seed=4)
    R.check_against_restatement(gn, 'graph_norm', x, [n], batch, go, 'one hub, batch')
    R.check_against_restatement(gn, 'graph_norm', x, [n], None, go, 'one hub, no batch')
    R.check_against_restatement(ln, 'layer_norm', x, [n], batch, go, 'one hub, batch')
    ln.eps = 0.5   # (the two formulas differ visibly)
    x = x - 30
    R.check_against_restatement(ln, 'layer_norm', x, [n], None, go, 'one hub, no batch',
                                no_batch=True)
    R.check_against_restatement(ln, 'layer_norm', x, [n], batch, go, 'one hub, batch, eps 0.5')
    assert float((ln(x) - ln(x, batch)).detach().abs().max()) > 1e-2
    small = x[:50].contiguous()    # and under the threshold: one wave
    R.check_against_restatement(ln, 'layer_norm', small, [50], None, go[:50].contiguous(),
                                'one small graph, no batch', no_batch=True)


def test_empty_graphs_first_in_the_middle_and_last(dev):
    sizes = [0, 0, 7, 0, TH + 5, 0, 3, 0, 0]
    N, F = sum(sizes), 24
    x = torch.randn(N, F, generator=gen(5)).to(dev)
    go = torch.randn(N, F, generator=gen(6)).to(dev)
    batch = R.batch_of(sizes, dev)
    for layer, kind in zip(_layers(F, dev, seed=6), ('graph_norm', 'layer_norm')):
        R.check_against_restatement(layer, kind, x, sizes, batch, go, f'{kind}, empty graphs',
                                    batch_size=len(sizes))
        # batch_size read from the batch vector: the trailing empty graphs are not there
        R.check_against_restatement(layer, kind, x, sizes, batch, go, f'{kind}, batch_size=None')
    none = torch.empty(0, F, device=dev, requires_grad=True)
    out = nn.GraphNorm(F).to(dev)(none, torch.empty(0, dtype=torch.int64, device=dev), 3)
    out.sum().backward()
    assert out.shape == (0, F)


@pytest.mark.parametrize('F', [20, 64])
def test_a_column_slice_is_read_in_place(dev, monkeypatch, F):
    """``wide[:, 5:5 + F]``: a row pitch beyond F and a base that is not 16-byte aligned"""
    sizes = [3, 70, TH + 2]
    N = sum(sizes)
    wide = torch.randn(N, F + 11, generator=gen(7)).to(dev)
    go = torch.randn(N, F, generator=gen(8)).to(dev)
    batch = R.batch_of(sizes, dev)
    for layer, kind in zip(_layers(F, dev, seed=8), ('graph_norm', 'layer_norm')):
        leaf = wide.clone().requires_grad_(True)
        c = T._counted(monkeypatch,
                       lambda: layer(leaf[:, 5:5 + F], batch).backward(go))
        assert c.calls.get(FWD) == 1 and c.calls.get(BWD) == 1, c.calls
        assert not [n for n in c.calls if 'copy' in n], c.calls
        params = {n: p.detach() for n, p in layer.named_parameters()}
        out64, gx64, _ = R.restate_with_grads(kind, wide[:, 5:5 + F], sizes, go, params,
                                              torch.float64)
        T.assert_close_scaled(layer(wide[:, 5:5 + F], batch).double(), out64, what=f'{kind} out')
        T.assert_close_scaled(leaf.grad[:, 5:5 + F].double(), gx64, what=f'{kind} grad_x')
        assert float(leaf.grad[:, :5].abs().max()) == 0 == float(leaf.grad[:, 5 + F:].abs().max())


# ---- exact results ---------------------------------------------------------------------------------
def test_equal_rows_give_exactly_the_bias_and_no_gradient(dev):
    """dyadic data (multiples of 1/8: every sum is exact).  A graph whose rows are all equal has
    u = 0 under GraphNorm with mean_scale = 1, so y is exactly the bias; under LayerNorm when its
    columns are equal too.  With grad_y constant over the graph grad_x is exactly 0."""
    F = 24
    sizes = [1, 5, 64, 100, TH + 40]
    batch = R.batch_of(sizes, dev)
    row = (torch.randint(-40, 40, (len(sizes), F), generator=gen(9)).float() / 8)
    bias = (torch.randint(-16, 16, (F, ), generator=gen(10)).float() / 8).to(dev)
    weight = (torch.randint(1, 16, (F, ), generator=gen(11)).float() / 8).to(dev)
    gn = nn.GraphNorm(F).to(dev)
    ln = nn.LayerNorm(F).to(dev)
    with torch.no_grad():
        gn.bias.copy_(bias)
        gn.weight.copy_(weight)
        ln.bias.copy_(bias)
    x = row[batch.cpu()].to(dev).requires_grad_(True)
    out = gn(x, batch)
    assert torch.equal(out, bias.expand_as(out))
    out.backward(torch.full_like(out, 0.375))
    assert float(x.grad.abs().max()) == 0.0
    flat = row[:, :1].expand(-1, F)[batch.cpu()].contiguous().to(dev).requires_grad_(True)
    out = ln(flat, batch)
    assert torch.equal(out, bias.expand_as(out))
    out.backward(torch.full_like(out, 0.375))
    assert float(flat.grad.abs().max()) == 0.0


def test_a_graph_does_not_depend_on_the_rest_of_its_batch(dev):
    """bit for bit: a small graph and a hub graph alone and inside a larger batch"""
    F = 36
    sizes = [9, 41, 2 * CH + TH + 3, 17]
    x = (torch.randn(sum(sizes), F, generator=gen(12)) + 3).to(dev)
    go = torch.randn(sum(sizes), F, generator=gen(13)).to(dev)
    batch = R.batch_of(sizes, dev)
    for layer in _layers(F, dev, seed=13):
        xx = x.clone().requires_grad_(True)
        out = layer(xx, batch)
        out.backward(go)
        for g in (1, 2):
            lo = sum(sizes[:g])
            alone = x[lo:lo + sizes[g]].clone().requires_grad_(True)
            one = layer(alone, torch.zeros(sizes[g], dtype=torch.int64, device=dev))
            one.backward(go[lo:lo + sizes[g]])
            assert torch.equal(one, out[lo:lo + sizes[g]]), (type(layer).__name__, g)
            assert torch.equal(alone.grad, xx.grad[lo:lo + sizes[g]]), (type(layer).__name__, g)


def test_two_runs_agree_bit_for_bit(dev):
    F = 48
    sizes = [30] * 40 + [TH + 100, 3 * CH + 1] + [12] * 25
    x = torch.randn(sum(sizes), F, generator=gen(14)).to(dev)
    go = torch.randn(sum(sizes), F, generator=gen(15)).to(dev)
    batch = R.batch_of(sizes, dev)
    for layer in _layers(F, dev, seed=15):
        runs = []
        for _ in range(2):
            xx = x.clone().requires_grad_(True)
            layer.zero_grad()
            out = layer(xx, batch)
            out.backward(go)
            runs.append([out.detach(), xx.grad] + [p.grad.clone() for p in layer.parameters()])
        assert len(runs[0]) == 2 + len(list(layer.parameters()))
        for a, b in zip(*runs):
            assert torch.equal(a, b)


# ---- 64-bit addressing ------------------------------------------------------------------------------
def test_row_offsets_past_2_to_the_31(dev):
    """``row * ldx`` passes 2^31 from row 65,536 on when x is a slice of a 32,768-wide plane"""
    N, LD, F = 66_000, 32_768, 8
    sizes = [20_000, 45_000, 100, 900]
    assert sum(sizes) == N and (N - 1) * LD > 2 ** 31
    x = torch.empty(N, LD, device=dev)[:, :F]
    dense = (torch.randn(N, F, generator=gen(16)) + 2).to(dev)
    x.copy_(dense)
    x.requires_grad_(True)      # (a leaf: grad_x comes from the rows read at the wide pitch)
    go = torch.randn(N, F, generator=gen(17)).to(dev)
    batch = R.batch_of(sizes, dev)
    for layer, kind in zip(_layers(F, dev, seed=17), ('graph_norm', 'layer_norm')):
        params = {n: p.detach() for n, p in layer.named_parameters()}
        out64, gx64, gp64 = R.restate_with_grads(kind, dense, sizes, go, params, torch.float64)
        out32, gx32, gp32 = R.restate_with_grads(kind, dense, sizes, go, params, torch.float32)
        layer.zero_grad()
        x.grad = None
        out = layer(x, batch)
        out.backward(go)
        T.assert_close_scaled(out.double(), out64, tol=R.tol_of(R.scaled_err(out32, out64)),
                              what=f'{kind} out')
        T.assert_close_scaled(x.grad.double(), gx64, tol=R.tol_of(R.scaled_err(gx32, gx64)),
                              what=f'{kind} grad_x')
        for n, p in layer.named_parameters():
            T.assert_close_scaled(p.grad.double(), gp64[n],
                                  tol=R.tol_of(R.scaled_err(gp32[n], gp64[n])),
                                  what=f'{kind} grad_{n}')
    del x


# ---- memory ------------------------------------------------------------------------------------------
def test_memory_promise(dev):
    """forward + backward at N = 200,000, F = 128: the fused route allocates y, grad_x and O(B F +
    workspace) — under 2.5 N F 4 bytes plus the workspace formula; the generic route of the same
    commit, measured here too, is over that bound (otherwise this test would show nothing)"""
    N, F, per = 200_000, 128, 25
    sizes = [per] * (N // per)
    batch = R.batch_of(sizes, dev)
    x = torch.randn(N, F, device=dev).requires_grad_(True)
    go = torch.randn(N, F, device=dev)
    handle = _norm.batch_handle(batch, None)
    ws = _native.graph_norm_workspace_bytes(handle.hub.n_chunks, handle.hub.n_hub, F, True)
    bound = 2.5 * N * F * 4 + ws
    for layer in _layers(F, dev, seed=18):
        peaks = {}
        for fuse in (True, False):
            layer.fuse = fuse
            layer(x[:1000], batch[:1000].contiguous()).sum().backward()   # (caches, handles)
            x.grad = None
            layer.zero_grad()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = layer(x, batch)
            out.backward(go)
            torch.cuda.synchronize()
            peaks[fuse] = torch.cuda.max_memory_allocated() - before
            del out
            x.grad = None
        print(f'{type(layer).__name__}: fused {peaks[True] / 2 ** 20:.1f} MiB, generic '
              f'{peaks[False] / 2 ** 20:.1f} MiB, bound {bound / 2 ** 20:.1f} MiB')
        assert peaks[True] <= bound, (peaks, bound)
        assert peaks[False] > bound, (peaks, bound)


# ---- dtypes, operators, pools --------------------------------------------------------------------
def test_half_inputs_are_widened(dev, monkeypatch):
    F, sizes = 32, [10, 70, TH + 9]
    batch = R.batch_of(sizes, dev)
    x = torch.randn(sum(sizes), F, generator=gen(19))
    for low in (torch.float16, torch.bfloat16):
        for layer in _layers(F, dev, seed=19):
            half = layer.to(low)
            xl = x.to(dev).to(low)
            state = {}
            c = T._counted(monkeypatch, lambda: state.update(out=half(xl, batch)))
            assert c.calls.get(FWD) == 1, (low, c.calls)
            assert state['out'].dtype == low
            wide = type(layer)(F).to(dev)
            wide.load_state_dict({k: v.float() for k, v in half.state_dict().items()})
            want = wide(xl.float(), batch)
            assert torch.equal(state['out'], want.to(low))
            layer.float()


def test_registered_operator_under_torch_compile(dev):
    sizes = [4, 30, TH + 20, 0, 6]
    F = 16
    x = torch.randn(sum(sizes), F, generator=gen(20)).to(dev).requires_grad_(True)
    go = torch.randn(sum(sizes), F, generator=gen(21)).to(dev)
    ptr = R.ptr_of(sizes, dev)
    w, b, ms = (torch.rand(F, generator=gen(22 + i)).add(0.5).to(dev).requires_grad_(True)
                for i in range(3))

    def fn(x, w, b, ms):
        return torch.ops.pyg_amd.graph_norm(x, ptr, w, b, ms, 1e-5, 'channel', False)[0] * 2.0

    out = torch.compile(fn, fullgraph=True)(x, w, b, ms)
    grads = torch.autograd.grad(out, [x, w, b, ms], go)
    params = {'weight': w, 'bias': b, 'mean_scale': ms}
    out64, gx64, gp64 = R.restate_with_grads('graph_norm', x, sizes, 2.0 * go, params,
                                             torch.float64)
    _, _, gp32 = R.restate_with_grads('graph_norm', x, sizes, 2.0 * go, params, torch.float32)
    T.assert_close_scaled(out.double(), 2.0 * out64, what='compiled out')
    T.assert_close_scaled(grads[0].double(), gx64, what='compiled grad_x')
    for g, n in zip(grads[1:], params):
        T.assert_close_scaled(g.double(), gp64[n], tol=R.tol_of(R.scaled_err(gp32[n], gp64[n])),
                              what=f'compiled grad_{n}')
    y, mean, rstd = torch.ops.pyg_amd.graph_norm(x.detach(), ptr, w.detach(), b.detach(), None,
                                                 1e-5, 'graph', False)
    assert mean.shape == rstd.shape == (len(sizes), )
    want = R.restate('layer_norm', x.detach().double(), sizes, w.detach().double(),
                     b.detach().double())
    T.assert_close_scaled(y.double(), want, what='operator, graph mode')


def test_pools_on_the_device(dev):
    R.check_pools(dev)


def test_handle_is_shared_and_follows_the_batch_tensor(dev, monkeypatch):
    """all norm layers of a step share one handle per batch tensor: one plan per (batch, size)"""
    sizes = [12, TH + 1, 40]
    batch = R.batch_of(sizes, dev)
    x = torch.randn(sum(sizes), 16, device=dev)
    a, b = _layers(16, dev)

    def step():
        a(x, batch)
        b(x, batch)
        a(x, batch, 3)

    c = T._counted(monkeypatch, step)
    assert c.calls.get(FWD) == 3, c.calls
    assert c.calls.get('pygamd_hub_plan') == 2, c.calls   # (batch_size None and 3: two keys)
    before = a(x, batch)
    batch[-1] = 3            # an in-place edit: the cached handle is stale
    after = a(x, batch)
    assert not torch.equal(before[-1], after[-1])
