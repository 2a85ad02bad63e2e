"""nn.GATv2Conv / nn.GAT(v2=True) on the device: the recorded reference cases on the fused and the
generic route, the one-pass kernels against the float64 restatement (tests/_gatv2_ref.py) at
shapes that take every lane layout, long rows through the chunked schedule, bitwise
repeatability, the score-mode route, the memory and launch-count promises, routing, and the
registered operator.  Nothing here reads the reference tree: the golden file is the only thing
taken from it."""
import pytest
import torch

import _gatv2_ref as R
from _util import (_counted, assert_close, assert_close_scaled, assert_sum_close, gen,
                   random_graph)

pytestmark = pytest.mark.gpu

CASES = ['v2', 'v2_mean', 'v2_share', 'v2_noloops', 'v2_res_nobias', 'v2_c5', 'v2_pair', 'v2_edge',
         'v2_attention']


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('fuse', [True, False])
@pytest.mark.parametrize('name', CASES)
def test_golden_cases(dev, name, fuse):
    R.check_class_case(R.load_golden(), name, dev, fuse=fuse)


def test_golden_cases_int32_edge_index(dev):
    for name in ('v2', 'v2_pair', 'v2_attention'):
        R.check_class_case(R.load_golden(), name, dev, index_dtype=torch.int32)


@pytest.mark.parametrize('fuse', [True, False])
def test_golden_model(dev, fuse):
    R.check_model_case(R.load_golden(), dev, fuse=fuse)


# ---- the kernels against float64 ----------------------------------------------------------------------
def _problem(n_src, n_dst, ei, H, C, seed):
    g = gen(seed)
    return {'x_l': torch.randn(n_src, H, C, generator=g), 'x_r': torch.randn(n_dst, H, C, generator=g),
            'att': torch.randn(1, H, C, generator=g) / C ** 0.5,
            'go': torch.randn(n_dst, H, C, generator=g), 'ei': ei, 'n_dst': n_dst}


def _reference(P, dtype):
    leaves = [P[k].to(dtype).requires_grad_(True) for k in ('x_l', 'x_r', 'att')]
    out, alpha = R.attend(*leaves, P['ei'], P['n_dst'])
    grads = torch.autograd.grad(out, leaves, P['go'].to(dtype))
    return [out.detach(), alpha.detach()] + [g.detach() for g in grads]


def _device_run(P, dev, index_dtype=torch.int64, score=False):
    """(out, alpha in COO order, grad_x_l, grad_x_r, grad_att, handle) through the autograd nodes"""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import (Gatv2AttendFunction, Gatv2ScoreFunction,
                                                  SpmmFunction)
    leaves = [P[k].to(dev).requires_grad_(True) for k in ('x_l', 'x_r', 'att')]
    graph = P.get('graph')
    if graph is None or graph.edge_index.dtype != index_dtype:
        graph = as_edge_index(P['ei'].to(dev).to(index_dtype), leaves[0].size(0), P['n_dst'])
    H, C = leaves[0].shape[1:]
    if score:
        slot_alpha = Gatv2ScoreFunction.apply(*leaves, graph, 0.2, P['n_dst'])
        out = SpmmFunction.apply(leaves[0].reshape(-1, H * C), slot_alpha, graph, 'sum',
                                 'slot').view(-1, H, C)
    else:
        out = Gatv2AttendFunction.apply(*leaves, graph, 0.2, P['n_dst'])
        slot_alpha = out.grad_fn.saved_tensors[3] if hasattr(out.grad_fn, 'saved_tensors') else None
    grads = torch.autograd.grad(out, leaves, P['go'].to(dev))
    alpha = None
    if slot_alpha is not None:
        alpha = torch.empty_like(slot_alpha.detach())
        alpha[graph.by_dst().perm.long()] = slot_alpha.detach()
    return [out.detach(), alpha] + list(grads), graph


_UNIFORM = {}


def _uniform_graph():
    if not _UNIFORM:
        _UNIFORM['ei'] = random_graph(2000, 2000, 24000, 41)
    return _UNIFORM['ei']


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('H,C', [(1, 8), (3, 5), (4, 6), (2, 32), (8, 32), (4, 128)])
def test_kernels_match_float64(dev, H, C, index_dtype):
    """H*C below 64, odd widths, heads that straddle lanes, the float4 width and the 512 limit."""
    P = _problem(2000, 2000, _uniform_graph(), H, C, 100 + H * C)
    want = _reference(P, torch.float64)
    got, _ = _device_run(P, dev, index_dtype)
    for name, a, b in zip(('out', 'alpha', 'grad_x_l', 'grad_x_r', 'grad_att'), got, want):
        assert_close_scaled(a, b.float(), tol=2e-5, what=f'({H}, {C}) {name}')


def test_destinations_a_prefix_and_an_empty_graph(dev):
    ei = random_graph(900, 300, 5000, 43)
    P = _problem(900, 300, ei, 4, 6, 7)
    P['x_r'] = torch.randn(900, 4, 6, generator=gen(8))       # more rows than destinations
    want = _reference(P, torch.float64)
    got, _ = _device_run(P, dev)
    assert got[3].shape == (900, 4, 6) and float(got[3][300:].abs().max()) == 0.0
    for name, a, b in zip(('out', 'alpha', 'grad_x_l', 'grad_x_r', 'grad_att'), got, want):
        assert_close_scaled(a, b.float(), tol=2e-5, what=f'prefix {name}')
    E = _problem(50, 40, torch.zeros(2, 0, dtype=torch.int64), 2, 8, 9)
    got, _ = _device_run(E, dev)
    assert got[0].shape == (40, 2, 8) and float(got[0].abs().max()) == 0.0   # rows without slots
    assert all(float(g.abs().max()) == 0.0 for g in got[2:])


# ---- long rows ------------------------------------------------------------------------------------
_LONG = {}


def _long_problem():
    """N = 3000: destination 5 has 6000 edges, destination 11 exactly the hub threshold + 1,
    source 7 has 2000 out-edges (a long row of the by-source form); the rest is uniform."""
    from pytorch_geometric_amd import _native
    if not _LONG:
        g = gen(51)
        n = 3000
        thr = _native.HUB_THRESHOLD
        src = torch.cat([torch.randint(0, n, (20000, ), generator=g),
                         torch.randint(0, n, (6000, ), generator=g),
                         torch.randint(0, n, (thr + 1, ), generator=g),
                         torch.full((2000, ), 7)])
        base_dst = torch.randint(0, n, (20000, ), generator=g)
        base_dst[(base_dst == 5) | (base_dst == 11)] = 12
        dst = torch.cat([base_dst, torch.full((6000, ), 5), torch.full((thr + 1, ), 11),
                         torch.randint(12, n, (2000, ), generator=g)])
        perm = torch.randperm(src.numel(), generator=g)
        P = _problem(n, n, torch.stack([src, dst])[:, perm].contiguous(), 4, 16, 52)
        P['want64'] = _reference(P, torch.float64)
        P['want32'] = _reference(P, torch.float32)
        _LONG['P'] = P
    return _LONG['P']


def test_long_rows_match_float64(dev):
    from pytorch_geometric_amd import _native
    P = _long_problem()
    got, graph = _device_run(P, dev)
    P['graph'] = graph
    ptr = graph.by_dst().ptr
    assert int(ptr[6] - ptr[5]) == 6000 and int(ptr[12] - ptr[11]) == _native.HUB_THRESHOLD + 1
    names = ('out', 'alpha', 'grad_x_l', 'grad_x_r', 'grad_att')
    for name, a, w32, w64 in zip(names, got, P['want32'], P['want64']):
        if name in ('out', 'alpha'):
            assert_sum_close(a, w32, w64, what=f'long {name}')
        else:
            assert_close_scaled(a, w64.float(), tol=2e-5, what=f'long {name}')


def test_hub_rows_take_the_chunked_schedule(dev, monkeypatch):
    from pytorch_geometric_amd import _native
    P = _long_problem()
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    _device_run(P, dev)
    torch.cuda.synchronize()
    info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'gatv2'}
    assert set(info) == {'forward', 'backward_dst', 'backward_src'}
    chunk = _native.HUB_CHUNK
    want = -(-6000 // chunk) + -(-(_native.HUB_THRESHOLD + 1) // chunk)
    assert info['forward']['n_hub'] == 2 and info['forward']['n_chunks'] == want
    assert info['backward_dst']['n_hub'] == 2
    assert info['backward_src']['n_hub'] == 1                  # source 7
    # the uniform graph has no such row: one plain launch
    sink.clear()
    _device_run(_problem(2000, 2000, _uniform_graph(), 2, 8, 3), dev)
    assert [i['n_hub'] for i, _, _ in sink if i.get('kind') == 'gatv2'] == [0, 0, 0]


def test_two_runs_are_bitwise_identical(dev):
    """No float atomics anywhere — chunk partials are merged in chunk order, the att gradient is
    reduced per wave, per workgroup, then over a partials buffer — so EVERY result repeats."""
    P = _long_problem()
    a, graph = _device_run(P, dev)
    P['graph'] = graph
    b, _ = _device_run(P, dev)
    for name, x, y in zip(('out', 'alpha', 'grad_x_l', 'grad_x_r', 'grad_att'), a, b):
        assert torch.equal(x, y), f'{name} differs between two runs'


# ---- score mode -----------------------------------------------------------------------------------
def test_score_route_agrees_with_the_fused_route(dev):
    for P in (_problem(2000, 2000, _uniform_graph(), 4, 6, 61), _long_problem()):
        fused, _ = _device_run(P, dev)
        score, _ = _device_run(P, dev, score=True)
        for name, a, b in zip(('out', 'alpha', 'grad_x_l', 'grad_x_r', 'grad_att'), score, fused):
            if name == 'grad_att':
                # ONE sum over all E edges with cancellation (|terms| add up to ~1e3 here): two
                # summation orders differ by fp32 rounding of the tensor's magnitude, so the
                # 1e-5 is taken relative to that magnitude, not per element
                assert_close_scaled(a, b, tol=1e-5, what=f'score vs fused {name}')
            else:
                assert_close(a, b, what=f'score vs fused {name}')


def test_dropout_in_training_runs_in_score_mode(dev, monkeypatch):
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn import GATv2Conv
    torch.manual_seed(5)
    conv = GATv2Conv(16, 6, heads=4, dropout=0.5).to(dev).train()
    x = torch.randn(500, 16, generator=gen(62)).to(dev).requires_grad_(True)
    ei = random_graph(500, 500, 6000, 63).to(dev)
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    torch.manual_seed(77)
    out, (used, alpha) = conv(x, ei, return_attention_weights=True)
    out.sum().backward()
    assert [i['op'] for i, _, _ in sink if i.get('kind') == 'gatv2'] == \
        ['score', 'backward_dst', 'backward_src']
    monkeypatch.undo()
    assert used.size(1) == alpha.size(0) and alpha.shape[1] == 4
    dropped = float((alpha == 0).float().mean())
    assert 0.4 < dropped < 0.6                                  # post-dropout coefficients
    # ... which reproduce the output through a plain weighted scatter
    x_l = conv.lin_l(x.detach()).view(-1, 4, 6)
    msg = alpha.unsqueeze(-1) * x_l[used[0]]
    want = torch.zeros(500, 4, 6, device=dev).index_add_(0, used[1], msg).view(500, 24) + conv.bias
    assert_close(out, want, what='out from the returned coefficients')
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    # same seed, same mask: the route is reproducible
    torch.manual_seed(77)
    again, _ = conv(x, ei, return_attention_weights=True)
    assert torch.equal(again, out)
    # eval: the score route (coefficients asked for) and the fused route agree
    conv.eval()
    leaves = [x] + list(conv.parameters())
    go = torch.randn(500, 24, generator=gen(64)).to(dev)
    a, _ = conv(x, ei, return_attention_weights=True)
    b = conv(x, ei)
    assert_close(a, b, what='eval out')
    for n, ga, gb in zip(['x'] + [n for n, _ in conv.named_parameters()],
                         torch.autograd.grad(a, leaves, go), torch.autograd.grad(b, leaves, go)):
        assert_close(ga, gb, what=f'eval grad {n}')


# ---- nothing of size E x H*C ------------------------------------------------------------------------
def test_fused_route_keeps_nothing_of_edge_times_width(dev):
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import Gatv2AttendFunction
    N, E, H, C = 4096, 262144, 4, 32
    graph = as_edge_index(random_graph(N, N, E, 71).to(dev), N, N)
    graph.fill_cache_()
    graph.src_slot_to_dst_slot()
    g = gen(72)
    x_l = torch.randn(N, H, C, generator=g).to(dev).requires_grad_(True)
    x_r = torch.randn(N, H, C, generator=g).to(dev).requires_grad_(True)
    att = torch.randn(1, H, C, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(N, H, C, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = Gatv2AttendFunction.apply(x_l, x_r, att, graph, 0.2, N)
    grads = torch.autograd.grad(out, [x_l, x_r, att], go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'peak above the inputs: {extra / 2 ** 20:.1f} MiB')
    assert extra < E * H * C * 4 // 2                          # 64 MiB; one [E, H*C] is 128 MiB
    assert all(bool(torch.isfinite(t).all()) for t in grads)


# ---- launch counts ------------------------------------------------------------------------------------
def test_launch_counts(dev, monkeypatch):
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import Gatv2AttendFunction
    P = _problem(2000, 2000, _uniform_graph(), 4, 16, 81)
    graph = as_edge_index(P['ei'].to(dev), 2000, 2000)
    graph.fill_cache_()
    graph.src_slot_to_dst_slot()
    leaves = [P[k].to(dev).requires_grad_(True) for k in ('x_l', 'x_r', 'att')]
    go = P['go'].to(dev)
    state = {}

    def forward():
        state['out'] = Gatv2AttendFunction.apply(*leaves, graph, 0.2, 2000)

    c = _counted(monkeypatch, forward)
    assert c.calls == {'pygamd_gatv2_forward': 1}, c.calls

    c = _counted(monkeypatch, lambda: torch.autograd.grad(state['out'], leaves, go))
    assert c.order == ['pygamd_gatv2_workspace_bytes', 'pygamd_gatv2_backward_dst',
                       'pygamd_gatv2_backward_src'], c.order

    # a whole layer step: no SpMM, SDDMM or softmax launch anywhere
    from pytorch_geometric_amd.nn import GAT, GATv2Conv
    torch.manual_seed(3)
    conv = GATv2Conv(16, 8, heads=4).to(dev)
    x = torch.randn(2000, 16, generator=gen(82)).to(dev).requires_grad_(True)
    ei = P['ei'].to(dev)
    c = _counted(monkeypatch, lambda: conv(x, ei).sum().backward())
    assert c.calls['pygamd_gatv2_forward'] == 1 and c.calls['pygamd_gatv2_backward_dst'] == 1 \
        and c.calls['pygamd_gatv2_backward_src'] == 1
    assert not [n for n in c.calls if 'spmm' in n or 'sddmm' in n or 'softmax' in n], c.calls

    # a 3-layer model sorts the (self-looped) graph at most twice: by destination, by source
    model = GAT(16, 32, num_layers=3, out_channels=5, heads=4, v2=True).to(dev)
    c = _counted(monkeypatch, lambda: model(x, ei).sum().backward())
    assert c.calls['pygamd_gatv2_forward'] == 3
    assert c.calls.get('pygamd_index_sort', 0) <= 2, c.calls


# ---- routing --------------------------------------------------------------------------------------------
def test_routing_to_the_generic_route(dev, monkeypatch):
    from pytorch_geometric_amd.nn import GATv2Conv
    ei = random_graph(300, 300, 3000, 91)
    x = torch.randn(300, 16, generator=gen(92))
    ea = torch.randn(3000, 3, generator=gen(93))
    for what, kw, fuse, attr in (('edge_dim', dict(heads=2, out_channels=8, edge_dim=3), True, ea),
                                 ('fuse off', dict(heads=2, out_channels=8), False, None),
                                 ('H*C = 1024', dict(heads=8, out_channels=128), True, None)):
        torch.manual_seed(9)
        conv = GATv2Conv(16, **kw).to(dev)
        conv.fuse = fuse
        xd = x.to(dev).requires_grad_(True)
        state = {}

        def step():
            state['out'] = conv(xd, ei.to(dev), edge_attr=None if attr is None else attr.to(dev))
            state['grad'] = torch.autograd.grad(state['out'].sum(), xd)[0]

        c = _counted(monkeypatch, step)
        assert not [n for n in c.calls if 'gatv2_forward' in n or 'gatv2_backward' in n], what
        p = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
        x64 = x.double().requires_grad_(True)
        want, _, _ = R.conv(x64, ei, p, edge_attr=None if attr is None else attr.double(), **kw)
        assert_close_scaled(state['out'], want.detach().float(), tol=2e-5, what=f'{what} out')
        assert_close_scaled(state['grad'], torch.autograd.grad(want.sum(), x64)[0].float(),
                            tol=2e-5, what=f'{what} grad_x')
    # the fused route is what a plain layer takes
    conv = GATv2Conv(16, 8, heads=2).to(dev)
    c = _counted(monkeypatch, lambda: conv(x.to(dev), ei.to(dev)))
    assert c.calls.get('pygamd_gatv2_forward') == 1
    flipped = GATv2Conv(16, 8, heads=2, flow='target_to_source').to(dev)
    c = _counted(monkeypatch, lambda: flipped(x.to(dev), ei.to(dev)))
    assert 'pygamd_gatv2_forward' not in c.calls


def test_half_inputs_are_widened(dev):
    from pytorch_geometric_amd.nn import GATv2Conv
    torch.manual_seed(4)
    conv = GATv2Conv(16, 8, heads=2).to(dev)
    x = torch.randn(300, 16, generator=gen(94)).to(dev)
    ei = random_graph(300, 300, 3000, 95).to(dev)
    want = conv(x, ei)
    got = conv.half()(x.half(), ei)
    assert got.dtype == torch.float16
    assert_close_scaled(got.float(), want, tol=2e-2, what='half')


# ---- the registered operator ------------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.pyg_amd.gatv2_attend
    with FakeTensorMode():
        x_l = torch.empty(50, 4, 8, device='cuda', requires_grad=True)
        x_r = torch.empty(12, 4, 8, device='cuda')
        att = torch.empty(1, 4, 8, device='cuda')
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        out, alpha = op(x_l, x_r, att, ptr, col, 0.2)
        assert out.shape == (12, 4, 8) and alpha.shape == (400, 4) and out.requires_grad
        assert out.device.type == 'cuda' and out.dtype == torch.float32

    P = _problem(2000, 2000, _uniform_graph(), 4, 6, 97)
    want = _reference(P, torch.float64)
    order = torch.argsort(P['ei'][1], stable=True)
    col = P['ei'][0][order].to(dev)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], 2000).to(dev)
    go = P['go'].to(dev)

    def fn(a, b, c):
        out, _ = op(a * 1.0, b, c, ptr, col, 0.2)
        return (out * go).sum()

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        leaves = [P[k].to(dev).requires_grad_(True) for k in ('x_l', 'x_r', 'att')]
        y = f(*leaves)
        results.append([y.detach()] + list(torch.autograd.grad(y, leaves)))
    for a, b in zip(*results):
        assert_close(b, a, what='compiled vs eager')
    for name, a, b in zip(('grad_x_l', 'grad_x_r', 'grad_att'), results[0][1:], want[2:]):
        assert_close_scaled(a, b.float(), tol=2e-5, what=f'operator {name}')
    out, alpha = op(P['x_l'].to(dev), P['x_r'].to(dev), P['att'].to(dev), ptr, col, 0.2)
    assert_close_scaled(out, want[0].float(), tol=2e-5, what='operator out')
    assert_close_scaled(alpha, want[1][order].float(), tol=2e-5, what='operator alpha')
    torch.library.opcheck(op, (P['x_l'].to(dev).requires_grad_(True), P['x_r'].to(dev),
                               P['att'].to(dev), ptr, col, 0.2))
