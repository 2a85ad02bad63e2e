"""nn.TransformerConv on the device: the recorded reference cases on the fused and the generic
route, the one-pass kernels against the float64 restatement (tests/_transformer_ref.py) at shapes
that take every lane layout — with separate key / value tensors and with the packed projection —
long rows through the chunked schedule, bitwise repeatability, the score-mode route, the memory
and launch-count promises, routing, and the registered operator.  Nothing here reads the reference
tree: the golden file is the only thing taken from it."""
import math

import pytest
import torch

import _transformer_ref as R
from _util import (_counted, assert_close, assert_close_scaled, assert_sum_close, gen,
                   random_graph)

pytestmark = pytest.mark.gpu

CASES = ['t', 't_mean', 't_beta', 't_beta_mean', 't_noroot', 't_nobias', 't_c5', 't_pair', 't_edge',
         't_attention']
NAMES = ('out', 'alpha', 'grad_query', 'grad_key', 'grad_value')


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('fuse', [True, False])
@pytest.mark.parametrize('name', CASES)
def test_golden_cases(dev, name, fuse):
    R.check_class_case(R.load_golden(), name, dev, fuse=fuse)


def test_golden_cases_int32_edge_index(dev):
    for name in ('t', 't_pair', 't_attention'):
        R.check_class_case(R.load_golden(), name, dev, index_dtype=torch.int32)


# ---- the kernels against float64 ----------------------------------------------------------------------
def _problem(n_src, n_dst, ei, H, C, seed):
    g = gen(seed)
    return {'q': torch.randn(n_dst, H, C, generator=g), 'k': torch.randn(n_src, H, C, generator=g),
            'v': torch.randn(n_src, H, C, generator=g),
            'go': torch.randn(n_dst, H, C, generator=g), 'ei': ei, 'n_dst': n_dst}


def _reference(P, dtype):
    leaves = [P[k].to(dtype).requires_grad_(True) for k in ('q', 'k', 'v')]
    out, alpha = R.attend(*leaves, P['ei'], P['n_dst'])
    grads = torch.autograd.grad(out, leaves, P['go'].to(dtype))
    return [out.detach(), alpha.detach()] + [g.detach() for g in grads]


def _device_run(P, dev, index_dtype=torch.int64, score=False, packed=False):
    """(out, alpha in COO order, grad_query, grad_key, grad_value, handle) through the autograd
    nodes; ``packed``: key and value as the halves of one [N_src, 2, H, C] leaf (ld = 2 * H * C)"""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import (SpmmFunction, TransformerAttendFunction,
                                                  TransformerScoreFunction)
    q, k, v = [P[n].to(dev).requires_grad_(True) for n in ('q', 'k', 'v')]
    n_src, H, C = k.shape
    graph = P.get('graph')
    if graph is None or graph.edge_index.dtype != index_dtype:
        graph = as_edge_index(P['ei'].to(dev).to(index_dtype), n_src, P['n_dst'])
    scale = 1.0 / math.sqrt(C)
    go = P['go'].to(dev)
    if score:
        slot_alpha = TransformerScoreFunction.apply(q, k, graph, scale, P['n_dst'])
        out = SpmmFunction.apply(v.reshape(-1, H * C), slot_alpha, graph, 'sum',
                                 'slot').view(-1, H, C)
        grads = torch.autograd.grad(out, [q, k, v], go)
    elif packed:
        kv = torch.stack([k.detach(), v.detach()], dim=1).requires_grad_(True)   # [N_src, 2, H, C]
        out = TransformerAttendFunction.apply(q, kv, None, graph, scale, P['n_dst'])
        slot_alpha = out.grad_fn.saved_tensors[3]
        g_q, g_kv = torch.autograd.grad(out, [q, kv], go)
        grads = [g_q, g_kv[:, 0], g_kv[:, 1]]
    else:
        out = TransformerAttendFunction.apply(q, k, v, graph, scale, P['n_dst'])
        slot_alpha = out.grad_fn.saved_tensors[3]
        grads = torch.autograd.grad(out, [q, k, v], go)
    alpha = torch.empty_like(slot_alpha.detach())
    alpha[graph.by_dst().perm.long()] = slot_alpha.detach()
    return [out.detach(), alpha] + list(grads), graph


_UNIFORM = {}


def _uniform_graph():
    if not _UNIFORM:
        _UNIFORM['ei'] = random_graph(2000, 2000, 24000, 41)
    return _UNIFORM['ei']


def _uniform_case(H, C):
    """problem and float64 results at one head layout, computed once for both index dtypes"""
    if (H, C) not in _UNIFORM:
        P = _problem(2000, 2000, _uniform_graph(), H, C, 100 + H * C)
        _UNIFORM[(H, C)] = (P, _reference(P, torch.float64))
    return _UNIFORM[(H, C)]


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('H,C', [(1, 8), (3, 5), (4, 6), (2, 32), (8, 32), (4, 128)])
def test_kernels_match_float64(dev, H, C, index_dtype):
    """H*C below 64, odd widths, heads that straddle lanes, the float4 width and the 512 limit;
    separate contiguous key and value (ld = H*C), then the packed projection (ld = 2*H*C)."""
    P, want = _uniform_case(H, C)
    for packed in (False, True):
        got, _ = _device_run(P, dev, index_dtype, packed=packed)
        for name, a, b in zip(NAMES, got, want):
            assert_close_scaled(a, b.float(), tol=2e-5,
                                what=f'({H}, {C}) {"packed " if packed else ""}{name}')


def test_strided_views_of_one_projection_are_read_in_place(dev, monkeypatch):
    """key = kv[:, :W] and value = kv[:, W:] handed over as two tensors: same stride, no copy."""
    from pytorch_geometric_amd import _native, as_edge_index
    P, want = _uniform_case(4, 6)
    kv = torch.cat([P['k'].reshape(2000, 24), P['v'].reshape(2000, 24)], dim=1).to(dev)
    graph = as_edge_index(P['ei'].to(dev), 2000, 2000)
    fwd = graph.by_dst()
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    alpha, out = _native.transformer_forward(fwd.ptr, fwd.idx, P['q'].to(dev).reshape(2000, 24),
                                             kv[:, :24], kv[:, 24:], 4, 6, 1 / math.sqrt(6),
                                             hub=fwd.hub)
    torch.cuda.synchronize()
    assert [i['ld'] for i, _, _ in sink if i.get('kind') == 'transformer'] == [48]
    assert_close_scaled(out.view(2000, 4, 6), want[0].float(), tol=2e-5, what='views out')


def test_destinations_a_prefix_and_an_empty_graph(dev):
    ei = random_graph(900, 300, 5000, 43)
    P = _problem(900, 300, ei, 4, 6, 7)
    P['q'] = torch.randn(900, 4, 6, generator=gen(8))       # more rows than destinations
    want = _reference(P, torch.float64)
    for packed in (False, True):
        got, _ = _device_run(P, dev, packed=packed)
        assert got[2].shape == (900, 4, 6) and float(got[2][300:].abs().max()) == 0.0
        for name, a, b in zip(NAMES, got, want):
            assert_close_scaled(a, b.float(), tol=2e-5, what=f'prefix {name}')
    E = _problem(50, 40, torch.zeros(2, 0, dtype=torch.int64), 2, 8, 9)
    for packed in (False, True):
        got, _ = _device_run(E, dev, packed=packed)
        assert got[0].shape == (40, 2, 8) and float(got[0].abs().max()) == 0.0   # rows without slots
        assert got[3].shape == (50, 2, 8) and got[4].shape == (50, 2, 8)
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


@pytest.mark.parametrize('packed', [False, True])
def test_long_rows_match_float64(dev, packed):
    from pytorch_geometric_amd import _native
    P = _long_problem()
    got, graph = _device_run(P, dev, packed=packed)
    P['graph'] = graph
    ptr = graph.by_dst().ptr
    assert int(ptr[6] - ptr[5]) == 6000 and int(ptr[12] - ptr[11]) == _native.HUB_THRESHOLD + 1
    for name, a, w32, w64 in zip(NAMES, got, P['want32'], P['want64']):
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
    info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'transformer'}
    assert set(info) == {'forward', 'backward_dst', 'backward_src'}
    chunk = _native.HUB_CHUNK
    want = -(-6000 // chunk) + -(-(_native.HUB_THRESHOLD + 1) // chunk)
    assert info['forward']['n_hub'] == 2 and info['forward']['n_chunks'] == want
    assert info['backward_dst']['n_hub'] == 2 and info['backward_dst']['n_chunks'] == want
    assert info['backward_src']['n_hub'] == 1                  # source 7
    assert info['backward_src']['n_chunks'] >= -(-2000 // chunk)
    # the uniform graph has no such row: one plain launch each
    sink.clear()
    _device_run(_problem(2000, 2000, _uniform_graph(), 2, 8, 3), dev)
    records = [i for i, _, _ in sink if i.get('kind') == 'transformer']
    assert [i['op'] for i in records] == ['forward', 'backward_dst', 'backward_src']
    assert [i['n_hub'] for i in records] == [0, 0, 0]
    assert [i['n_chunks'] for i in records] == [0, 0, 0]


@pytest.mark.parametrize('packed', [False, True])
def test_two_runs_are_bitwise_identical(dev, packed):
    """No float atomics anywhere — chunk partials are merged in chunk order — so EVERY output and
    gradient repeats bit for bit, long rows included."""
    P = _long_problem()
    a, graph = _device_run(P, dev, packed=packed)
    P['graph'] = graph
    b, _ = _device_run(P, dev, packed=packed)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), f'{name} differs between two runs'
    s1, _ = _device_run(P, dev, score=True)
    s2, _ = _device_run(P, dev, score=True)
    for name, x, y in zip(NAMES, s1, s2):
        assert torch.equal(x, y), f'score mode: {name} differs between two runs'


# ---- score mode -----------------------------------------------------------------------------------
def test_score_route_agrees_with_the_fused_route(dev):
    for P in (_problem(2000, 2000, _uniform_graph(), 4, 6, 61), _long_problem()):
        fused, _ = _device_run(P, dev)
        score, _ = _device_run(P, dev, score=True)
        for name, a, b in zip(NAMES, score, fused):
            assert_close(a, b, what=f'score vs fused {name}')


def test_dropout_in_training_runs_in_score_mode(dev, monkeypatch):
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn import TransformerConv
    torch.manual_seed(5)
    conv = TransformerConv(16, 6, heads=4, dropout=0.5).to(dev).train()
    x = torch.randn(500, 16, generator=gen(62)).to(dev).requires_grad_(True)
    ei = random_graph(500, 500, 6000, 63).to(dev)
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    torch.manual_seed(77)
    out, (used, alpha) = conv(x, ei, return_attention_weights=True)
    out.sum().backward()
    assert [i['op'] for i, _, _ in sink if i.get('kind') == 'transformer'] == \
        ['score', 'backward_dst', 'backward_src']
    monkeypatch.undo()
    assert torch.equal(used, ei) and alpha.shape == (6000, 4)
    # the PRE-dropout softmax (transformer_conv.py:274-276), in the caller's edge order: every
    # destination's coefficients sum to one and none was zeroed
    sums = torch.zeros(500, 4, device=dev).index_add_(0, ei[1], alpha.detach())
    has = torch.bincount(ei[1], minlength=500) > 0
    assert float((sums[has] - 1).abs().max()) <= 1e-5
    assert int((alpha == 0).sum()) == 0
    q = conv.lin_query(x.detach()).view(-1, 4, 6).double().cpu()
    k = conv.lin_key(x.detach()).view(-1, 4, 6).double().cpu()
    _, want_alpha = R.attend(q, k, k, ei.cpu(), 500)
    assert_close_scaled(alpha, want_alpha.float(), tol=2e-5, what='returned coefficients')
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    # the output did see dropout: it differs from the eval output, and the same seed repeats it
    torch.manual_seed(77)
    again, _ = conv(x, ei, return_attention_weights=True)
    assert torch.equal(again, out)
    torch.manual_seed(78)
    other, _ = conv(x, ei, return_attention_weights=True)
    assert not torch.equal(other, out)
    # without the request the training layer takes the same route
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    torch.manual_seed(77)
    plain = conv(x, ei)
    assert [i['op'] for i, _, _ in sink if i.get('kind') == 'transformer'] == ['score']
    monkeypatch.undo()
    assert torch.equal(plain, out)
    # eval: the score route (coefficients asked for, True or False) and the fused route agree
    conv.eval()
    leaves = [x] + list(conv.parameters())
    go = torch.randn(500, 24, generator=gen(64)).to(dev)
    a, (_, alpha_eval) = conv(x, ei, return_attention_weights=False)
    b = conv(x, ei)
    assert_close(a, b, what='eval out')
    assert_close(alpha_eval, alpha, what='eval coefficients = training coefficients')
    for n, ga, gb in zip(['x'] + [n for n, _ in conv.named_parameters()],
                         torch.autograd.grad(a, leaves, go), torch.autograd.grad(b, leaves, go)):
        assert_close(ga, gb, what=f'eval grad {n}')


# ---- nothing of size E x H*C ------------------------------------------------------------------------
def test_fused_route_keeps_nothing_of_edge_times_width(dev):
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import TransformerAttendFunction
    N, E, H, C = 4096, 262144, 4, 32
    graph = as_edge_index(random_graph(N, N, E, 71).to(dev), N, N)
    graph.fill_cache_()
    graph.src_slot_to_dst_slot()
    g = gen(72)
    q = torch.randn(N, H, C, generator=g).to(dev).requires_grad_(True)
    kv = torch.randn(N, 2, H, C, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(N, H, C, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = TransformerAttendFunction.apply(q, kv, None, graph, 1 / math.sqrt(C), N)
    grads = torch.autograd.grad(out, [q, kv], go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'peak above the inputs: {extra / 2 ** 20:.1f} MiB')
    assert extra < E * H * C * 4 // 2                          # 64 MiB; one [E, H*C] is 128 MiB
    assert all(bool(torch.isfinite(t).all()) for t in grads)


# ---- launch counts ------------------------------------------------------------------------------------
def _gemms(sink, op):
    return sum(1 for i, _, _ in sink if i.get('kind') == 'gemm' and i.get('op') == op)


def test_launch_counts(dev, monkeypatch):
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import TransformerAttendFunction
    P = _problem(2000, 2000, _uniform_graph(), 4, 16, 81)
    graph = as_edge_index(P['ei'].to(dev), 2000, 2000)
    graph.fill_cache_()
    graph.src_slot_to_dst_slot()
    leaves = [P[k].to(dev).requires_grad_(True) for k in ('q', 'k', 'v')]
    go = P['go'].to(dev)
    state = {}

    def forward():
        state['out'] = TransformerAttendFunction.apply(*leaves, graph, 0.25, 2000)

    c = _counted(monkeypatch, forward)
    assert c.calls == {'pygamd_transformer_forward': 1}, c.calls

    c = _counted(monkeypatch, lambda: torch.autograd.grad(state['out'], leaves, go))
    assert c.order == ['pygamd_transformer_workspace_bytes', 'pygamd_transformer_backward_dst',
                       'pygamd_transformer_backward_src'], c.order

    # a whole layer step: no SpMM, SDDMM or softmax launch anywhere
    from pytorch_geometric_amd.nn import TransformerConv
    torch.manual_seed(3)
    conv = TransformerConv(16, 8, heads=4).to(dev)
    x = torch.randn(2000, 16, generator=gen(82)).to(dev).requires_grad_(True)
    ei = P['ei'].to(dev)
    fused = []
    c = _counted(monkeypatch, lambda: conv(x, ei).sum().backward(), sink=fused)
    assert c.calls['pygamd_transformer_forward'] == 1 \
        and c.calls['pygamd_transformer_backward_dst'] == 1 \
        and c.calls['pygamd_transformer_backward_src'] == 1
    assert not [n for n in c.calls if 'spmm' in n or 'sddmm' in n or 'softmax' in n], c.calls
    # ... and ONE projection for key + value: query, key | value, skip = three products forward
    # where the generic route makes four, and one input-gradient product less in the backward
    assert _gemms(fused, 'forward') == 3, [i for i, _, _ in fused]
    conv.fuse = False
    generic = []
    g = _counted(monkeypatch, lambda: conv(x, ei).sum().backward(), sink=generic)
    assert _gemms(generic, 'forward') == 4, [i for i, _, _ in generic]
    assert _gemms(fused, 'dgrad') == _gemms(generic, 'dgrad') - 1 == 3
    assert not [n for n in g.calls if 'transformer_forward' in n or 'transformer_backward' in n], \
        g.calls


# ---- routing --------------------------------------------------------------------------------------------
def test_routing_to_the_generic_route(dev, monkeypatch):
    from pytorch_geometric_amd.nn import TransformerConv
    ei = random_graph(300, 300, 3000, 91)
    x = torch.randn(300, 16, generator=gen(92))
    ea = torch.randn(3000, 3, generator=gen(93))
    for what, kw, fuse, attr in (
            ('edge_dim', dict(heads=2, out_channels=8, edge_dim=3), True, ea),
            ('fuse off', dict(heads=2, out_channels=8, beta=True), False, None),
            ('H*C = 1024', dict(heads=8, out_channels=128), True, None),
            ('target_to_source', dict(heads=2, out_channels=8, flow='target_to_source'), True,
             None)):
        torch.manual_seed(9)
        conv = TransformerConv(16, **kw).to(dev)
        conv.fuse = fuse
        xd = x.to(dev).requires_grad_(True)
        state = {}

        def step():
            state['out'] = conv(xd, ei.to(dev), edge_attr=None if attr is None else attr.to(dev))
            state['grad'] = torch.autograd.grad(state['out'].sum(), xd)[0]

        c = _counted(monkeypatch, step)
        assert not [n for n in c.calls if 'transformer_forward' in n or 'transformer_backward' in n], \
            (what, c.calls)                      # (the `supported` query is no launch)
        p = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
        x64 = x.double().requires_grad_(True)
        flipped = kw.get('flow') == 'target_to_source'     # the roles of the two rows swap
        want, _ = R.conv(x64, ei.flip(0) if flipped else ei, p,
                         edge_attr=None if attr is None else attr.double(),
                         **{k: v for k, v in kw.items() if k != 'flow'})
        assert_close_scaled(state['out'], want.detach().float(), tol=2e-5, what=f'{what} out')
        assert_close_scaled(state['grad'], torch.autograd.grad(want.sum(), x64)[0].float(),
                            tol=2e-5, what=f'{what} grad_x')
    # the fused route is what a plain layer takes
    conv = TransformerConv(16, 8, heads=2).to(dev)
    c = _counted(monkeypatch, lambda: conv(x.to(dev), ei.to(dev)))
    assert c.calls.get('pygamd_transformer_forward') == 1


def test_half_inputs_are_widened(dev):
    from pytorch_geometric_amd.nn import TransformerConv
    torch.manual_seed(4)
    conv = TransformerConv(16, 8, heads=2, beta=True).to(dev)
    x = torch.randn(300, 16, generator=gen(94)).to(dev)
    ei = random_graph(300, 300, 3000, 95).to(dev)
    want = conv(x, ei)
    got = conv.half()(x.half(), ei)
    assert got.dtype == torch.float16
    assert_close_scaled(got.float(), want, tol=2e-2, what='half')


def test_inside_hetero_conv(dev):
    from pytorch_geometric_amd.nn import HeteroConv, TransformerConv
    torch.manual_seed(6)
    layer = TransformerConv((16, 12), 8, heads=2)
    hetero = HeteroConv({('a', 'to', 'b'): layer}).to(dev)
    g = gen(96)
    x_a, x_b = torch.randn(400, 16, generator=g), torch.randn(150, 12, generator=g)
    ei = random_graph(400, 150, 2500, 97)
    xa, xb = x_a.to(dev).requires_grad_(True), x_b.to(dev).requires_grad_(True)
    out = hetero({'a': xa, 'b': xb}, {('a', 'to', 'b'): ei.to(dev)})
    assert set(out) == {'b'} and out['b'].shape == (150, 16)
    grads = torch.autograd.grad(out['b'].sum(), [xa, xb])
    p = {k: v.detach().cpu().double() for k, v in layer.state_dict().items()}
    a64, b64 = x_a.double().requires_grad_(True), x_b.double().requires_grad_(True)
    want, _ = R.conv((a64, b64), ei, p, heads=2, out_channels=8)
    assert_close_scaled(out['b'], want.detach().float(), tol=2e-5, what='hetero out')
    for name, got, ref in zip(('grad a', 'grad b'), grads,
                              torch.autograd.grad(want.sum(), [a64, b64])):
        assert_close_scaled(got, ref.float(), tol=2e-5, what=f'hetero {name}')


# ---- the registered operator ------------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'transformer_attend' in ops.OPS and 'transformer_attend_backward' in ops.OPS
    op = torch.ops.pyg_amd.transformer_attend
    with FakeTensorMode():
        q = torch.empty(12, 4, 8, device='cuda', requires_grad=True)
        k = torch.empty(50, 4, 8, device='cuda')
        v = torch.empty(50, 4, 8, device='cuda')
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        out, alpha = op(q, k, v, ptr, col, 0.35)
        assert out.shape == (12, 4, 8) and alpha.shape == (400, 4) and out.requires_grad
        assert out.device.type == 'cuda' and out.dtype == torch.float32

    P, want = _uniform_case(4, 6)
    order = torch.argsort(P['ei'][1], stable=True)
    col = P['ei'][0][order].to(dev)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], 2000).to(dev)
    go = P['go'].to(dev)
    scale = 1 / math.sqrt(6)

    def fn(a, b, c):
        out, _ = op(a * 1.0, b, c, ptr, col, scale)
        return (out * go).sum()

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        leaves = [P[n].to(dev).requires_grad_(True) for n in ('q', 'k', 'v')]
        y = f(*leaves)
        results.append([y.detach()] + list(torch.autograd.grad(y, leaves)))
    for a, b in zip(*results):
        assert_close(b, a, what='compiled vs eager')
    for name, a, b in zip(NAMES[2:], results[0][1:], want[2:]):
        assert_close_scaled(a, b.float(), tol=2e-5, what=f'operator {name}')
    out, alpha = op(P['q'].to(dev), P['k'].to(dev), P['v'].to(dev), ptr, col, scale)
    assert_close_scaled(out, want[0].float(), tol=2e-5, what='operator out')
    assert_close_scaled(alpha, want[1][order].float(), tol=2e-5, what='operator alpha')
    torch.library.opcheck(op, (P['q'].to(dev).requires_grad_(True), P['k'].to(dev),
                               P['v'].to(dev), ptr, col, scale))
