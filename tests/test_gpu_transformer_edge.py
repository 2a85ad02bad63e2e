"""nn.TransformerConv with edge features inside the one-pass kernels (``fuse_edge = True``): the
recorded reference cases with their launch counts, the kernels against the float64 restatement of
the node (tests/_transformer_edge_ref.py) at shapes that take every lane layout of the edge
registers, long rows through the chunked schedule, bitwise repeatability, the score-mode route,
the memory promise, routing, half inputs, HeteroConv and the registered operator.  Helpers and
tolerances are those of tests/test_gpu_transformer.py.  Nothing here reads the reference tree."""
import math

import pytest
import torch

import _transformer_edge_ref as RE
import _transformer_ref as R
import test_gpu_transformer as T
from _util import assert_close, assert_close_scaled, assert_sum_close, gen, random_graph

pytestmark = pytest.mark.gpu

NAMES = ('out_nodes', 'z', 'alpha', 'grad_query', 'grad_key', 'grad_value', 'grad_b',
         'grad_edge_attr')


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', RE.CASES)
def test_golden_cases_on_the_fused_edge_route(dev, monkeypatch, name, index_dtype):
    """Every recorded case with ``fuse_edge = True``; and the launches of a step: ONE edge forward,
    ONE edge backward by destination, ONE (unchanged) backward by source.  Without the request
    for the coefficients nothing else touches the edges: no SpMM, SDDMM or softmax launch.  (The
    case that asks for them runs in score mode, whose aggregation IS the weighted SpMM.)"""
    c = T._counted(monkeypatch, lambda: RE.check_class_case(RE.load_golden(), name, dev,
                                                            index_dtype=index_dtype))
    assert c.calls.get('pygamd_transformer_edge_forward') == 1, c.calls
    assert c.calls.get('pygamd_transformer_edge_backward_dst') == 1, c.calls
    assert c.calls.get('pygamd_transformer_backward_src') == 1, c.calls
    assert 'pygamd_transformer_forward' not in c.calls, c.calls
    assert 'pygamd_transformer_backward_dst' not in c.calls, c.calls
    if name != 'e_attention':
        assert not [n for n in c.calls if 'spmm' in n or 'sddmm' in n or 'softmax' in n], c.calls


# ---- the kernels against float64 ----------------------------------------------------------------------
def _problem(n_src, n_dst, ei, H, C, De, seed):
    g = gen(seed)
    return {'q': torch.randn(n_dst, H, C, generator=g), 'k': torch.randn(n_src, H, C, generator=g),
            'v': torch.randn(n_src, H, C, generator=g),
            'a': torch.randn(ei.size(1), De, generator=g),
            'b': torch.randn(n_dst, H, De, generator=g) / math.sqrt(De),
            'go': torch.randn(n_dst, H, C, generator=g),
            'gz': torch.randn(n_dst, H, De, generator=g), 'ei': ei, 'n_dst': n_dst}


LEAVES = ('q', 'k', 'v', 'b', 'a')


def _reference(P, dtype):
    """[out_nodes, z, alpha, grad_query, grad_key, grad_value, grad_b, grad_edge_attr]"""
    q, k, v, b, a = [P[n].detach().to(dtype).requires_grad_(True) for n in LEAVES]
    out, z, alpha = RE.attend_edge(q, k, v, a, b, P['ei'], P['n_dst'])
    grads = torch.autograd.grad([out, z], [q, k, v, b, a],
                                [P['go'].to(dtype), P['gz'].to(dtype)])
    return [out.detach(), z.detach(), alpha.detach()] + [g.detach() for g in grads]


def _device_run(P, dev, index_dtype=torch.int64, score=False, packed=False, edge_grad=True):
    """the same eight through the autograd nodes (alpha in COO order; grad_edge_attr None without
    ``edge_grad``), and the handle"""
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import (SegmentFunction, SpmmFunction,
                                                  TransformerEdgeAttendFunction,
                                                  TransformerEdgeScoreFunction)
    q, k, v, b = [P[n].detach().to(dev).requires_grad_(True) for n in ('q', 'k', 'v', 'b')]
    a = P['a'].detach().to(dev).requires_grad_(edge_grad)
    n_src, H, C = k.shape
    De = a.size(1)
    graph = P.get('graph')
    if graph is None or graph.edge_index.dtype != index_dtype:
        graph = as_edge_index(P['ei'].to(dev).to(index_dtype), n_src, P['n_dst'])
    scale = 1.0 / math.sqrt(C)
    heads = [P['go'].to(dev), P['gz'].to(dev)]
    wrt = [q, k, v, b] + ([a] if edge_grad else [])
    perm = graph.by_dst().perm.long()
    if score:
        slot_alpha = TransformerEdgeScoreFunction.apply(q, k, a, b, graph, scale, P['n_dst'])
        out = SpmmFunction.apply(v.reshape(-1, H * C), slot_alpha, graph, 'sum',
                                 'slot').view(-1, H, C)
        z = SegmentFunction.apply((slot_alpha.unsqueeze(-1) * a[perm].unsqueeze(1))
                                  .reshape(-1, H * De), graph.by_dst().ptr, 'sum').view(-1, H, De)
        grads = list(torch.autograd.grad([out, z], wrt, heads))
    elif packed:
        kv = torch.stack([k.detach(), v.detach()], dim=1).requires_grad_(True)   # [N_src, 2, H, C]
        out, z = TransformerEdgeAttendFunction.apply(q, kv, None, a, b, graph, scale, P['n_dst'])
        slot_alpha = out.grad_fn.saved_tensors[5]
        g = torch.autograd.grad([out, z], [q, kv] + wrt[3:], heads)
        grads = [g[0], g[1][:, 0], g[1][:, 1]] + list(g[2:])
    else:
        out, z = TransformerEdgeAttendFunction.apply(q, k, v, a, b, graph, scale, P['n_dst'])
        slot_alpha = out.grad_fn.saved_tensors[5]
        grads = list(torch.autograd.grad([out, z], wrt, heads))
    alpha = torch.empty_like(slot_alpha.detach())
    alpha[perm] = slot_alpha.detach()
    if not edge_grad:
        grads.append(None)
    return [out.detach(), z.detach(), alpha] + grads, graph


_UNIFORM = {}


def _uniform_case(H, C, De):
    """problem and float64 results at one layout, computed once for both index dtypes"""
    if (H, C, De) not in _UNIFORM:
        P = _problem(2000, 2000, T._uniform_graph(), H, C, De, 200 + H * C + De)
        _UNIFORM[(H, C, De)] = (P, _reference(P, torch.float64))
    return _UNIFORM[(H, C, De)]


@pytest.mark.parametrize('index_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('H,C,De', [(1, 8, 1), (3, 5, 3), (4, 6, 7), (2, 32, 16), (8, 32, 4),
                                    (4, 128, 32), (64, 8, 2), (8, 8, 32)])
def test_kernels_match_float64(dev, H, C, De, index_dtype):
    """De below, equal to and above the lanes of a head, De > C, the float4 width, the 512 limit
    and one lane per head; (8, 8, 32) widens the lane group beyond what C alone would take;
    separate key and value, then the packed projection."""
    P, want = _uniform_case(H, C, De)
    for packed in (False, True):
        got, _ = _device_run(P, dev, index_dtype, packed=packed)
        for name, a, b in zip(NAMES, got, want):
            assert_close_scaled(a, b.float(), tol=2e-5,
                                what=f'({H}, {C}, {De}) {"packed " if packed else ""}{name}')


def test_destinations_a_prefix_and_an_empty_graph(dev):
    ei = random_graph(900, 300, 5000, 43)
    P = _problem(900, 300, ei, 4, 6, 5, 7)
    P['q'] = torch.randn(900, 4, 6, generator=gen(8))       # more rows than destinations
    P['b'] = torch.randn(900, 4, 5, generator=gen(9))
    want = _reference(P, torch.float64)
    for packed in (False, True):
        got, _ = _device_run(P, dev, packed=packed)
        assert got[0].shape == (300, 4, 6) and got[1].shape == (300, 4, 5)
        assert got[3].shape == (900, 4, 6) and float(got[3][300:].abs().max()) == 0.0
        assert got[6].shape == (900, 4, 5) and float(got[6][300:].abs().max()) == 0.0
        for name, a, b in zip(NAMES, got, want):
            assert_close_scaled(a, b.float(), tol=2e-5, what=f'prefix {name}')
    # rows without slots in a graph that has edges: out_nodes = z = 0 there
    ei2 = ei[:, ei[1] % 7 != 0]
    P2 = _problem(900, 300, ei2, 4, 6, 5, 10)
    got, _ = _device_run(P2, dev)
    empty = torch.bincount(ei2[1], minlength=300) == 0
    assert int(empty.sum()) >= 40
    for t in (got[0], got[1], got[3], got[6]):
        assert float(t[:300][empty.to(t.device)].abs().max()) == 0.0
    for name, a, b in zip(NAMES, got, _reference(P2, torch.float64)):
        assert_close_scaled(a, b.float(), tol=2e-5, what=f'empty rows {name}')
    # no edges at all
    E = _problem(50, 40, torch.zeros(2, 0, dtype=torch.int64), 2, 8, 3, 9)
    for packed in (False, True):
        got, _ = _device_run(E, dev, packed=packed)
        assert got[0].shape == (40, 2, 8) and float(got[0].abs().max()) == 0.0
        assert got[1].shape == (40, 2, 3) and float(got[1].abs().max()) == 0.0
        assert got[4].shape == (50, 2, 8) and got[5].shape == (50, 2, 8)
        assert got[7].shape == (0, 3)
        assert all(float(g.abs().max()) == 0.0 for g in got[3:7])


# ---- long rows ------------------------------------------------------------------------------------
_LONG = {}


def _long_problem():
    """the graph of test_gpu_transformer._long_problem (6000 slots, threshold + 1 slots, a
    2000-slot source row) with H = 4, C = 16, De = 6"""
    if not _LONG:
        P = _problem(3000, 3000, T._long_problem()['ei'], 4, 16, 6, 53)
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
        if name in ('out_nodes', 'z', 'alpha'):
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
    assert set(info) == {'edge_forward', 'edge_backward_dst', 'backward_src'}
    chunk = _native.HUB_CHUNK
    want = -(-6000 // chunk) + -(-(_native.HUB_THRESHOLD + 1) // chunk)
    for op in ('edge_forward', 'edge_backward_dst'):
        assert info[op]['n_hub'] == 2 and info[op]['n_chunks'] == want and info[op]['De'] == 6
    assert info['backward_src']['n_hub'] == 1                  # source 7
    sink.clear()
    _device_run(P, dev, score=True)
    torch.cuda.synchronize()
    ops = [i['op'] for i, _, _ in sink if i.get('kind') == 'transformer']
    assert ops == ['edge_score', 'edge_backward_dst', 'backward_src']
    rec = [i for i, _, _ in sink if i.get('kind') == 'transformer']
    assert rec[0]['n_hub'] == 2 and rec[0]['n_chunks'] == want and rec[1]['score'] is True


def test_two_runs_are_bitwise_identical(dev):
    """No float atomics anywhere: every output and gradient, z, grad_b and grad_edge_attr
    included, repeats bit for bit, long rows included, in fused and in score mode."""
    P = _long_problem()
    for kw in (dict(), dict(packed=True), dict(score=True)):
        a, graph = _device_run(P, dev, **kw)
        P['graph'] = graph
        b, _ = _device_run(P, dev, **kw)
        for name, x, y in zip(NAMES, a, b):
            assert torch.equal(x, y), f'{kw}: {name} differs between two runs'


def test_without_a_gradient_for_edge_attr(dev, monkeypatch):
    """``edge_attr.requires_grad == False``: no grad_edge_attr is computed (the kernel is told so)
    and the other gradients are bitwise those of the run that does compute it."""
    from pytorch_geometric_amd import _native
    for P in (_uniform_case(4, 6, 7)[0], _long_problem()):
        full, _ = _device_run(P, dev)
        sink = []
        monkeypatch.setattr(_native, 'timing_sink', sink)
        lean, _ = _device_run(P, dev, edge_grad=False)
        torch.cuda.synchronize()
        monkeypatch.undo()
        rec = [i for i, _, _ in sink if i.get('op') == 'edge_backward_dst']
        assert len(rec) == 1 and rec[0]['grad_edge_attr'] is False
        assert lean[7] is None and full[7] is not None
        for name, x, y in zip(NAMES[:7], lean, full):
            assert torch.equal(x, y), f'{name} differs without grad_edge_attr'
    # through the node itself: None comes back for edge_attr
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import TransformerEdgeAttendFunction
    P = _uniform_case(4, 6, 7)[0]
    graph = as_edge_index(P['ei'].to(dev), 2000, 2000)
    q, k, v, b = [P[n].detach().to(dev).requires_grad_(True) for n in ('q', 'k', 'v', 'b')]
    a = P['a'].detach().to(dev)
    out, z = TransformerEdgeAttendFunction.apply(q, k, v, a, b, graph, 0.4, 2000)
    (out.sum() + z.sum()).backward()
    assert a.grad is None and q.grad is not None and b.grad is not None


# ---- score mode -----------------------------------------------------------------------------------
def test_score_node_agrees_with_the_fused_node(dev):
    for P in (_uniform_case(4, 6, 7)[0], _long_problem()):
        fused, _ = _device_run(P, dev)
        score, _ = _device_run(P, dev, score=True)
        for name, a, b in zip(NAMES, score, fused):
            assert_close(a, b, what=f'score vs fused {name}')


def test_dropout_in_training_runs_in_score_mode(dev, monkeypatch):
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn import TransformerConv
    torch.manual_seed(5)
    conv = TransformerConv(16, 6, heads=4, dropout=0.5, edge_dim=5).to(dev).train()
    conv.fuse_edge = True
    x = torch.randn(500, 16, generator=gen(62)).to(dev).requires_grad_(True)
    ei = random_graph(500, 500, 6000, 63).to(dev)
    ea = torch.randn(6000, 5, generator=gen(65)).to(dev).requires_grad_(True)
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    torch.manual_seed(77)
    out, (used, alpha) = conv(x, ei, ea, return_attention_weights=True)
    out.sum().backward()
    assert [i['op'] for i, _, _ in sink if i.get('kind') == 'transformer'] == \
        ['edge_score', 'edge_backward_dst', 'backward_src']
    monkeypatch.undo()
    assert torch.equal(used, ei) and alpha.shape == (6000, 4)
    # the PRE-dropout softmax, in the caller's edge order: rows sum to one, nothing was zeroed
    sums = torch.zeros(500, 4, device=dev).index_add_(0, ei[1], alpha.detach())
    has = torch.bincount(ei[1], minlength=500) > 0
    assert float((sums[has] - 1).abs().max()) <= 1e-5
    assert int((alpha == 0).sum()) == 0
    p = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
    _, want_alpha = R.conv(x.detach().cpu().double(), ei.cpu(), p, heads=4, out_channels=6,
                           edge_attr=ea.detach().cpu().double())
    assert_close_scaled(alpha, want_alpha.float(), tol=2e-5, what='returned coefficients')
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(ea.grad).all())
    # the output did see dropout, and the same seed repeats it
    torch.manual_seed(77)
    again, _ = conv(x, ei, ea, return_attention_weights=True)
    assert torch.equal(again, out)
    torch.manual_seed(78)
    other, _ = conv(x, ei, ea, return_attention_weights=True)
    assert not torch.equal(other, out)
    # eval: the score route (coefficients asked for) and the fused-edge route agree, and both
    # match float64
    conv.eval()
    names = ['x', 'edge_attr'] + [n for n, _ in conv.named_parameters()]
    leaves = [x, ea] + list(conv.parameters())
    go = torch.randn(500, 24, generator=gen(64)).to(dev)
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    a, (_, alpha_eval) = conv(x, ei, ea, return_attention_weights=False)
    b = conv(x, ei, ea)
    assert [i['op'] for i, _, _ in sink if i.get('kind') == 'transformer'] == \
        ['edge_score', 'edge_forward']
    monkeypatch.undo()
    assert_close(a, b, what='eval out')
    assert_close(alpha_eval, alpha, what='eval coefficients = training coefficients')
    x64 = x.detach().cpu().double().requires_grad_(True)
    ea64 = ea.detach().cpu().double().requires_grad_(True)
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    want, _ = R.conv(x64, ei.cpu(), p, heads=4, out_channels=6, edge_attr=ea64)
    want_g = torch.autograd.grad(want, [x64, ea64] + [p[n] for n in names[2:]], go.cpu().double())
    for n, ga, gb, gw in zip(names, torch.autograd.grad(a, leaves, go),
                             torch.autograd.grad(b, leaves, go), want_g):
        assert_close(ga, gb, what=f'eval grad {n}')
        assert_close_scaled(gb, gw.float(), tol=2e-5, what=f'eval grad {n} vs float64')
    assert_close_scaled(b, want.detach().float(), tol=2e-5, what='eval out vs float64')


# ---- nothing of size E x H*C ------------------------------------------------------------------------
def test_fused_edge_route_keeps_nothing_of_edge_times_width(dev):
    from pytorch_geometric_amd import as_edge_index
    from pytorch_geometric_amd._functions import TransformerEdgeAttendFunction
    N, E, H, C, De = 4096, 262144, 4, 32, 8
    graph = as_edge_index(random_graph(N, N, E, 71).to(dev), N, N)
    graph.fill_cache_()
    graph.src_slot_to_dst_slot()
    g = gen(72)
    q = torch.randn(N, H, C, generator=g).to(dev).requires_grad_(True)
    kv = torch.randn(N, 2, H, C, generator=g).to(dev).requires_grad_(True)
    a = torch.randn(E, De, generator=g).to(dev).requires_grad_(True)
    b = torch.randn(N, H, De, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(N, H, C, generator=g).to(dev)
    gz = torch.randn(N, H, De, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, z = TransformerEdgeAttendFunction.apply(q, kv, None, a, b, graph, 1 / math.sqrt(C), N)
    grads = torch.autograd.grad([out, z], [q, kv, a, b], [go, gz])
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'peak above the inputs: {extra / 2 ** 20:.1f} MiB')
    assert extra < E * H * C * 4 // 2                          # 64 MiB; one [E, H*C] is 128 MiB
    assert all(bool(torch.isfinite(t).all()) for t in grads)


# ---- routing --------------------------------------------------------------------------------------------
def test_routing_with_fuse_edge(dev, monkeypatch):
    """An unsupported De, target_to_source, H*C = 1024 and host tensors take the generic or the
    host route with ``fuse_edge = True``, and match float64; a supported layer takes the new one."""
    from pytorch_geometric_amd.nn import TransformerConv
    ei = random_graph(300, 300, 3000, 91)
    x = torch.randn(300, 16, generator=gen(92))
    for what, kw, De, device in (
            ('De = 5 at H = 64', dict(heads=64, out_channels=2, edge_dim=5), 5, dev),
            ('target_to_source', dict(heads=2, out_channels=8, edge_dim=3,
                                      flow='target_to_source'), 3, dev),
            ('H*C = 1024', dict(heads=8, out_channels=128, edge_dim=3), 3, dev),
            ('host tensors', dict(heads=2, out_channels=8, edge_dim=3), 3, 'cpu'),
            ('supported', dict(heads=2, out_channels=8, edge_dim=3), 3, dev)):
        ea = torch.randn(3000, De, generator=gen(93))
        torch.manual_seed(9)
        conv = TransformerConv(16, **kw).to(device)
        conv.fuse_edge = True
        xd = x.detach().to(device).requires_grad_(True)
        ead = ea.detach().to(device).requires_grad_(True)
        state = {}

        def step():
            state['out'] = conv(xd, ei.to(device), edge_attr=ead)
            state['grad'] = torch.autograd.grad(state['out'].sum(), [xd, ead])

        c = T._counted(monkeypatch, step)
        fused = [n for n in c.calls if 'transformer_edge_forward' in n
                 or 'transformer_edge_backward' in n or 'transformer_forward' in n
                 or 'transformer_backward' in n]
        if what == 'supported':
            assert sorted(fused) == ['pygamd_transformer_backward_src',
                                     'pygamd_transformer_edge_backward_dst',
                                     'pygamd_transformer_edge_forward'], c.calls
        else:
            assert not fused, (what, c.calls)
        p = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
        x64, ea64 = x.double().requires_grad_(True), ea.double().requires_grad_(True)
        flipped = kw.get('flow') == 'target_to_source'     # the roles of the two rows swap
        want, _ = R.conv(x64, ei.flip(0) if flipped else ei, p, edge_attr=ea64,
                         **{k: v for k, v in kw.items() if k != 'flow'})
        assert_close_scaled(state['out'], want.detach().float(), tol=2e-5, what=f'{what} out')
        for n, g, w in zip(('grad_x', 'grad_edge_attr'), state['grad'],
                           torch.autograd.grad(want.sum(), [x64, ea64])):
            assert_close_scaled(g, w.float(), tol=2e-5, what=f'{what} {n}')
    # the switch is per layer and off by default: the same layer without it stays generic
    conv.fuse_edge = False
    c = T._counted(monkeypatch, lambda: conv(x.to(dev), ei.to(dev), ea.to(dev)))
    assert not [n for n in c.calls if 'transformer_edge' in n], c.calls


def test_half_inputs_are_widened(dev):
    from pytorch_geometric_amd.nn import TransformerConv
    torch.manual_seed(4)
    conv = TransformerConv(16, 8, heads=2, beta=True, edge_dim=4).to(dev)
    conv.fuse_edge = True
    x = torch.randn(300, 16, generator=gen(94)).to(dev)
    ei = random_graph(300, 300, 3000, 95).to(dev)
    ea = torch.randn(3000, 4, generator=gen(98)).to(dev)
    want = conv(x, ei, ea)
    got = conv.half()(x.half(), ei, ea.half())
    assert got.dtype == torch.float16
    assert_close_scaled(got.float(), want, tol=2e-2, what='half')


def test_inside_hetero_conv_with_edge_attr_dict(dev, monkeypatch):
    from pytorch_geometric_amd.nn import HeteroConv, TransformerConv
    torch.manual_seed(6)
    layer = TransformerConv((16, 12), 8, heads=2, edge_dim=3)
    layer.fuse_edge = True
    hetero = HeteroConv({('a', 'to', 'b'): layer}).to(dev)
    g = gen(96)
    x_a, x_b = torch.randn(400, 16, generator=g), torch.randn(150, 12, generator=g)
    ei = random_graph(400, 150, 2500, 97)
    ea = torch.randn(2500, 3, generator=g)
    xa, xb = x_a.to(dev).requires_grad_(True), x_b.to(dev).requires_grad_(True)
    ead = ea.to(dev).requires_grad_(True)
    state = {}

    def step():
        state['out'] = hetero({'a': xa, 'b': xb}, {('a', 'to', 'b'): ei.to(dev)},
                              edge_attr_dict={('a', 'to', 'b'): ead})

    c = T._counted(monkeypatch, step)
    assert c.calls.get('pygamd_transformer_edge_forward') == 1, c.calls
    out = state['out']
    assert set(out) == {'b'} and out['b'].shape == (150, 16)
    grads = torch.autograd.grad(out['b'].sum(), [xa, xb, ead])
    p = {k: v.detach().cpu().double() for k, v in layer.state_dict().items()}
    leaves = [t.double().requires_grad_(True) for t in (x_a, x_b, ea)]
    want, _ = R.conv((leaves[0], leaves[1]), ei, p, heads=2, out_channels=8, edge_attr=leaves[2])
    assert_close_scaled(out['b'], want.detach().float(), tol=2e-5, what='hetero out')
    for name, got, ref in zip(('grad a', 'grad b', 'grad edge_attr'), grads,
                              torch.autograd.grad(want.sum(), leaves)):
        assert_close_scaled(got, ref.float(), tol=2e-5, what=f'hetero {name}')


# ---- the registered operator ------------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'transformer_edge_attend' in ops.OPS and 'transformer_edge_attend_backward' in ops.OPS
    op = torch.ops.pyg_amd.transformer_edge_attend
    with FakeTensorMode():
        q = torch.empty(12, 4, 8, device='cuda', requires_grad=True)
        k = torch.empty(50, 4, 8, device='cuda')
        v = torch.empty(50, 4, 8, device='cuda')
        a = torch.empty(400, 5, device='cuda')
        b = torch.empty(12, 4, 5, device='cuda')
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        out, z, alpha = op(q, k, v, a, b, ptr, col, 0.35)
        assert out.shape == (12, 4, 8) and z.shape == (12, 4, 5) and alpha.shape == (400, 4)
        assert out.requires_grad and out.device.type == 'cuda' and out.dtype == torch.float32

    P, want = _uniform_case(4, 6, 7)
    order = torch.argsort(P['ei'][1], stable=True)
    col = P['ei'][0][order].to(dev)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], 2000).to(dev)
    go, gz = P['go'].to(dev), P['gz'].to(dev)
    scale = 1 / math.sqrt(6)
    a_slot = P['a'][order]                                  # the operator's edge order is col's

    def fn(q, k, v, a, b):
        out, z, _ = op(q * 1.0, k, v, a, b, ptr, col, scale)
        return (out * go).sum() + (z * gz).sum()

    def leaves():
        return [P[n].detach().to(dev).requires_grad_(True) for n in ('q', 'k', 'v')] + \
            [a_slot.to(dev).requires_grad_(True), P['b'].detach().to(dev).requires_grad_(True)]

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        y = f(*ls)
        results.append([y.detach()] + list(torch.autograd.grad(y, ls)))
    for x, y in zip(*results):
        assert_close(y, x, what='compiled vs eager')
    g_q, g_k, g_v, g_a, g_b = results[0][1:]
    for name, x, y in zip(NAMES[3:], (g_q, g_k, g_v, g_b, g_a),
                          want[3:7] + [want[7][order]]):
        assert_close_scaled(x, y.float(), tol=2e-5, what=f'operator {name}')
    out, z, alpha = op(*[t.detach() for t in leaves()], ptr, col, scale)
    assert_close_scaled(out, want[0].float(), tol=2e-5, what='operator out')
    assert_close_scaled(z, want[1].float(), tol=2e-5, what='operator z')
    assert_close_scaled(alpha, want[2][order].float(), tol=2e-5, what='operator alpha')
    torch.library.opcheck(op, (*leaves(), ptr, col, scale))
