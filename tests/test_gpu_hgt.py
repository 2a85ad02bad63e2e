"""nn.HGTConv on the device: the recorded reference cases on the fused and the generic route, the
relation-transform kernels (csrc/hgt.hip) against the float64 restatement (tests/_hgt_ref.py) at
the smallest shapes that reach every path, bitwise repeatability, a hub destination fed by two edge
types, the launch structure, the memory promise, a sampled typed batch, routing and the registered
operator.  Nothing here reads the reference tree: the golden file is the only thing taken from
it."""
import ctypes

import pytest
import torch

import _hgt_ref as R
from _util import _call_counts as _counted
from _util import assert_close, assert_close_scaled, gen, random_graph

pytestmark = pytest.mark.gpu

CASES = ['three_types', 'skip', 'shared', 'empty_missing', 'source_only', 'heads1', 'd5']


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('fuse', [True, False])
@pytest.mark.parametrize('name', CASES)
def test_golden_cases(dev, name, fuse, index_dtype):
    R.check_class_case(R.load_golden(), name, dev, fuse=fuse, index_dtype=index_dtype)


# ---- the relation kernels against float64 ------------------------------------------------------------
# five node types with 257, 63, 65, 1 and 0 rows (partial 128-row workgroups and 16-row tiles, an
# empty edge type); three edge types read node type 0 (the accumulation order of its input
# gradient); nine edge types in the metadata, seven in the call, in no particular metadata order
SIZES = [257, 63, 65, 1, 0]
SRC_POS = [0, 1, 0, 2, 3, 0, 4]
WIDX = [5, 0, 7, 2, 8, 3, 1]
T_META = 9
_REF = {}


def _relation_problem(H, D, seed=11, sizes=SIZES, src_pos=SRC_POS, widx=WIDX, T=T_META):
    g = gen(seed + 100 * H + D)
    F = H * D
    S = sum(sizes[p] for p in src_pos)
    return {'kqv': [torch.randn(n, 3 * F, generator=g) for n in sizes],
            'wk': torch.randn(H * T, D, D, generator=g) / D ** 0.5,
            'wv': torch.randn(H * T, D, D, generator=g) / D ** 0.5,
            'go': torch.randn(S, 2 * F, generator=g), 'H': H, 'D': D, 'src_pos': src_pos,
            'widx': widx}


def _relation_reference(P):
    """(kv, grad_wk, grad_wv, grad_kqv...) in float64, computed once per problem."""
    key = id(P)
    if key not in _REF:
        H, F = P['H'], P['H'] * P['D']
        kqv = [x.double().requires_grad_(True) for x in P['kqv']]
        wk, wv = P['wk'].double().requires_grad_(True), P['wv'].double().requires_grad_(True)
        kv = R.relation([kqv[p][:, :F] for p in P['src_pos']],
                        [kqv[p][:, 2 * F:] for p in P['src_pos']], P['widx'], wk, wv, H)
        grads = torch.autograd.grad(kv, [wk, wv] + kqv, P['go'].double())
        _REF[key] = [kv.detach()] + [g.detach() for g in grads]
    return _REF[key]


def _relation_device(P, dev, strided=True):
    """The same list from the device.  ``strided``: through the autograd node, the rows read in
    place from the [N, 3F] projections; otherwise through the wrappers on contiguous [N, F]
    tensors, with contiguous gradient blocks."""
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd._functions import HgtRelationPlan, HGTRelationFunction
    H, D = P['H'], P['D']
    F = H * D
    wk, wv = P['wk'].to(dev), P['wv'].to(dev)
    go = P['go'].to(dev)
    if strided:
        kqv = [x.to(dev).requires_grad_(True) for x in P['kqv']]
        wk, wv = wk.requires_grad_(True), wv.requires_grad_(True)
        plan = HgtRelationPlan(H, P['src_pos'], P['widx'])
        kv = HGTRelationFunction.apply(plan, wk, wv, *kqv)
        grads = torch.autograd.grad(kv, [wk, wv] + kqv, go)
        return [kv.detach()] + list(grads)
    k = [x[:, :F].contiguous().to(dev) for x in P['kqv']]
    v = [x[:, 2 * F:].contiguous().to(dev) for x in P['kqv']]
    ks, vs = [k[p] for p in P['src_pos']], [v[p] for p in P['src_pos']]
    kv = _native.hgt_relation_forward(ks, vs, P['widx'], wk, wv, H, D)
    gk, gv = [torch.empty_like(x) for x in k], [torch.empty_like(x) for x in v]
    g_wk, g_wv = _native.hgt_relation_backward(ks, vs, P['widx'], P['src_pos'], wk, wv, H, D, go,
                                               gk, gv)
    full = [torch.cat([a, torch.zeros_like(a), b], dim=1) for a, b in zip(gk, gv)]
    return [kv, g_wk, g_wv] + full


def _names(P):
    return ['kv', 'grad_wk', 'grad_wv'] + [f'grad_kqv[{t}]' for t in range(len(P['kqv']))]


_PROBLEMS = {}


def _problem(H, D):
    if (H, D) not in _PROBLEMS:
        _PROBLEMS[(H, D)] = _relation_problem(H, D)
    return _PROBLEMS[(H, D)]


@pytest.mark.parametrize('strided', [True, False])
@pytest.mark.parametrize('H,D', [(1, 5), (3, 8), (4, 16), (2, 32), (8, 64), (4, 128), (1, 128)])
def test_relation_kernels_match_float64(dev, H, D, strided):
    P = _problem(H, D)
    want = _relation_reference(P)
    got = _relation_device(P, dev, strided=strided)
    assert got[0].shape == (sum(SIZES[p] for p in SRC_POS), 2 * H * D)
    for name, a, w in zip(_names(P), got, want):
        assert_close_scaled(a, w.float(), tol=2e-5, what=f'H={H} D={D} {name}')
    # the matrices of the two edge types that are not in the call take no gradient: exact zeros
    T = T_META
    absent = sorted(set(range(T)) - set(WIDX))
    for g in got[1:3]:
        assert not bool(g.view(H, T, D, D)[:, absent].any())


def test_sixty_four_edge_types_in_one_call_and_sixty_five_refused(dev):
    from pytorch_geometric_amd import _lib, _native
    from pytorch_geometric_amd._lib import PygAmdError
    H, D, T = 2, 8, 64
    sizes = [33, 70]
    src_pos = [e % 2 for e in range(64)]
    widx = [(7 * e + 3) % 64 for e in range(64)]               # a permutation of 0..63
    P = _relation_problem(H, D, seed=23, sizes=sizes, src_pos=src_pos, widx=widx, T=T)
    want = _relation_reference(P)
    for strided in (True, False):
        got = _relation_device(P, dev, strided=strided)
        for name, a, w in zip(_names(P), got, want):
            assert_close_scaled(a, w.float(), tol=2e-5, what=f'64 edge types {name}')
    # 65: the wrapper refuses, and so does the entry point itself (status 2, before any device work)
    F = H * D
    k = [torch.zeros(4, F, device=dev) for _ in range(65)]
    w = torch.zeros(H * 65, D, D, device=dev)
    with pytest.raises(PygAmdError, match='at most 64 edge types'):
        _native.hgt_relation_forward(k, k, list(range(65)), w, w, H, D)
    lib = _lib.load()
    table = (ctypes.c_int64 * (4 * 65))(*[v for e in range(65) for v in (F, 4, e, 0)])
    ptrs = (ctypes.c_void_p * 65)(*[t.data_ptr() for t in k])
    kv = torch.zeros(65 * 4, 2 * F, device=dev)
    assert lib.pygamd_hgt_relation_forward(ptrs, ptrs, table, 65, w.data_ptr(), w.data_ptr(), 65,
                                           H, D, kv.data_ptr(), None) == 2
    nbytes = ctypes.c_size_t(0)
    assert lib.pygamd_hgt_workspace_bytes(table, 65, H, D, ctypes.byref(nbytes)) == 2
    # a head layout outside the supported set: status 2 as well
    assert not _native.hgt_supported(1, 129) and not _native.hgt_supported(65, 4)
    assert _native.hgt_supported(4, 128) and not _native.hgt_supported(8, 128)
    assert lib.pygamd_hgt_relation_forward(ptrs, ptrs, table, 2, w.data_ptr(), w.data_ptr(), 65,
                                           1, 129, kv.data_ptr(), None) == 2
    # one edge type named twice: status 1
    twice = (ctypes.c_int64 * 8)(F, 4, 3, 0, F, 4, 3, 0)
    assert lib.pygamd_hgt_relation_forward(ptrs, ptrs, twice, 2, w.data_ptr(), w.data_ptr(), 65,
                                           H, D, kv.data_ptr(), None) == 1


def test_two_backward_runs_are_bitwise_identical(dev):
    """No float atomics: partial weight gradients are reduced in chunk order, the input gradients
    accumulate over the edge types in call order."""
    P = _problem(2, 32)
    a = _relation_device(P, dev)
    b = _relation_device(P, dev)
    for name, x, y in zip(_names(P), a, b):
        assert torch.equal(x, y), f'{name} differs between two runs'


# ---- the class against the float64 restatement ------------------------------------------------------
def _layer_and_reference(kwargs, x_dict, ei_dict, dev, seed=3, **layer_kw):
    """(layer on the device with random skip / p_rel, float64 outputs, float64 gradient of
    sum(out * go) with respect to the inputs and the parameters, go)"""
    from pytorch_geometric_amd.nn import HGTConv
    torch.manual_seed(seed)
    layer = HGTConv(**kwargs, **layer_kw)
    with torch.no_grad():
        for p in list(layer.skip.values()) + list(layer.p_rel.values()):
            p.copy_(torch.randn(p.shape, generator=gen(seed + 1)))
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    x64 = {t: v.double().requires_grad_(True) for t, v in x_dict.items()}
    want = R.conv(x64, ei_dict, p64, **kwargs)
    go = {t: torch.randn(v.shape, generator=gen(seed + 2)) for t, v in want.items()}
    loss = sum((want[t] * go[t].double()).sum() for t in want)
    grads = torch.autograd.grad(loss, list(x64.values()) + list(p64.values()), allow_unused=True)
    g_x = dict(zip(x64, grads[:len(x64)]))
    g_p = dict(zip(p64, grads[len(x64):]))
    return layer.to(dev), {t: v.detach() for t, v in want.items()}, g_x, g_p, go


def _check_layer(layer, x_dict, ei_dict, want, g_x, g_p, go, dev, what, tol=2e-5):
    xs = {t: v.to(dev).requires_grad_(True) for t, v in x_dict.items()}
    out = layer(xs, {et: ei.to(dev) for et, ei in ei_dict.items()})
    assert list(out) == list(want), what
    params = list(layer.named_parameters())
    loss = sum((out[t] * go[t].to(dev)).sum() for t in out)
    grads = torch.autograd.grad(loss, list(xs.values()) + [p for _, p in params],
                                allow_unused=True)
    for t in out:
        assert_close_scaled(out[t], want[t].float(), tol=tol, what=f'{what} out[{t}]')
    for t, g in zip(xs, grads):
        ref = g_x[t]
        assert_close_scaled(g, torch.zeros_like(g) if ref is None else ref.float(), tol=tol,
                            what=f'{what} grad_x[{t}]')
    for (n, _), g in zip(params, grads[len(xs):]):
        ref = g_p[n]
        if ref is None:
            assert g is None or not bool(g.any()), f'{what}: unexpected gradient for {n}'
        else:
            assert_close_scaled(g, ref.float(), tol=tol, what=f'{what} grad {n}')


AB, AB2, BA = ('a', 'r1', 'b'), ('a', 'r2', 'b'), ('b', 'r3', 'a')


def test_hub_destination_fed_by_two_edge_types(dev, monkeypatch):
    """Destination b[3] has 800 + 700 incoming slots, spread over two edge types: more than the hub
    threshold, so the stacked row takes the attention kernels' chunked schedule."""
    from pytorch_geometric_amd import _native
    assert 800 + 700 > _native.HUB_THRESHOLD
    g = gen(31)
    sizes = {'a': 1500, 'b': 40}
    x = {'a': torch.randn(1500, 12, generator=g), 'b': torch.randn(40, 20, generator=g)}

    def to_hub(n_hub, n_rest, seed):
        ei = random_graph(1500, 40, n_hub + n_rest, seed)
        ei[1, :n_hub] = 3
        return ei

    ei = {AB: to_hub(800, 300, 32), AB2: to_hub(700, 200, 33), BA: random_graph(40, 1500, 900, 34)}
    kwargs = dict(in_channels={'a': 12, 'b': 20}, out_channels=16,
                  metadata=(list(sizes), [AB, AB2, BA]), heads=2)
    layer, want, g_x, g_p, go = _layer_and_reference(kwargs, x, ei, dev)
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    _check_layer(layer, x, ei, want, g_x, g_p, go, dev, 'hub')
    info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'transformer'}
    assert info['forward']['n_hub'] >= 1 and info['forward']['n_chunks'] >= 1500 // _native.HUB_CHUNK
    assert [i['op'] for i, _, _ in sink if i.get('kind') == 'hgt'] == ['relation_forward',
                                                                      'relation_backward']


# ---- launch structure ---------------------------------------------------------------------------------
def _split_graph(dev, parts):
    base = {('a', 'b'): random_graph(3000, 2000, 24000, 90), ('b', 'a'): random_graph(2000, 3000,
                                                                                    24000, 91)}
    ei = {}
    for (s, d), full in base.items():
        for p, chunk in enumerate(full.chunk(parts, dim=1)):
            ei[(s, f'r{p}', d)] = chunk.contiguous().to(dev)
    return ei


def test_launch_structure_does_not_depend_on_the_number_of_edge_types(dev, monkeypatch):
    from pytorch_geometric_amd.nn import HGTConv
    g = gen(92)
    x = {'a': torch.randn(3000, 32, generator=g).to(dev),
         'b': torch.randn(2000, 32, generator=g).to(dev)}
    once = ('pygamd_hgt_relation_forward', 'pygamd_hgt_relation_backward',
            'pygamd_transformer_forward', 'pygamd_transformer_backward_dst',
            'pygamd_transformer_backward_src')
    calls = {}
    for parts in (1, 4):
        ei = _split_graph(dev, parts)
        torch.manual_seed(parts)
        layer = HGTConv(32, 32, (['a', 'b'], list(ei)), heads=2).to(dev)
        xs = {t: v.clone().requires_grad_(True) for t, v in x.items()}

        def step():
            out = layer(xs, ei)
            sum(v.sum() for v in out.values()).backward()

        calls[parts] = _counted(monkeypatch, step)
        assert len(ei) == 2 * parts
        for name in once:
            assert calls[parts].get(name) == 1, (parts, name, calls[parts])
        assert not [n for n in calls[parts] if 'spmm' in n or 'softmax' in n or 'segment' in n], \
            calls[parts]
    assert calls[1] == calls[4], (calls[1], calls[4])

    # three layers on one batch share one stacked handle: it is sorted by destination once and by
    # source once
    ei = _split_graph(dev, 2)
    layers = [HGTConv(32, 32, (['a', 'b'], list(ei)), heads=2).to(dev) for _ in range(3)]
    xs = {t: v.clone().requires_grad_(True) for t, v in x.items()}

    def model_step():
        h = xs
        for layer in layers:
            h = layer(h, ei)
        sum(v.sum() for v in h.values()).backward()

    c = _counted(monkeypatch, model_step)
    assert c['pygamd_index_sort'] == 2, c
    assert c['pygamd_hgt_relation_forward'] == 3 and c['pygamd_transformer_backward_src'] == 3


# ---- the memory promise --------------------------------------------------------------------------------
def test_fused_route_keeps_nothing_of_edge_times_width(dev):
    """3 node types x 2,000 nodes, 1 M edges, F = 64, H = 2.  The fused route's edge-sized tensors
    are alpha and grad_s, 2 * E * H * 4 bytes = 16 MB; every node-sized tensor together (the
    stacked source table has 4 x 2,000 rows) is far below 100 MB; one [E, F] float32 tensor is
    256 MB, and the generic route holds several."""
    from pytorch_geometric_amd.nn import HGTConv
    N, E, F, H = 2000, 1_000_000, 64, 2
    ets = [('a', 'r0', 'b'), ('b', 'r1', 'c'), ('c', 'r2', 'a'), ('a', 'r3', 'a')]
    g = gen(70)
    x = {t: torch.randn(N, F, generator=g).to(dev).requires_grad_(True) for t in 'abc'}
    ei = {et: random_graph(N, N, E // 4, 71 + k).to(dev) for k, et in enumerate(ets)}
    torch.manual_seed(7)
    layer = HGTConv(F, F, (list('abc'), ets), heads=H).to(dev)

    def step():
        out = layer(x, ei)
        sum(v.sum() for v in out.values()).backward()

    def peak():
        for t in list(x.values()) + list(layer.parameters()):
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    step()                                                     # warm-up: the handle is cached
    fused = peak()
    print(f'fused: peak above the level before {fused / 2 ** 20:.1f} MiB')
    assert fused < E * F * 4
    layer.fuse = False
    step()
    generic = peak()
    print(f'generic: {generic / 2 ** 20:.1f} MiB')
    assert generic > E * F * 4
    assert all(bool(torch.isfinite(v.grad).all()) for v in x.values())


# ---- a sampled typed batch -------------------------------------------------------------------------------
def test_two_layers_on_a_sampled_batch(dev):
    from pytorch_geometric_amd.loader import HeteroNeighborLoader
    from pytorch_geometric_amd.nn import HGTConv
    num_nodes = {'u': 3000, 'i': 1500, 't': 200}
    widths = {'u': 12, 'i': 20, 't': 6}
    ets = [('u', 'buys', 'i'), ('i', 'bought_by', 'u'), ('u', 'follows', 'u'), ('i', 'has', 't')]
    g = gen(80)
    x_full = {t: torch.randn(n, widths[t], generator=g).to(dev) for t, n in num_nodes.items()}
    ei_full = {et: random_graph(num_nodes[et[0]], num_nodes[et[-1]], 12000, 81 + k).to(dev)
               for k, et in enumerate(ets)}
    loader = HeteroNeighborLoader(x_full, ei_full, [4, 4], 'u', batch_size=64, seed=5)
    batch = next(iter(loader))
    x = {t: v.cpu() for t, v in batch.x_dict.items()}
    ei = {et: v.cpu().long() for et, v in batch.edge_index_dict.items()}
    # 't' is never a source: no hop reaches it from the 'u' seeds
    assert x['t'].size(0) == 0 and any(v.size(1) == 0 for v in ei.values())
    meta = (list(num_nodes), ets)
    torch.manual_seed(8)
    layers = [HGTConv(widths, 16, meta, heads=2), HGTConv(16, 16, meta, heads=4)]
    for layer in layers:
        with torch.no_grad():
            for p in list(layer.skip.values()) + list(layer.p_rel.values()):
                p.copy_(torch.randn(p.shape, generator=g))
    # float64 restatement of the model: loss = sum of the seed rows of 'u' times a fixed tensor
    states = [{k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
              for m in layers]
    h = {t: v.double() for t, v in x.items()}
    h = R.conv(h, ei, states[0], out_channels=16, metadata=meta, heads=2)
    h = R.conv(h, ei, states[1], out_channels=16, metadata=meta, heads=4)
    go = torch.randn(64, 16, generator=g)
    want = h['u'][:64]
    leaves = [v for s in states for v in s.values()]
    ref = torch.autograd.grad((want * go.double()).sum(), leaves, allow_unused=True)

    layers = [m.to(dev) for m in layers]
    hd = layers[0](batch.x_dict, batch.edge_index_dict)
    hd = layers[1](hd, batch.edge_index_dict)
    got = hd['u'][:64]
    params = [p for m in layers for p in m.parameters()]
    grads = torch.autograd.grad((got * go.to(dev)).sum(), params, allow_unused=True)
    assert_close(got, want.detach().float(), what='sampled out')
    names = [f'{i}.{n}' for i, m in enumerate(layers) for n, _ in m.named_parameters()]
    assert len(names) == len(ref)
    for n, a, w in zip(names, grads, ref):
        if w is None:
            assert a is None or not bool(a.any()), n
        else:
            assert_close(a, w.float(), atol=5e-5, rtol=5e-5, what=f'sampled grad {n}')


# ---- routing ------------------------------------------------------------------------------------------------
def _routing_inputs():
    g = gen(60)
    x = {'a': torch.randn(300, 16, generator=g), 'b': torch.randn(200, 16, generator=g)}
    ei = {AB: random_graph(300, 200, 2000, 61), AB2: random_graph(300, 200, 1500, 62),
          BA: random_graph(200, 300, 1800, 63)}
    return x, ei, (['a', 'b'], [AB, AB2, BA])


@pytest.mark.parametrize('what', ['D = 256', 'fuse off', 'target_to_source', 'message hook'])
def test_routing_to_the_generic_route(dev, monkeypatch, what):
    x, ei, meta = _routing_inputs()
    kwargs = dict(in_channels=16, out_channels=256 if what == 'D = 256' else 16, metadata=meta,
                  heads=1 if what == 'D = 256' else 2)
    layer_kw = {'flow': 'target_to_source'} if what == 'target_to_source' else {}
    layer, want, g_x, g_p, go = _layer_and_reference(kwargs, x, ei, dev, seed=9, **layer_kw)
    if what == 'fuse off':
        layer.fuse = False
    seen = []
    if what == 'message hook':
        layer.register_message_forward_hook(lambda mod, args, out: seen.append(tuple(out.shape)))
    c = _counted(monkeypatch, lambda: _check_layer(layer, x, ei, want, g_x, g_p, go, dev, what))
    assert not [n for n in c if 'hgt_relation' in n or 'transformer_forward' in n], (what, c)
    if what == 'message hook':
        assert seen == [(5300, 2, 8)]                          # [E, H, D] messages exist here


def test_half_inputs_take_the_generic_route(dev, monkeypatch):
    from pytorch_geometric_amd.nn import HGTConv
    x, ei, meta = _routing_inputs()
    torch.manual_seed(4)
    layer = HGTConv(16, 16, meta, heads=2).to(dev)
    xd = {t: v.to(dev) for t, v in x.items()}
    eid = {et: v.to(dev) for et, v in ei.items()}
    c = _counted(monkeypatch, lambda: layer(xd, eid))
    assert c.get('pygamd_hgt_relation_forward') == 1           # what a plain layer takes
    want = layer(xd, eid)
    layer = layer.half()
    state = {}
    c = _counted(monkeypatch, lambda: state.update(
        out=layer({t: v.half() for t, v in xd.items()}, eid)))
    assert not [n for n in c if 'hgt_relation' in n or 'transformer_forward' in n], c
    for t in want:
        assert state['out'][t].dtype == torch.float16
        assert_close_scaled(state['out'][t].float(), want[t], tol=2e-2, what=f'half {t}')


# ---- the registered operator ----------------------------------------------------------------------------
def test_operator_equals_the_autograd_node_and_has_a_fake_kernel(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'hgt_relation' in ops.OPS and 'hgt_relation_backward' in ops.OPS
    op = torch.ops.pyg_amd.hgt_relation
    with FakeTensorMode():
        kqv = [torch.empty(50, 3 * 24, device='cuda', requires_grad=True),
               torch.empty(7, 3 * 24, device='cuda')]
        w = torch.empty(4 * 5, 6, 6, device='cuda')
        kv = op(kqv, w, w, [0, 1, 0], [4, 0, 2], 4)
        assert kv.shape == (50 + 7 + 50, 2 * 24) and kv.requires_grad
        assert kv.device.type == 'cuda' and kv.dtype == torch.float32
        g_x, g_wk, g_wv = torch.ops.pyg_amd.hgt_relation_backward(
            torch.empty(107, 48, device='cuda'), kqv, w, w, [0, 1, 0], [4, 0, 2], 4)
        assert [t.shape for t in g_x] == [(50, 72), (7, 72)] and g_wk.shape == g_wv.shape == w.shape

    P = _problem(3, 8)
    want = _relation_device(P, dev)                            # the autograd node
    go = P['go'].to(dev)

    def fn(wk, wv, *kqv):
        return (op([t * 1.0 for t in kqv], wk, wv, P['src_pos'], P['widx'], 3) * go).sum()

    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        leaves = [P['wk'].to(dev).requires_grad_(True), P['wv'].to(dev).requires_grad_(True)] \
            + [x.to(dev).requires_grad_(True) for x in P['kqv']]
        grads = torch.autograd.grad(f(*leaves), leaves)
        for name, a, w in zip(_names(P)[1:], grads, want[1:]):
            assert torch.equal(a, w), f'operator vs node: {name}'
    kv = op([x.to(dev) for x in P['kqv']], P['wk'].to(dev), P['wv'].to(dev), P['src_pos'],
            P['widx'], 3)
    assert torch.equal(kv, want[0])
