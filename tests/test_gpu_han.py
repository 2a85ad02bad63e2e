"""nn.HANConv on the device: the recorded reference cases on the fused and the generic route, the
typed additive-attention kernels (csrc/han.hip) against the float64 restatement (tests/_han_ref.py)
at the smallest shapes that reach every path, long rows in both directions, bitwise repeatability,
the non-finite rules, the edge-type limit, the launch structure, the memory promise, routing, a
sampled typed batch and the registered operator.  Nothing here reads the reference tree: the golden
file is the only thing taken from it.  Comparisons are at ``assert_close_scaled(tol=2e-5)`` over
every element unless a test says otherwise."""
import copy
import functools

import pytest
import torch

import _han_ref as R
from _util import _call_counts as _counted
from _util import assert_close_scaled, assert_sum_close, gen, random_graph

pytestmark = pytest.mark.gpu

CASES = ['three_types', 'shared', 'empty_missing', 'source_only', 'heads1', 'd5', 'no_venue_rows']
HAN_CALLS = ('pygamd_han_forward', 'pygamd_han_backward_dst', 'pygamd_han_backward_src')


# ---- 1. the recorded cases ---------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('fuse', [True, False])
@pytest.mark.parametrize('name', CASES)
def test_golden_cases(dev, monkeypatch, name, fuse, index_dtype):
    G = R.load_golden()
    c = _counted(monkeypatch, lambda: R.check_class_case(
        G, name, dev, functools.partial(assert_close_scaled, tol=2e-5), fuse=fuse,
        index_dtype=index_dtype))
    assert c.get('pygamd_han_forward', 0) == (1 if fuse else 0), c


# ---- 2. the kernels against float64 ------------------------------------------------------------------
# five node types with 257, 63, 65, 1 and 0 rows; seven edge types in no metadata order: two share
# source and destination type, one has no edges, one ends in the type without rows; node type 0
# feeds three edge types (one copy of its rows, three column blocks)
SIZES = {'n0': 257, 'n1': 63, 'n2': 65, 'n3': 1, 'n4': 0}
EDGES = [(('n0', 'r5', 'n1'), 900), (('n2', 'r0', 'n0'), 1200), (('n0', 'r7', 'n1'), 500),
         (('n1', 'r2', 'n2'), 0), (('n3', 'r8', 'n0'), 300), (('n0', 'r3', 'n4'), 0),
         (('n1', 'r1', 'n0'), 700)]
GRID = [(1, 5), (3, 5), (4, 6), (2, 32), (8, 32), (4, 128), (64, 1)]
# seeds at which every LeakyReLU argument keeps 1e-6 * max|arg| from 0 (asserted below)
SEEDS = {(1, 5): 12, (3, 5): 12, (4, 6): 11, (2, 32): 11, (8, 32): 11, (4, 128): 11, (64, 1): 11}
SLOPE = 0.2


def _typed_problem(H, D, seed, sizes=SIZES, edges=EDGES, ei=None, sort_dst=False):
    """Inputs of one attention step on a stacked typed graph, float32 on the host."""
    from pytorch_geometric_amd import _han
    g = gen(seed + 100 * H + D)
    ets = [et for et, _ in edges]
    if ei is None:
        ei = [random_graph(sizes[et[0]], max(sizes[et[-1]], 1), e, seed + k, skew=True)
              for k, (et, e) in enumerate(edges)]
    if sort_dst:   # every edge list, and so the stacked one, sorted by destination
        ei = [e[:, e[1].sort(stable=True).indices] for e in ei]
    st = _han.Stacking(sizes, ets)
    stacked = _han.build_stacked(st, ei).edge_index
    P = {'H': H, 'D': D, 'st': st, 'ei': ei, 'col': stacked[0], 'row': stacked[1],
         'x': torch.randn(st.num_nodes, H, D, generator=g),
         'a_src': torch.randn(st.num_cols, H, generator=g),
         'a_dst': torch.randn(st.num_rows, H, generator=g),
         'go': torch.randn(st.num_rows, H * D, generator=g)}
    pre = P['a_src'][P['col']] + P['a_dst'][P['row']]
    P['leaky_margin'] = float(pre.abs().min() / pre.abs().max()) if pre.numel() else 1.0
    return P


def _reference(P, relu, mask=None, dtype=torch.float64):
    """(out, alpha in edge order, grad_x, grad_a_src, grad_a_dst) of the restatement"""
    leaves = [P[k].to(dtype).requires_grad_(True) for k in ('x', 'a_src', 'a_dst')]
    out, alpha = R.attend(*leaves, P['col'], P['row'], P['st'].types, SLOPE, relu=relu, mask=mask)
    grads = torch.autograd.grad(out, leaves, P['go'].to(dtype))
    return (out.detach(), alpha.detach()) + grads


def _device(P, dev, relu, sink=None, monkeypatch=None):
    """The autograd node on the device: (out, alpha in slot order, grads..., the handle)"""
    from pytorch_geometric_amd import _han, _native
    from pytorch_geometric_amd._functions import HanAttendFunction
    graph = _han.build_stacked(P['st'], [e.to(dev) for e in P['ei']])
    leaves = [P[k].to(dev).requires_grad_(True) for k in ('x', 'a_src', 'a_dst')]
    if sink is not None:
        monkeypatch.setattr(_native, 'timing_sink', sink)
    out, alpha = HanAttendFunction.apply(*leaves, graph, P['st'].types, SLOPE, relu)
    grads = torch.autograd.grad(out, leaves, P['go'].to(dev))
    torch.cuda.synchronize()
    if sink is not None:
        monkeypatch.undo()
    return (out.detach(), alpha.detach()) + grads + (graph, )


def _check(got, want, what, names=('out', 'alpha', 'grad_x', 'grad_a_src', 'grad_a_dst')):
    for n, a, w in zip(names, got, want):
        assert_close_scaled(a, w.float().reshape(a.shape), tol=2e-5, what=f'{what} {n}')


@pytest.mark.parametrize('H,D', GRID)
def test_kernels_against_float64(dev, monkeypatch, H, D):
    P = _typed_problem(H, D, SEEDS[(H, D)])
    assert [et[0] for et in P['st'].edge_types].count('n0') == 3 and P['st'].num_nodes == 386
    assert P['leaky_margin'] >= 1e-6, P['leaky_margin']     # no argument near LeakyReLU's kink
    deg = torch.bincount(P['row'], minlength=P['st'].num_rows)
    assert int((deg == 0).sum()) > 0 and int(deg.max()) > 64  # empty rows and long ones
    # without the ReLU everything is compared elementwise
    sink = []
    got = _device(P, dev, False, sink, monkeypatch)
    perm = got[-1].by_dst().perm.long().cpu()
    want = _reference(P, False)
    want = (want[0], want[1][perm]) + want[2:]
    _check(got, want, f'{H}x{D} relu off')
    # a uniform graph has no long row: no hub plan in either direction
    records = [i for i, _, _ in sink if i.get('kind') == 'han']
    assert [i['op'] for i in records] == ['forward', 'backward_dst', 'backward_src']
    assert all(i['n_hub'] == 0 and i['n_chunks'] == 0 for i in records), records
    # with it: the forward elementwise, the gradients under the DEVICE's mask
    got = _device(P, dev, True)
    mask = (got[0] > 0).cpu()
    fwd = _reference(P, True)
    assert_close_scaled(got[0], fwd[0].float(), tol=2e-5, what=f'{H}x{D} relu out')
    want = _reference(P, True, mask=mask)
    _check(got[1:5], (want[1][perm], ) + want[2:], f'{H}x{D} relu', names=('alpha', 'grad_x',
                                                                           'grad_a_src',
                                                                           'grad_a_dst'))
    # and the device's mask is the float64 mask but for elements within rounding of 0
    pre = _reference(P, False)[0]
    differs = mask != (pre > 0)
    assert int(differs.sum()) <= 8, int(differs.sum())
    if bool(differs.any()):
        assert float(pre[differs].abs().max()) <= 2e-5 * float(pre.abs().max())


# ---- 3. long rows ----------------------------------------------------------------------------------------
AB, AB2, BA = ('a', 'r1', 'b'), ('a', 'r2', 'b'), ('b', 'r3', 'a')
LONG_SEED = 44   # (43 puts a LeakyReLU argument within 1e-6 of the kink)


@functools.lru_cache(maxsize=None)
def _long_row_problem():
    """Destination b[3] has exactly HUB_THRESHOLD + 1 slots under edge type AB and 6000 under AB2;
    source a[5] has 1500 out-edges under AB and 500 under AB2 (none of them to b[3])."""
    from pytorch_geometric_amd import _native
    T = _native.HUB_THRESHOLD
    g = gen(41)
    sizes = {'a': 7000, 'b': 40}

    def edges(n_hub, n_a5, n_rest):
        src = torch.cat([torch.randint(6, 7000, (n_hub, ), generator=g),
                         torch.full((n_a5, ), 5),
                         torch.randint(6, 7000, (n_rest, ), generator=g)])
        other = torch.randint(4, 40, (n_a5 + n_rest, ), generator=g)
        return torch.stack([src, torch.cat([torch.full((n_hub, ), 3), other])])

    ei = [edges(T + 1, 1500, 300), edges(6000, 500, 200), random_graph(40, 7000, 900, 42)]
    P = _typed_problem(2, 8, LONG_SEED, sizes=sizes, edges=[(AB, 0), (AB2, 0), (BA, 0)], ei=ei)
    assert P['leaky_margin'] >= 1e-6
    return P


def test_long_rows_in_both_directions(dev, monkeypatch):
    from pytorch_geometric_amd import _native
    T, C = _native.HUB_THRESHOLD, _native.HUB_CHUNK
    P = _long_row_problem()
    sink = []
    got = _device(P, dev, True, sink, monkeypatch)
    perm = got[-1].by_dst().perm.long().cpu()
    mask = (got[0] > 0).cpu()
    w64, w32 = _reference(P, True), _reference(P, True, dtype=torch.float32)
    assert_sum_close(got[0], w32[0], w64[0], what='long rows out')
    assert_sum_close(got[1], w32[1][perm], w64[1][perm], what='long rows alpha')
    want = _reference(P, True, mask=mask)
    _check(got[2:5], want[2:], 'long rows', names=('grad_x', 'grad_a_src', 'grad_a_dst'))
    info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'han'}
    chunks = lambda n: -(-n // C)                              # noqa: E731
    for op in ('forward', 'backward_dst'):
        assert info[op]['n_hub'] == 2 and info[op]['n_chunks'] == chunks(T + 1) + chunks(6000)
    assert info['backward_src']['n_hub'] == 1 and info['backward_src']['n_chunks'] == chunks(1500)


# ---- 4. repeatability ------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_identical(dev):
    P = _long_row_problem()
    a, b = _device(P, dev, True), _device(P, dev, True)
    for name, x, y in zip(('out', 'alpha', 'grad_x', 'grad_a_src', 'grad_a_dst'), a, b):
        assert torch.equal(x, y), f'{name} differs between two runs'


# ---- 5. non-finite scores, forward only ----------------------------------------------------------------
def test_non_finite_scores(dev):
    from pytorch_geometric_amd import _han
    from pytorch_geometric_amd._functions import HanAttendFunction
    P = dict(_typed_problem(3, 5, 23))
    col, row, st = P['col'], P['row'], P['st']
    deg = torch.bincount(row, minlength=st.num_rows)
    a_src = P['a_src'].clone()
    a_src[torch.arange(0, st.num_cols, 7), 0] = float('-inf')  # masked sources, head 0
    full = int(torch.nonzero((deg > 1) & (deg < 20))[0])       # a row whose every source is masked
    a_src[col[row == full], 1] = float('-inf')
    others = torch.nonzero(deg > 2).flatten()
    r_nan, r_inf = int(others[-1]), int(others[-2])
    c_nan, c_inf = int(col[row == r_nan][0]), int(col[row == r_inf][0])
    a_src[c_nan, 2] = float('nan')
    a_src[c_inf, 2] = float('inf')
    P['a_src'] = a_src
    graph = _han.build_stacked(st, [e.to(dev) for e in P['ei']])
    out, alpha = HanAttendFunction.apply(P['x'].to(dev), a_src.to(dev), P['a_dst'].to(dev), graph,
                                         st.types, SLOPE, True)
    want, want_alpha = R.attend(P['x'].double(), a_src.double(), P['a_dst'].double(), col, row,
                                st.types, SLOPE)
    perm = graph.by_dst().perm.long().cpu()
    for name, a, w in (('out', out.cpu(), want.float()),
                       ('alpha', alpha.cpu(), want_alpha[perm].float())):
        assert torch.equal(a.isnan(), w.isnan()), f'{name}: NaN pattern'
        assert_close_scaled(a.nan_to_num(nan=0.0), w.nan_to_num(nan=0.0), tol=2e-5, what=name)
    out3 = out.cpu().view(-1, 3, 5)
    assert bool(out3[full, 1].isnan().all()) and not bool(out3[full, 0].isnan().any())
    # NaN and +inf poison their own (row, head): the rows that read the poisoned column, head 2
    poisoned = torch.zeros(st.num_rows, dtype=torch.bool)
    poisoned[row[(col == c_nan) | (col == c_inf)]] = True
    assert bool(out3[poisoned, 2].isnan().all()) and not bool(out3[~poisoned, 2].isnan().any())
    assert bool((out3[deg == 0] == 0).all()) and int((deg == 0).sum()) > 0


# ---- the class against the float64 restatement ------------------------------------------------------
def _layer_and_reference(kwargs, x_dict, ei_dict, seed=3, flow='source_to_target', **layer_kw):
    from pytorch_geometric_amd.nn import HANConv
    torch.manual_seed(seed)
    layer = HANConv(**kwargs, flow=flow, **layer_kw).eval()
    with torch.no_grad():
        for p in list(layer.lin_src.values()) + list(layer.lin_dst.values()):
            p.copy_(torch.randn(p.shape, generator=gen(seed + 1)))
        # q ~ N(0, 1 / F): the semantic score, a sum of F products, stays O(1) at every width.  At
        # unit variance and F = 1024 it reaches tens, and the float32 rounding of that one sum
        # (F terms) alone moves beta, and every gradient behind it, by more than 2e-5
        layer.q.copy_(torch.randn(layer.q.shape, generator=gen(seed + 3)) / layer.q.size(-1) ** 0.5)
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    x64 = {t: v.double().requires_grad_(True) for t, v in x_dict.items()}
    want, beta = R.layer(p64, x64, ei_dict, kwargs['heads'], flow=flow)
    go = {t: torch.randn(v.shape, generator=gen(seed + 2)) for t, v in want.items()
          if v is not None}
    loss = sum((want[t] * go[t].double()).sum() for t in go)
    grads = torch.autograd.grad(loss, list(x64.values()) + list(p64.values()), allow_unused=True)
    return layer, want, beta, dict(zip(x64, grads)), dict(zip(p64, grads[len(x64):])), go


def _check_layer(layer, x_dict, ei_dict, ref, dev, what, tol=2e-5):
    want, beta, g_x, g_p, go = ref
    layer = layer.to(dev)
    xs = {t: v.to(dev).requires_grad_(True) for t, v in x_dict.items()}
    out, b = layer(xs, {et: ei.to(dev) for et, ei in ei_dict.items()},
                   return_semantic_attention_weights=True)
    assert list(out) == list(want), what
    params = list(layer.named_parameters())
    loss = sum((out[t] * go[t].to(dev)).sum() for t in go)
    grads = torch.autograd.grad(loss, list(xs.values()) + [p for _, p in params],
                                allow_unused=True)
    for t in want:
        if want[t] is None:
            assert out[t] is None and b[t] is None
            continue
        assert_close_scaled(out[t], want[t].float(), tol=tol, what=f'{what} out[{t}]')
        assert_close_scaled(b[t], beta[t].float(), tol=tol, what=f'{what} beta[{t}]')
    for t, g in zip(xs, grads):
        ref_g = g_x[t]
        assert_close_scaled(g, torch.zeros_like(g) if ref_g is None else ref_g.float(), tol=tol,
                            what=f'{what} grad_x[{t}]')
    for (n, _), g in zip(params, grads[len(xs):]):
        if g_p[n] is None:
            assert g is None or not bool(g.any()), f'{what}: unexpected gradient for {n}'
        else:
            assert_close_scaled(g, g_p[n].float(), tol=tol, what=f'{what} grad {n}')


# ---- 6. the edge-type limit -----------------------------------------------------------------------------
@pytest.mark.parametrize('n_et', [64, 65])
def test_edge_type_limit(dev, monkeypatch, n_et):
    g = gen(50)
    x = {'a': torch.randn(50, 6, generator=g), 'b': torch.randn(40, 6, generator=g)}
    ets = [('a', f'r{i}', 'b') for i in range(n_et)]
    ei = {et: random_graph(50, 40, 60, 51 + k) for k, et in enumerate(ets)}
    kwargs = dict(in_channels=6, out_channels=8, metadata=(['a', 'b'], ets), heads=2)
    layer, *ref = _layer_and_reference(kwargs, x, ei)
    layer.fuse = True
    c = _counted(monkeypatch, lambda: _check_layer(layer, x, ei, ref, dev, f'{n_et} edge types'))
    for name in HAN_CALLS:
        assert c.get(name, 0) == (1 if n_et == 64 else 0), (name, c)


# ---- 7. launch structure ---------------------------------------------------------------------------------
def _split_graph(dev, parts):
    base = {('a', 'b'): random_graph(3000, 2000, 24000, 90), ('b', 'a'): random_graph(2000, 3000,
                                                                                    24000, 91)}
    ei = {}
    for (s, d), full in base.items():
        for p, chunk in enumerate(full.chunk(parts, dim=1)):
            ei[(s, f'r{p}', d)] = chunk.contiguous().to(dev)
    return ei


def test_launch_structure_does_not_depend_on_the_number_of_edge_types(dev, monkeypatch):
    from pytorch_geometric_amd.nn import HANConv
    g = gen(92)
    x = {'a': torch.randn(3000, 32, generator=g).to(dev),
         'b': torch.randn(2000, 32, generator=g).to(dev)}
    for parts in (1, 4):
        ei = _split_graph(dev, parts)
        torch.manual_seed(parts)
        layer = HANConv(32, 32, (['a', 'b'], list(ei)), heads=2).to(dev)
        layer.fuse = True
        xs = {t: v.clone().requires_grad_(True) for t, v in x.items()}

        def step():
            out = layer(xs, ei)
            sum(v.sum() for v in out.values()).backward()

        calls = _counted(monkeypatch, step)
        assert len(ei) == 2 * parts
        for name in HAN_CALLS:
            assert calls.get(name) == 1, (parts, name, calls)
        assert not [n for n in calls if 'spmm' in n or 'softmax' in n or 'segment' in n], calls

    # three layers on one batch share one stacked handle: it is sorted by destination once and by
    # source once
    ei = _split_graph(dev, 2)
    layers = [HANConv(32, 32, (['a', 'b'], list(ei)), heads=2).to(dev) for _ in range(3)]
    for layer in layers:
        layer.fuse = True
    xs = {t: v.clone().requires_grad_(True) for t, v in x.items()}

    def model_step():
        h = xs
        for layer in layers:
            h = layer(h, ei)
        sum(v.sum() for v in h.values()).backward()

    c = _counted(monkeypatch, model_step)
    assert c['pygamd_index_sort'] <= 2, c
    assert all(c[name] == 3 for name in HAN_CALLS), c


# ---- 8. the memory promise -------------------------------------------------------------------------------
def test_fused_route_keeps_nothing_of_edge_times_width(dev):
    """3 node types x 2,000 nodes, four edge types x 250,000 edges, F = 64, H = 2.  The fused
    route's edge-sized tensors are alpha and grad_s, 2 * E * H * 4 bytes = 16 MB; one [E, F]
    float32 tensor is 256 MB, and the generic route holds several."""
    from pytorch_geometric_amd.nn import HANConv
    N, E, F, H = 2000, 1_000_000, 64, 2
    ets = [('a', 'r0', 'b'), ('b', 'r1', 'c'), ('c', 'r2', 'a'), ('a', 'r3', 'a')]
    g = gen(70)
    x = {t: torch.randn(N, F, generator=g).to(dev).requires_grad_(True) for t in 'abc'}
    ei = {et: random_graph(N, N, E // 4, 71 + k).to(dev) for k, et in enumerate(ets)}
    torch.manual_seed(7)
    layer = HANConv(F, F, (list('abc'), ets), heads=H).to(dev)
    layer.fuse = True

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
    print(f'generic: peak above the level before {generic / 2 ** 20:.1f} MiB')
    assert all(bool(torch.isfinite(v.grad).all()) for v in x.values())


# ---- 9. routing ----------------------------------------------------------------------------------------------
def _routing_inputs():
    g = gen(60)
    x = {'a': torch.randn(300, 16, generator=g), 'b': torch.randn(200, 16, generator=g)}
    ei = {AB: random_graph(300, 200, 2000, 61), AB2: random_graph(300, 200, 1500, 62),
          BA: random_graph(200, 300, 1800, 63)}
    return x, ei, (['a', 'b'], [AB, AB2, BA])


@pytest.mark.parametrize('what', ['H * D = 1024', 'fuse off', 'target_to_source', 'message hook',
                                  'dropout in training'])
def test_routing_to_the_generic_route(dev, monkeypatch, what):
    """Every one of these makes no ``pygamd_han_*`` call and still matches the restatement.  (With
    dropout in training the coefficients are random: the call is checked for its route, and the
    same layer in ``eval()`` — fused again — for its values.)"""
    x, ei, meta = _routing_inputs()
    wide = what == 'H * D = 1024'
    kwargs = dict(in_channels=16, out_channels=1024 if wide else 16, metadata=meta,
                  heads=8 if wide else 2)
    layer_kw = {'dropout': 0.5} if what == 'dropout in training' else {}
    flow = 'target_to_source' if what == 'target_to_source' else 'source_to_target'
    layer, *ref = _layer_and_reference(kwargs, x, ei, seed=9, flow=flow, **layer_kw)
    layer.fuse = what != 'fuse off'
    seen = []
    if what == 'message hook':
        layer.register_message_forward_hook(lambda mod, args, out: seen.append(tuple(out.shape)))
    if what == 'dropout in training':
        layer = layer.to(dev).train()
        xd = {t: v.to(dev) for t, v in x.items()}
        eid = {et: v.to(dev) for et, v in ei.items()}
        state = {}
        c = _counted(monkeypatch, lambda: state.update(out=layer(xd, eid)))
        assert not [n for n in c if 'pygamd_han' in n], c
        assert all(bool(torch.isfinite(v).all()) for v in state['out'].values())
        layer = layer.eval()
        c = _counted(monkeypatch, lambda: _check_layer(layer, x, ei, ref, dev, what))
        assert c.get('pygamd_han_forward') == 1, c
        return
    c = _counted(monkeypatch, lambda: _check_layer(layer, x, ei, ref, dev, what))
    assert not [n for n in c if 'pygamd_han' in n], (what, c)
    if what == 'message hook':
        assert seen == [(2000, 16), (1500, 16), (1800, 16)]    # [E, F] messages exist here


def test_plain_layer_is_fused_and_half_inputs_are_widened(dev, monkeypatch):
    from pytorch_geometric_amd.nn import HANConv
    x, ei, meta = _routing_inputs()
    torch.manual_seed(4)
    layer = HANConv(16, 16, meta, heads=2).to(dev).eval()
    layer.fuse = True
    xd = {t: v.to(dev) for t, v in x.items()}
    eid = {et: v.to(dev) for et, v in ei.items()}
    c = _counted(monkeypatch, lambda: layer(xd, eid))
    assert c.get('pygamd_han_forward') == 1 and 'pygamd_han_backward_dst' not in c
    want = layer(xd, eid)
    layer = layer.half()
    state = {}
    c = _counted(monkeypatch, lambda: state.update(
        out=layer({t: v.half() for t, v in xd.items()}, eid)))
    assert not [n for n in c if 'pygamd_han' in n], c
    for t in want:
        assert state['out'][t].dtype == torch.float16
        assert_close_scaled(state['out'][t].float(), want[t], tol=2e-2, what=f'half {t}')


# ---- 10. a sampled typed batch -----------------------------------------------------------------------------
def test_two_layers_on_a_sampled_batch_fused_against_generic(dev, monkeypatch):
    from pytorch_geometric_amd.loader import HeteroNeighborLoader
    from pytorch_geometric_amd.nn import HANConv
    num_nodes = {'u': 3000, 'i': 1500, 't': 200}
    widths = {'u': 12, 'i': 20, 't': 6}
    ets = [('u', 'buys', 'i'), ('i', 'bought_by', 'u'), ('u', 'follows', 'u'), ('i', 'has', 't')]
    g = gen(80)
    x_full = {t: torch.randn(n, widths[t], generator=g).to(dev) for t, n in num_nodes.items()}
    ei_full = {et: random_graph(num_nodes[et[0]], num_nodes[et[-1]], 12000, 81 + k).to(dev)
               for k, et in enumerate(ets)}
    loader = HeteroNeighborLoader(x_full, ei_full, [4, 4], 'u', batch_size=64, seed=5)
    batch = next(iter(loader))
    meta = (list(num_nodes), ets)
    torch.manual_seed(8)
    fused = [HANConv(widths, 16, meta, heads=2).to(dev), HANConv(16, 16, meta, heads=4).to(dev)]
    generic = copy.deepcopy(fused)
    for m in fused:
        m.fuse = True
    for m in generic:
        m.fuse = False
    go = torch.randn(64, 16, generator=g).to(dev)
    results = []
    for layers in (fused, generic):
        def run():
            h = layers[0](batch.x_dict, batch.edge_index_dict)
            h = layers[1](h, batch.edge_index_dict)
            out = h['u'][:64]
            params = [p for m in layers for p in m.parameters()]
            return out, torch.autograd.grad((out * go).sum(), params, allow_unused=True)
        state = {}
        c = _counted(monkeypatch, lambda: state.update(r=run()))
        assert c.get('pygamd_han_forward', 0) == (2 if layers is fused else 0), c
        results.append(state['r'])
    (out_f, g_f), (out_g, g_g) = results
    assert_close_scaled(out_f, out_g, tol=2e-5, what='sampled out')
    names = [f'{i}.{n}' for i, m in enumerate(fused) for n, _ in m.named_parameters()]
    for n, a, w in zip(names, g_f, g_g):
        if w is None:
            assert a is None or not bool(a.any()), n
        else:
            assert_close_scaled(a, w, tol=2e-5, what=f'sampled grad {n}')


# ---- 11. the registered operator ---------------------------------------------------------------------------
def test_operator_equals_the_autograd_node_and_has_a_fake_kernel(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'han_attend' in ops.OPS and 'han_attend_backward' in ops.OPS
    op = torch.ops.pyg_amd.han_attend
    with FakeTensorMode():
        x = torch.empty(50, 3, 8, device='cuda', requires_grad=True)
        a_s, a_d = torch.empty(70, 3, device='cuda'), torch.empty(30, 3, device='cuda')
        ptr = torch.empty(31, dtype=torch.int64, device='cuda')
        col = torch.empty(400, dtype=torch.int64, device='cuda')
        out, alpha = op(x, a_s, a_d, ptr, col, [0, 10, 30], [0, 50, 70], [0, -20], 0.2, True)
        assert out.shape == (30, 24) and alpha.shape == (400, 3) and out.requires_grad
        assert out.device.type == 'cuda' and out.dtype == torch.float32
        gx, gs, gd = torch.ops.pyg_amd.han_attend_backward(
            torch.empty(30, 24, device='cuda'), x, a_s, a_d, alpha, out, ptr, col, [0, 10, 30],
            [0, 50, 70], [0, -20], 0.2, True)
        assert gx.shape == x.shape and gs.shape == a_s.shape and gd.shape == a_d.shape

    # the stacked edge list sorted by destination: the operator's by-source form (a stable sort of
    # col) then orders the slots of a source as the handle's does, and the sums agree bit for bit
    P = _typed_problem(3, 8, 29, sort_dst=True)
    want = _device(P, dev, True)
    graph = want[-1]
    fwd = graph.by_dst()
    types = [list(t) for t in P['st'].types]
    go = P['go'].to(dev)

    def leaves():
        return [P[k].to(dev).requires_grad_(True) for k in ('x', 'a_src', 'a_dst')]

    def fn(x, a_s, a_d):
        return op(x * 1.0, a_s, a_d, fwd.ptr, fwd.idx, *types, SLOPE, True)

    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        out, alpha = f(*ls)
        grads = torch.autograd.grad((out * go).sum(), ls)
        for name, a, w in zip(('out', 'alpha', 'grad_x', 'grad_a_src', 'grad_a_dst'),
                              (out, alpha) + grads, want):
            assert torch.equal(a, w), f'operator vs node: {name}'
    torch.library.opcheck(op, (*leaves(), fwd.ptr, fwd.idx, *types, SLOPE, True))
    torch.library.opcheck(op, (*leaves(), fwd.ptr, fwd.idx, *types, SLOPE, False))
