"""nn.HeteroConv on the device: the reference's recorded cases on the fast and on the generic path,
the two kernels of csrc/hetero_conv.hip against pygamd_spmm_csr and the float64 restatement
(tests/_hetero_conv_ref.py), an end-to-end sampled training step, the launch structure and the
kernel's own index guard."""

import pytest
import torch
import torch.nn.functional as F

import _hetero_conv_ref as R
from pytorch_geometric_amd.nn import HeteroConv, HeteroDictLinear, SAGEConv
from _util import _call_counts as _counted
from _util import assert_close, assert_close_scaled, assert_sum_close, random_graph
from test_hetero_conv_host import build_layer, load_golden

pytestmark = pytest.mark.gpu


def cpu64(t):
    return t.detach().cpu().double()


# ---- 1. the golden cases ------------------------------------------------------------------------
def run_golden_case(G, name, case, dev, fuse):
    from pytorch_geometric_amd import _hetero
    layer = build_layer(G, case, dev)
    layer.fuse = fuse
    xs = {t: v.to(dev).requires_grad_(True) for t, v in G['x_dict'].items()}
    ei = {et: v.to(dev) for et, v in G['edge_index'].items()}
    planned = layer._fast_plan((xs, ei), {}) is not None
    assert planned == (fuse and case['group_aggr'] in _hetero.FAST_GROUP_AGGRS), name
    out = layer(xs, ei)
    assert list(out) == case['out_order']
    for t in out:
        assert_close(out[t], case['out'][t], what=f'{name} fuse={fuse} out[{t}]')
    names = [n for n, _ in layer.named_parameters()]
    leaves = list(xs.values()) + [p for _, p in layer.named_parameters()]
    grads = torch.autograd.grad([out[t] for t in out], leaves,
                                [case['grad_out'][t].to(dev) for t in out])
    for t, g in zip(xs, grads):
        assert_close_scaled(g, case['grad_x'][t], what=f'{name} fuse={fuse} grad_x[{t}]')
    for n, g in zip(names, grads[len(xs):]):
        assert_close_scaled(g, case['grad_params'][n], what=f'{name} fuse={fuse} grad {n}')
    return planned


def test_golden_cases_fast_and_generic(dev):
    G = load_golden()
    fast = 0
    for name, case in G['cases'].items():
        fast += run_golden_case(G, name, case, dev, fuse=True)
        if case['group_aggr'] in ('sum', 'mean'):      # every eligible case once more, forced off
            assert not run_golden_case(G, name, case, dev, fuse=False)
    assert fast == 4


# ---- helpers: a random typed graph and its stacked handle ---------------------------------------------
def typed_graph(dev, num_nodes, spec, dtype=torch.int64, seed=0, skew=False):
    """``spec``: ``[(src type, dst type, edges)]`` -> (edge types, edge_index list)."""
    ets, eis = [], []
    for k, (s, d, e) in enumerate(spec):
        ets.append((s, f'r{k}', d))
        eis.append(random_graph(num_nodes[s], num_nodes[d], e, seed + k, dtype=dtype,
                                skew=skew).to(dev))
    return ets, eis


def make_handle(ets, eis, num_nodes):
    from pytorch_geometric_amd._hetero import HeteroGraph
    return HeteroGraph(ets, eis, [num_nodes[et[0]] for et in ets], [num_nodes[et[-1]] for et in ets])


def run_forward(h, ets, xs, means):
    from pytorch_geometric_amd import _native
    Fw = next(iter(xs.values())).size(1)
    dev = h.rowptr.device
    outs = [torch.full((h.row_begin[k + 1] - h.row_begin[k], Fw), float('nan'), device=dev)
            for k in range(len(ets))]
    _native.hetero_spmm(h.rowptr, h.col, h.row_begin, [xs[et[0]] for et in ets], outs, means)
    return outs


# ---- 2. the forward kernel against pygamd_spmm_csr ---------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('Fw', [16, 100, 256])
def test_forward_matches_spmm_csr_bit_for_bit(dev, Fw, dtype):
    from pytorch_geometric_amd import _native
    num_nodes = {'a': 700, 'b': 300, 'c': 50}
    spec = [('a', 'b', 4000), ('b', 'b', 2500), ('c', 'b', 0), ('c', 'a', 900), ('a', 'c', 30)]
    ets, eis = typed_graph(dev, num_nodes, spec, dtype=dtype, seed=40)
    # one row of 5,000 slots (above the SpMM's hub threshold) in the first edge type
    hub_row = 7
    long_row = torch.stack([torch.randint(0, 700, (5000, ), generator=torch.Generator().manual_seed(3)),
                            torch.full((5000, ), hub_row)]).to(dtype).to(dev)
    eis[0] = torch.cat([eis[0], long_row], dim=1)
    g = torch.Generator().manual_seed(41)
    xs = {t: torch.randn(n, Fw, generator=g).to(dev) for t, n in num_nodes.items()}
    means = [True, False, True, True, False]
    h = make_handle(ets, eis, num_nodes)
    assert h.rowptr.dtype == dtype and h.col.dtype == dtype
    outs = run_forward(h, ets, xs, means)
    empty_rows = 0
    for k, et in enumerate(ets):
        lo, hi = h.row_begin[k], h.row_begin[k + 1]
        rowptr = (h.rowptr[lo:hi + 1] - h.rowptr[lo]).contiguous()
        col = h.col[int(h.rowptr[lo]):int(h.rowptr[hi])].contiguous()
        reduce = 'mean' if means[k] else 'sum'
        if col.numel() == 0:                       # the empty edge type: every row is empty
            assert k == 2 and not bool(outs[k].any())
            empty_rows += hi - lo
            continue
        ref = _native.spmm_csr(rowptr, col, xs[et[0]], reduce, hub=_native.hub_plan(rowptr))
        deg = (rowptr[1:] - rowptr[:-1]).cpu()
        short = deg <= _native.HUB_THRESHOLD
        empty_rows += int((deg == 0).sum())
        assert torch.equal(outs[k].cpu()[short], ref.cpu()[short]), f'{et}: bits differ'
        assert bool((outs[k].cpu()[deg == 0] == 0).all())
        # every row, the long one included, against float64
        x64, ei = cpu64(xs[et[0]]), eis[k].cpu()
        exact = R.aggregate(x64, ei, num_nodes[et[-1]], reduce)
        ref32 = R.aggregate(xs[et[0]].cpu(), ei, num_nodes[et[-1]], reduce)
        assert_sum_close(outs[k], ref32, exact, what=f'{et} vs fp64')
        if k == 0:
            assert int(deg[hub_row]) >= 5000
    assert empty_rows > 0 and outs[2].shape == (300, Fw) and not bool(outs[2].any())


def test_forward_writes_column_blocks_and_unaligned_widths(dev):
    """Output blocks inside a wider matrix (the layer's layout) and a width that forces the scalar
    lane shape."""
    num_nodes = {'a': 200, 'b': 90}
    for Fw in (8, 7):
        ets, eis = typed_graph(dev, num_nodes, [('a', 'b', 900), ('b', 'b', 500)], seed=50)
        g = torch.Generator().manual_seed(51)
        xs = {t: torch.randn(n, Fw, generator=g).to(dev) for t, n in num_nodes.items()}
        h = make_handle(ets, eis, num_nodes)
        from pytorch_geometric_amd import _native
        wide = torch.full((90, 3 * Fw), -7.0, device=dev)
        _native.hetero_spmm(h.rowptr, h.col, h.row_begin, [xs['a'], xs['b']],
                            [wide[:, :Fw], wide[:, Fw:2 * Fw]], [True, False])
        assert bool((wide[:, 2 * Fw:] == -7.0).all())
        for k, (et, red) in enumerate(zip(ets, ('mean', 'sum'))):
            ref = R.aggregate(xs[et[0]].cpu(), eis[k].cpu(), 90, red)
            assert_close(wide[:, k * Fw:(k + 1) * Fw], ref, what=f'F={Fw} block {k}')


# ---- 3. the backward kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('Fw', [16, 100, 256])
def test_backward_matches_float64_and_is_deterministic(dev, Fw, dtype):
    from pytorch_geometric_amd import _native
    num_nodes = {'a': 700, 'b': 300, 'c': 50}
    spec = [('a', 'b', 4000), ('b', 'b', 2500), ('c', 'b', 0), ('c', 'a', 900), ('a', 'c', 30),
            ('a', 'a', 1500)]
    ets, eis = typed_graph(dev, num_nodes, spec, dtype=dtype, seed=60, skew=True)
    means = [True, False, True, True, False, True]
    h = make_handle(ets, eis, num_nodes)
    g = torch.Generator().manual_seed(61)
    grads = [torch.randn(num_nodes[et[-1]], Fw, generator=g).to(dev) for et in ets]
    rowptr_t, col_t = h.transposed()
    assert h.src_types == ['a', 'b', 'c']

    def run():
        gx = [torch.full((num_nodes[t], Fw), float('nan'), device=dev) for t in h.src_types]
        _native.hetero_spmm_backward(rowptr_t, col_t, h.rowptr, h.row_begin, grads, means,
                                     h.src_begin, gx)
        return gx

    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    xs = {t: torch.zeros(n, Fw, dtype=torch.float64, requires_grad=True)
          for t, n in num_nodes.items()}
    total = 0
    for k, et in enumerate(ets):
        agg = R.aggregate(xs[et[0]], eis[k].cpu(), num_nodes[et[-1]], 'mean' if means[k] else 'sum')
        total = total + (agg * cpu64(grads[k])).sum()
    want = torch.autograd.grad(total, [xs[t] for t in h.src_types])
    for t, got, ref in zip(h.src_types, first, want):
        assert_close_scaled(got, ref.float(), what=f'grad_x[{t}] F={Fw}')


# ---- 4. randomised property test ----------------------------------------------------------------------
def test_layer_on_a_large_skewed_graph(dev):
    num_nodes = {'a': 8000, 'b': 6000, 'c': 4000, 'd': 2000}
    spec = [('a', 'b', 50000), ('b', 'a', 50000), ('c', 'a', 50000), ('a', 'a', 50000),
            ('d', 'b', 50000), ('b', 'c', 50000), ('c', 'd', 50000), ('a', 'b', 50000)]
    ets, eis = typed_graph(dev, num_nodes, spec, seed=70, skew=True)
    K, N = 64, 32
    torch.manual_seed(7)
    layer = HeteroConv({et: SAGEConv((K, K), N, aggr='mean' if k % 2 else 'sum')
                        for k, et in enumerate(ets)}, aggr='mean').to(dev)
    g = torch.Generator().manual_seed(71)
    x = {t: torch.randn(n, K, generator=g) for t, n in num_nodes.items()}
    ei = dict(zip(ets, eis))
    xg = {t: v.to(dev) for t, v in x.items()}
    assert layer._fast_plan((xg, ei), {}) is not None
    out = layer(xg, ei)
    params = {k: v.detach().cpu() for k, v in layer.state_dict().items()}
    conv_aggr = {et: layer.convs[et].aggr for et in ets}
    ei_cpu = {et: v.cpu() for et, v in ei.items()}
    ref32 = R.hetero_conv(ets, x, ei_cpu, params, conv_aggr, 'mean')
    exact = R.hetero_conv(ets, {t: v.double() for t, v in x.items()}, ei_cpu,
                          {k: v.double() for k, v in params.items()}, conv_aggr, 'mean')
    assert list(out) == list(exact)
    for t in out:
        assert_sum_close(out[t], ref32[t], exact[t], what=f'out[{t}]')
    # the input gradients at this size: the long source rows of the transposed structure
    go = {t: torch.randn(out[t].shape, generator=g) for t in out}
    for v in xg.values():
        v.requires_grad_(True)
    got = torch.autograd.grad([layer(xg, ei)[t] for t in out], list(xg.values()),
                              [go[t].to(dev) for t in out])

    def input_grads(dtype):
        xs = {t: v.to(dtype).requires_grad_(True) for t, v in x.items()}
        res = R.hetero_conv(ets, xs, ei_cpu, {k: v.to(dtype) for k, v in params.items()},
                            conv_aggr, 'mean')
        return torch.autograd.grad([res[t] for t in out], list(xs.values()),
                                   [go[t].to(dtype) for t in out])

    for t, a, b, c in zip(xg, got, input_grads(torch.float32), input_grads(torch.float64)):
        assert_sum_close(a, b, c, what=f'grad_x[{t}]')


# ---- 5. end to end: sampled batch -> HeteroDictLinear -> 2 x (HeteroConv, ReLU) -> loss ----------------
def _restate_model(x, ei, ets, lin_state, conv_states, seeds, y, dtype):
    """The model of the end-to-end test in plain torch; returns (loss, logits, smallest distance of
    a pre-activation that matters from the ReLU kink)."""
    h = {t: v.to(dtype) @ lin_state[f'lins.{t}.weight'].to(dtype).t()
         + lin_state[f'lins.{t}.bias'].to(dtype) for t, v in x.items()}
    margin = float('inf')
    for i, st in enumerate(conv_states):
        pre = R.hetero_conv(ets, h, ei, {k: v.to(dtype) for k, v in st.items()}, 'mean', 'sum')
        for t, p in pre.items():
            rows = p if i + 1 < len(conv_states) else (p[:seeds] if t == 'u' else p[:0])
            if rows.numel():
                margin = min(margin, float(rows.detach().abs().min()))
        h = {t: p.relu() for t, p in pre.items()}
    logits = h['u'][:seeds]
    return F.cross_entropy(logits, y), logits, margin


def test_end_to_end_sampled_training_step(dev):
    from pytorch_geometric_amd.loader import HeteroNeighborLoader
    num_nodes = {'u': 6000, 'i': 3000}
    widths = {'u': 24, 'i': 40}
    H, C, B = 16, 16, 256
    ets = [('u', 'buys', 'i'), ('i', 'bought_by', 'u'), ('u', 'follows', 'u')]
    g = torch.Generator().manual_seed(80)
    x_full = {t: torch.randn(n, widths[t], generator=g).to(dev) for t, n in num_nodes.items()}
    ei_full = {et: random_graph(num_nodes[et[0]], num_nodes[et[-1]], 40000, 81 + k).to(dev)
               for k, et in enumerate(ets)}
    y_full = torch.randint(0, C, (num_nodes['u'], ), generator=g).to(dev)
    loader = HeteroNeighborLoader(x_full, ei_full, [6, 6], 'u', batch_size=B, y=y_full, seed=5)
    batch = next(iter(loader))
    assert batch.batch_size == B and batch.x_dict['u'].size(0) >= 1024
    y = batch.y[:B].long()

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = HeteroDictLinear(widths, H)
            self.convs = torch.nn.ModuleList(
                [HeteroConv({et: SAGEConv((H, H), H) for et in ets}, aggr='sum')
                 for _ in range(2)])

        def forward(self, x_dict, edge_index_dict):
            h = self.lin(x_dict)
            for conv in self.convs:
                h = {t: v.relu() for t, v in conv(h, edge_index_dict).items()}
            return h

    x_cpu = {t: v.cpu() for t, v in batch.x_dict.items()}
    ei_cpu = {et: v.cpu().long() for et, v in batch.edge_index_dict.items()}
    # ReLU makes two float32 evaluations comparable only away from the kink: take the first model
    # seed whose float64 pre-activations keep a margin, and assert that margin
    for model_seed in range(8):
        torch.manual_seed(model_seed)
        net = Net()
        lin_state = {k: v.clone() for k, v in net.lin.state_dict().items()}
        conv_states = [{k: v.clone() for k, v in c.state_dict().items()} for c in net.convs]
        _, _, margin = _restate_model(x_cpu, ei_cpu, ets, lin_state, conv_states, B, y.cpu(),
                                      torch.float64)
        if margin >= 2e-6:
            break
    assert margin >= 2e-6, f'a pre-activation sits {margin:.1e} from the ReLU kink'

    lin_leaves = {k: v.clone().requires_grad_(True) for k, v in lin_state.items()}
    conv_leaves = [{k: v.clone().requires_grad_(True) for k, v in st.items()} for st in conv_states]
    ref_loss, ref_logits, _ = _restate_model(x_cpu, ei_cpu, ets, lin_leaves, conv_leaves, B,
                                             y.cpu(), torch.float32)
    ref_loss.backward()

    net = net.to(dev)
    for conv in net.convs:
        assert conv._fast_plan((net.lin(batch.x_dict), batch.edge_index_dict), {}) is not None
    out = net(batch.x_dict, batch.edge_index_dict)
    loss = F.cross_entropy(out['u'][:B], y)
    loss.backward()
    assert_close(loss, ref_loss, what='loss')
    assert_close(out['u'][:B], ref_logits, what='logits')
    for k, p in net.lin.named_parameters():
        assert_close_scaled(p.grad, lin_leaves[k].grad, what=f'lin.{k}')
    for i, conv in enumerate(net.convs):
        for k, p in conv.named_parameters():
            want = conv_leaves[i][k].grad
            if want is None:   # the last layer's output for 'i' does not reach the loss
                assert i == 1 and k.startswith('convs.<u___buys___i>')
                assert p.grad is None or not bool(p.grad.any())
            else:
                assert_close_scaled(p.grad, want, what=f'convs.{i}.{k}')

    # a few optimizer steps on the user's own parameters: the loss falls
    opt = torch.optim.Adam(net.parameters(), lr=0.01)
    losses = []
    for _ in range(12):
        opt.zero_grad()
        step_loss = F.cross_entropy(net(batch.x_dict, batch.edge_index_dict)['u'][:B], y)
        step_loss.backward()
        opt.step()
        losses.append(step_loss.item())
    assert losses[-1] < losses[0]


# ---- 6. launch structure ----------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_the_number_of_edge_types(dev, monkeypatch):
    num_nodes = {'a': 3000, 'b': 2000}
    K = 32
    base = {('a', 'b'): random_graph(3000, 2000, 24000, 90).to(dev),
            ('b', 'a'): random_graph(2000, 3000, 24000, 91).to(dev)}
    g = torch.Generator().manual_seed(92)
    x = {t: torch.randn(n, K, generator=g).to(dev) for t, n in num_nodes.items()}

    def graph(parts):
        ei = {}
        for (s, d), full in base.items():
            for p, chunk in enumerate(full.chunk(parts, dim=1)):
                ei[(s, f'r{p}', d)] = chunk.contiguous()
        return ei

    def one_layer(parts):
        ei = graph(parts)
        torch.manual_seed(9)
        layer = HeteroConv({et: SAGEConv((K, K), K) for et in ei}, aggr='sum').to(dev)
        xs = {t: v.clone().requires_grad_(True) for t, v in x.items()}

        def step():
            out = layer(xs, ei)
            sum(o.sum() for o in out.values()).backward()
        assert layer._fast_plan((xs, ei), {}) is not None
        return _counted(monkeypatch, step)

    two, eight = one_layer(1), one_layer(4)
    assert len(graph(1)) == 2 and len(graph(4)) == 8
    assert two == eight, (two, eight)
    assert two['pygamd_hetero_spmm'] == 1 and two['pygamd_hetero_spmm_backward'] == 1
    assert two['pygamd_index_sort'] == 2

    # a 3-layer model on one batch: the handle is shared by the layers and by forward / backward
    ei = graph(4)
    torch.manual_seed(10)
    layers = torch.nn.ModuleList([HeteroConv({et: SAGEConv((K, K), K) for et in ei})
                                  for _ in range(3)]).to(dev)
    xs = {t: v.clone().requires_grad_(True) for t, v in x.items()}

    def model_step():
        h = xs
        for layer in layers:
            h = {t: v.relu() for t, v in layer(h, ei).items()}
        sum(o.sum() for o in h.values()).backward()

    calls = _counted(monkeypatch, model_step)
    assert calls['pygamd_index_sort'] <= 2
    assert calls['pygamd_hetero_spmm'] == 3 and calls['pygamd_hetero_spmm_backward'] == 3


# ---- 7. the kernel's own index guard ----------------------------------------------------------------------
def test_out_of_range_source_id_is_flagged_not_read(dev, monkeypatch):
    """A hand-built stacked CSR with one source id past its matrix, handed to the `_native` wrapper
    directly (the handle's range check never sees it): the kernel reads row 0 for that slot, sets
    the flag, and the flag travels the package's index-error route."""
    from pytorch_geometric_amd import _native
    xa = torch.arange(40, dtype=torch.float32, device=dev).view(10, 4) + 1
    xb = torch.ones(5, 4, device=dev)
    # edge type 0 (source a, 10 rows): destination rows 0..2; edge type 1 (source b, 5 rows): rows 3..4
    rowptr = torch.tensor([0, 2, 2, 3, 5, 6], device=dev)
    good = torch.tensor([1, 2, 9, 0, 4, 3], device=dev)
    bad = torch.tensor([1, 2, 9, 0, 7, 3], device=dev)        # 7 >= 5 rows of `b`

    def run(col, check):
        outs = [torch.zeros(3, 4, device=dev), torch.zeros(2, 4, device=dev)]
        _native.hetero_spmm(rowptr, col, [0, 3, 5], [xa, xb], outs, [False, False],
                            check_bounds=check)
        return outs

    monkeypatch.setattr(_native, 'INDEX_CHECK', 'sync')
    outs = run(good, True)
    assert torch.equal(outs[0][0], xa[1] + xa[2]) and torch.equal(outs[1][0], 2 * xb[0])
    with pytest.raises(IndexError):
        run(bad, True)
    monkeypatch.setattr(_native, 'INDEX_CHECK', 'async')
    _native.check_index_errors()
    outs = run(bad, True)                                      # reported later, nothing faults
    with pytest.raises(IndexError):
        _native.check_index_errors()
    _native.check_index_errors()                               # reported once
    torch.cuda.synchronize()
    assert torch.equal(outs[1][0], xb[0] + xb[0])              # the bad slot read row 0
    assert torch.equal(outs[0][2], xa[9])
    # the handle refuses such an edge_index before any launch
    from pytorch_geometric_amd._hetero import HeteroGraph
    with pytest.raises(IndexError, match="outside the valid range"):
        HeteroGraph([('b', 'r', 'a')], [torch.tensor([[0, 5], [1, 2]], device=dev)], [5], [10])
