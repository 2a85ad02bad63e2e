"""nn.PNAConv / nn.aggr.DegreeScalerAggregation on host tensors: the float64 restatement
(tests/_pna_ref.py) and the class against every recorded reference case
(tests/golden/golden_pna_v1.pt), state-dict keys, the constructor errors,
``get_degree_histogram``, the envelope of the kernel pair and the operator's registration.  No GPU
needed."""
import pytest
import torch

import _pna_ref as R
from _util import assert_close, assert_close_scaled, gen, random_graph


@pytest.mark.parametrize('name', R.CASES)
def test_restatement_matches_the_recorded_cases(name):
    G = R.load_golden()
    case = G['cases'][name]
    state = {k: v.double() for k, v in case['state'].items()}
    x = G['x'].double().requires_grad_(True)
    leaves = [x]
    ea = None
    if 'edge_attr' in case:
        ea = case['edge_attr'].double().requires_grad_(True)
        leaves.append(ea)
    out = R.pna_layer(x, ea, G['edge_index'], state, case['kwargs'])
    grads = torch.autograd.grad(out, leaves, case['grad_out'].double())
    assert_close(out.float(), case['out'], rtol=1e-5, atol=1e-5, what=f'{name} out')
    assert_close(grads[0].float(), case['grad_x'], rtol=1e-5, atol=1e-5, what=f'{name} grad_x')
    if ea is not None:
        assert_close(grads[1].float(), case['grad_edge_attr'], rtol=1e-5, atol=1e-5,
                     what=f'{name} grad_edge_attr')


@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_host_tensors(name):
    R.check_class_case(R.load_golden(), name, 'cpu')


def test_state_dicts_load_strictly_with_the_recorded_keys():
    G = R.load_golden()
    for name in R.CASES:
        layer = R.make_layer(G, name)               # asserts the key order, loads with strict=True
        case = G['cases'][name]
        kw = case['kwargs']
        keys = list(layer.state_dict())
        assert keys[:2] == ['aggr_module.avg_deg_lin', 'aggr_module.avg_deg_log']
        assert ('edge_encoder.weight' in keys) == bool(kw.get('edge_dim'))
        assert keys[-2:] == ['lin.weight', 'lin.bias']
        T = kw.get('towers', 1)
        assert f'pre_nns.{T - 1}.0.weight' in keys and f'post_nns.{T - 1}.0.bias' in keys
        assert (f'pre_nns.0.2.weight' in keys) == (kw.get('pre_layers', 1) == 2)
        trainable = 'aggr_module.avg_deg_lin' in dict(layer.named_parameters())
        assert trainable is bool(kw.get('train_norm'))
        for k, v in case['state'].items():
            assert torch.equal(layer.state_dict()[k], v), (name, k)


def test_degree_scaler_aggregation_matches_the_restatement():
    """The constants and the five scalers on host tensors, degree-0 rows included.  The package's
    aggregations themselves are device kernels without a host path: the whole module runs against
    the same restatement in tests/test_gpu_pna.py."""
    from pytorch_geometric_amd.nn.aggr import DegreeScalerAggregation, MultiAggregation
    x, index, hist, aggrs, scalers = R.scaler_problem()
    mod = DegreeScalerAggregation(aggrs, scalers, hist)
    assert isinstance(mod.aggr, MultiAggregation)
    assert list(mod.state_dict()) == ['avg_deg_lin', 'avg_deg_log'] and not list(mod.parameters())
    deg = torch.bincount(index, minlength=40)
    assert int((deg == 0).sum()) >= 5
    assert float(mod.avg_deg_lin) == pytest.approx(float(deg.double().mean()), rel=1e-6)
    assert float(mod.avg_deg_log) == pytest.approx(float((deg.double() + 1).log().mean()), rel=1e-6)
    agg = torch.cat(R.aggregate(x.double(), index, 40, aggrs), dim=-1)
    got = mod.scale(agg.float(), deg)
    want = R.scale(agg, deg.double().view(-1, 1), scalers, mod.avg_deg_lin.double(),
                   mod.avg_deg_log.double())
    assert got.shape == (40, 7 * 6 * 5)
    assert_close_scaled(got, want.float(), tol=2e-5, what='all scalers')
    assert float(got[deg == 0].abs().max()) == 0.0
    # one aggregation given as a string: the scaler comes as a string too; trainable constants
    mod = DegreeScalerAggregation('mean', 'linear', hist, train_norm=True)
    assert sorted(n for n, _ in mod.named_parameters()) == ['avg_deg_lin', 'avg_deg_log']
    assert mod.scaler == ['linear']
    mod.avg_deg_lin.data.fill_(9.0)
    mod.reset_parameters()
    assert float(mod.avg_deg_lin.detach()) == pytest.approx(float(deg.double().mean()), rel=1e-6)


def test_the_split_of_the_linear_message_and_the_coefficient_rows():
    """What the fused route rests on, in float64 on the host: the layer's packed projection and
    ``Wc`` reproduce the recorded output through the node's restatement, and the coefficient rows
    of ``pna_coefficients`` turn the slots' ``u`` into autograd's gradient of the node."""
    from pytorch_geometric_amd._functions import pna_coefficients
    G = R.load_golden()
    ei = G['edge_index']
    src, dst = ei[0], ei[1]
    n = G['x'].size(0)
    deg = torch.bincount(dst, minlength=n)
    for name in [c for c in R.CASES if c not in R.GENERIC_CASES]:
        case = G['cases'][name]
        layer = R.make_layer(G, name).double()
        kw = case['kwargs']
        T, Fi = layer.towers, layer.F_in
        W = T * Fi
        packed, bias, Wc = [None if t is None else t.double() for t in layer._split_weights()]
        P = G['x'].double() @ packed.t() + bias
        p_src, p_dst = P[:, :W].clone().requires_grad_(True), P[:, W:].clone().requires_grad_(True)
        ea = case['edge_attr'].double() if 'edge_attr' in case else None
        stats = tuple(kw['aggregators'])
        outs = R.pna_aggregate(p_src, p_dst, ea, Wc, ei, n, stats)
        agg = torch.cat([o.view(n, T, Fi) for o in outs], dim=-1)
        mod = layer.aggr_module
        agg = R.scale(agg, deg.double().view(-1, 1, 1), kw['scalers'], mod.avg_deg_lin.detach(),
                      mod.avg_deg_log.detach())
        xt = G['x'].double().view(n, -1, Fi).expand(n, T, Fi)
        h = torch.cat([xt, agg], dim=-1)
        out = layer.lin(torch.cat([nn(h[:, t]) for t, nn in enumerate(layer.post_nns)], dim=1))
        assert_close_scaled(out.float(), case['out'], tol=2e-5, what=f'{name} split out')
        # the coefficient rows against autograd through the node
        gs = [torch.randn(n, W, generator=gen(3 + q), dtype=torch.float64) for q in range(len(stats))]
        want_src, want_dst = torch.autograd.grad(outs, [p_src, p_dst], gs)
        u = p_src.detach()[src] + (0 if Wc is None else ea @ Wc.t())
        planes = dict(zip(('mean', 'min', 'max', 'std'),
                          R.aggregate(u, dst, n, ['mean', 'min', 'max', 'std'])))
        ties = [torch.zeros(n, W, dtype=torch.float64).index_add_(
            0, dst, (u == planes[k][dst]).double()).clamp(min=1) for k in ('min', 'max')]
        saved = torch.stack([planes['mean'], planes['min'], planes['max'], planes['std']] + ties)
        A, B, Gmin, Gmax, mn, mx = pna_coefficients(saved, deg, stats, gs).unbind(1)
        grad_u = A[dst] + B[dst] * u + Gmin[dst] * (u == mn[dst]) + Gmax[dst] * (u == mx[dst])
        got_src = torch.zeros(n, W, dtype=torch.float64).index_add_(0, src, grad_u)
        assert_close(got_src, want_src, rtol=1e-9, atol=1e-9, what=f'{name} grad_p_src')
        keep = [g for s_, g in zip(stats, gs) if s_ != 'std']
        got_dst = sum(keep) * (deg > 0).view(-1, 1) if keep else torch.zeros_like(want_dst)
        assert_close(got_dst, want_dst, rtol=1e-9, atol=1e-9, what=f'{name} grad_p_dst')


def test_constructor_and_forward_errors():
    from pytorch_geometric_amd.nn import PNAConv
    from pytorch_geometric_amd.nn.aggr import DegreeScalerAggregation
    hist = torch.tensor([1, 3, 2])
    with pytest.raises(ValueError, match='valid aggregation schemes'):
        DegreeScalerAggregation(3, ['identity'], hist)
    with pytest.raises(ValueError, match='Could not resolve aggregation'):
        DegreeScalerAggregation(['mean', 'median'], ['identity'], hist)
    mod = DegreeScalerAggregation(['mean'], ['identity', 'squared'], hist)
    with pytest.raises(ValueError, match="Unknown scaler 'squared'"):
        mod.scale(torch.randn(3, 2), torch.tensor([1, 2, 1]))
    with pytest.raises(NotImplementedError, match="requires 'index'"):
        mod(torch.randn(4, 2), ptr=torch.tensor([0, 2, 4]))
    with pytest.raises(ValueError, match='two-dimensional'):
        mod(torch.randn(4, 2, 2), torch.tensor([0, 1, 1, 2]), dim_size=3)
    with pytest.raises(AssertionError):
        PNAConv(16, 10, ['mean'], ['identity'], hist, towers=4)
    with pytest.raises(AssertionError):
        PNAConv(10, 16, ['mean'], ['identity'], hist, towers=4, divide_input=True)
    with pytest.raises(ValueError, match="'flow'"):
        PNAConv(16, 16, ['mean'], ['identity'], hist, flow='sideways')
    layer = PNAConv(16, 8, ['mean', 'std'], ['identity'], hist, towers=2, edge_dim=5)
    assert repr(layer) == 'PNAConv(16, 8, towers=2, edge_dim=5)'
    assert layer(torch.randn(6, 16), torch.randint(0, 6, (2, 20)),
                 torch.randn(20, 5)).shape == (6, 8)


def test_get_degree_histogram_over_two_batches():
    from types import SimpleNamespace
    from pytorch_geometric_amd.nn import PNAConv
    a = SimpleNamespace(edge_index=torch.tensor([[0, 1, 2, 3], [1, 1, 1, 0]]), num_nodes=5)
    b = SimpleNamespace(edge_index=torch.tensor([[0, 1], [2, 2]]), num_nodes=3)
    # in-degrees: a = [1, 3, 0, 0, 0], b = [0, 0, 2]
    assert PNAConv.get_degree_histogram([a, b]).tolist() == [5, 1, 1, 1]
    assert PNAConv.get_degree_histogram([b, a]).tolist() == [5, 1, 1, 1]
    assert PNAConv.get_degree_histogram([b]).tolist() == [2, 0, 1]
    assert PNAConv.get_degree_histogram([]).tolist() == [0]


def test_the_envelope_and_the_registered_operator():
    import pytorch_geometric_amd.ops as ops
    from pytorch_geometric_amd import _build, _native
    assert 'pna_aggregate' in ops.OPS and 'pna_aggregate_backward' in ops.OPS
    assert str(torch.ops.pyg_amd.pna_aggregate.default._schema) == (
        'pyg_amd::pna_aggregate(Tensor p_src, Tensor p_dst, Tensor? edge_attr, Tensor? wc, '
        'Tensor rowptr, Tensor col, Tensor? edge_id, SymInt stats) -> (Tensor, Tensor)')
    assert _native.PNA_STATS == ('mean', 'min', 'max', 'std')
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    ok = _native.pna_supported
    assert ok(1) and ok(512) and not ok(513) and not ok(0)
    assert ok(128, 32) and not ok(128, 33) and not ok(129, 32)
    assert ok(512, 8) and not ok(512, 9) and ok(256, 16) and not ok(257, 16)


def test_entry_points_reject_bad_arguments_before_any_device_work():
    import ctypes
    from _util import csr_arg
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    dev = ctypes.c_void_p(16)   # (never dereferenced: every call below is rejected or launches nothing)

    def fwd(g, W=8, De=0, stats=15):
        return lib.pygamd_pna_forward(g, None, dev, 8, dev, 8, None, None, 9, W, De, stats, dev,
                                      dev, None, 0, None)

    def bwd(g, W=8, De=0, stats=15):
        return lib.pygamd_pna_backward(g, None, dev, 8, None, None, dev, 7, W, De, stats, dev,
                                       None, None, None, 0, None)

    assert fwd(None) == 1 and bwd(None) == 1
    empty = dict(rowptr=dev, col=dev, idx_dtype=1, n_rows=0, hub_threshold=1024, hub_chunk=256)
    assert fwd(csr_arg(**empty)) == 0 and bwd(csr_arg(**empty)) == 0      # no rows: nothing to launch
    assert fwd(csr_arg(**empty), stats=0) == 1 and bwd(csr_arg(**empty), stats=16) == 1
    assert fwd(csr_arg(**dict(empty, idx_dtype=5))) == 1
    assert bwd(csr_arg(**dict(empty, n_hub=0, n_chunks=3))) == 1         # chunks without hub rows
    assert fwd(csr_arg(**empty), W=513) == 2 and bwd(csr_arg(**empty), W=64, De=33) == 2
