"""nn.GENConv, nn.norm.MessageNorm and nn.models.DeepGCNLayer on host tensors: every recorded
reference case (tests/golden/golden_gen_v1.pt), the state-dict keys, ``__repr__``, the constructor
errors, the float32 composition against the float64 restatement, and the argument checks of the
``pygamd_gen_*`` entry points.  No GPU needed."""
import pytest
import torch

import _gen_ref as R
from _util import assert_close, assert_close_scaled


@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_host_tensors(name):
    G = R.load_golden()
    layer = R.check_class_case(G, name, 'cpu')
    assert repr(layer) == G['cases'][name]['repr']


def test_golden_stack_on_host_tensors():
    R.check_stack(R.load_golden(), 'cpu')


def test_state_dicts_load_both_ways_with_the_reference_keys():
    from pytorch_geometric_amd.nn import GENConv
    G = R.load_golden()
    for name in R.CASES:
        case = G['cases'][name]
        layer = R.make_layer(case)                      # reference -> this package (strict)
        back = layer.state_dict()                       # and what this package writes ...
        assert list(back) == list(case['state'])        # ... has the reference's keys, in order,
        for k, v in case['state'].items():              # shapes and dtypes
            assert back[k].shape == v.shape and back[k].dtype == v.dtype, (name, k)
            assert torch.equal(back[k], v)
    multi = GENConv((16, 12), 8, aggr=['softmax', 'mean', 'max'], edge_dim=5, bias=True,
                    msg_norm=True, num_layers=3, norm='batch')
    assert list(multi.state_dict()) == G['multi']['keys']
    assert repr(multi) == G['multi']['repr']
    assert multi.lin_aggr_out.weight.shape == (8, 24)


def test_defaults_and_aliases():
    from pytorch_geometric_amd.nn import GENConv, PowerMeanAggregation, SoftmaxAggregation
    layer = GENConv(8, 8)
    assert type(layer.aggr_module) is SoftmaxAggregation and layer.aggr_module.t == 1.0
    assert not layer.aggr_module.learn and not layer.aggr_module.semi_grad
    assert layer.eps == 1e-7 and layer.mlp[0].bias is None            # bias = False
    assert not any(hasattr(layer, n) for n in ('lin_src', 'lin_edge', 'lin_dst', 'lin_aggr_out',
                                               'msg_norm'))
    assert [type(m).__name__ for m in layer.mlp] == ['Linear', 'BatchNorm1d', 'ReLU', 'Dropout',
                                                     'Linear']
    assert layer.mlp[0].weight.shape == (16, 8)                        # expansion = 2
    sg = GENConv(8, 8, aggr='softmax_sg', t=0.3)
    assert sg.aggr == 'softmax' and sg.aggr_module.semi_grad and sg.aggr_module.t == 0.3
    pw = GENConv(8, 8, aggr='power', p=2.0, learn_p=True)
    assert pw.aggr == 'powermean' and type(pw.aggr_module) is PowerMeanAggregation
    assert list(pw.state_dict())[0] == 'aggr_module.p' and float(pw.aggr_module.p.detach()) == 2.0
    kw = GENConv(8, 8, t=5.0, aggr_kwargs=dict(t=0.25, learn=True, channels=8))
    assert kw.aggr_module.t.shape == (8, ) and float(kw.aggr_module.t[0].detach()) == 0.25
    assert GENConv(8, 8, edge_dim=8).edge_dim == 8 and not hasattr(GENConv(8, 8, edge_dim=8),
                                                                   'lin_edge')
    for norm, cls in (('layer', 'LayerNorm'), ('instance', 'InstanceNorm1d'), (None, 'ReLU')):
        assert type(GENConv(8, 8, norm=norm).mlp[1]).__name__ == cls
    assert len(GENConv(8, 8, num_layers=1).mlp) == 1


def test_constructor_errors():
    from pytorch_geometric_amd.nn import GENConv
    with pytest.raises(NotImplementedError, match='Normalization layer "group" not supported'):
        GENConv(8, 8, norm='group')
    with pytest.raises(ValueError, match="Cannot enable 'semi_grad'"):
        GENConv(8, 8, aggr='softmax_sg', learn_t=True)
    with pytest.raises(ValueError, match="Cannot set 'channels' greater than '1'"):
        GENConv(8, 8, aggr_kwargs=dict(channels=8))
    with pytest.raises(ValueError, match='flow'):
        GENConv(8, 8, flow='sideways')
    layer = GENConv(8, 8)
    x, ei = torch.randn(10, 8), torch.randint(0, 10, (2, 30))
    with pytest.raises(AssertionError):                  # width of edge_attr without lin_edge
        layer(x, ei, edge_attr=torch.randn(30, 5))


def test_reset_parameters():
    from pytorch_geometric_amd.nn import GENConv
    layer = GENConv((8, 6), 4, learn_t=True, t=0.3, edge_dim=3, msg_norm=True,
                    learn_msg_scale=True)
    before = {k: v.clone() for k, v in layer.state_dict().items()}
    layer.aggr_module.t.data.fill_(9.0)
    layer.msg_norm.scale.data.fill_(9.0)
    layer.reset_parameters()
    assert float(layer.aggr_module.t.detach()) == pytest.approx(0.3)
    assert float(layer.msg_norm.scale.detach()) == 1.0
    for k in ('lin_src.weight', 'lin_edge.weight', 'lin_dst.weight', 'mlp.0.weight'):
        assert not torch.equal(layer.state_dict()[k], before[k]), k


def test_message_norm_matches_its_golden():
    from pytorch_geometric_amd.nn import MessageNorm
    from pytorch_geometric_amd.nn.norm import MessageNorm as FromNorm
    assert MessageNorm is FromNorm
    G = R.load_golden()
    case = G['msg_norm']
    mod = MessageNorm(learn_scale=True)
    assert list(mod.state_dict()) == list(case['state']) == ['scale']
    mod.load_state_dict(case['state'])
    x, msg = case['x'].clone().requires_grad_(True), case['msg'].clone().requires_grad_(True)
    out = mod(x, msg)
    gx, gm, gs = torch.autograd.grad(out, [x, msg, mod.scale], case['grad_out'])
    assert_close(out, case['out'], what='out')
    assert_close(gx, case['grad_x'][0], what='grad_x')
    assert_close(gm, case['grad_x'][1], what='grad_msg')
    assert_close(gs, case['grad_params']['scale'], what='grad_scale')
    assert_close(mod(x, msg, p=1.0), case['out_p1'], what='p = 1')
    assert repr(mod) == G['reprs']['msg_norm'] and repr(MessageNorm()) == G['reprs']['msg_norm_fixed']
    assert not MessageNorm().scale.requires_grad and float(MessageNorm().scale.detach()) == 1.0


def test_deep_gcn_layer_blocks_match_their_goldens():
    from pytorch_geometric_amd.nn import DeepGCNLayer
    from pytorch_geometric_amd.nn.models import DeepGCNLayer as FromModels
    assert DeepGCNLayer is FromModels
    G = R.load_golden()
    for block, ref in G['blocks']['out'].items():
        layer = R.make_stack(block)[0]
        layer.load_state_dict(G['blocks']['state'])
        assert_close(layer(G['x'], G['edge_index']), ref, what=block)
    assert repr(R.make_stack('dense')[0]) == G['reprs']['deep']
    with pytest.raises(AssertionError):
        DeepGCNLayer(block='skip')
    # dropout acts in training only; ckpt_grad recomputes the convolution and changes no value
    layer = R.make_stack('res')[0]
    layer.load_state_dict(G['blocks']['state'])
    layer.dropout = 0.5
    layer.eval()
    assert_close(layer(G['x'], G['edge_index']), G['blocks']['out']['res'], what='eval')
    layer.train()
    assert not torch.allclose(layer(G['x'], G['edge_index']), G['blocks']['out']['res'])
    layer.dropout = 0.0
    grads = []
    for ckpt in (False, True):
        layer.ckpt_grad = ckpt
        x = G['x'].detach().clone().requires_grad_(True)
        layer(x, G['edge_index']).sum().backward()
        grads.append(x.grad)
    assert_close(grads[1], grads[0], what='ckpt_grad')   # (the same terms in another order)
    layer.reset_parameters()


def test_float32_composition_against_float64():
    """The yardstick the GPU tests use for ``grad_t``: the float32 torch composition (gather ->
    message -> softmax -> sum) is itself within the project's 2e-5 of the float64 restatement."""
    G = R.load_golden()
    ei, n = G['edge_index'], G['x'].size(0)
    g = torch.Generator().manual_seed(3)
    x = G['x']
    ea = torch.randn(ei.size(1), 3, generator=g)
    W, b = torch.randn(16, 3, generator=g) * 0.5, torch.randn(16, generator=g) * 0.1
    go = torch.randn(n, 16, generator=g)
    for t0 in (torch.tensor([1.0]), torch.tensor([-2.0]), torch.rand(16, generator=g) + 0.5):
        res = {}
        for dt in (torch.float32, torch.float64):
            leaves = [v.to(dt).requires_grad_(True) for v in (x, ea, W, b, t0)]
            out = R.gen_aggregate(*leaves[:4], leaves[4], ei, n)
            res[dt] = [out] + list(torch.autograd.grad(out, leaves, go.to(dt)))
        for got, ref, what in zip(res[torch.float32], res[torch.float64],
                                  ('out', 'grad_x', 'grad_edge_attr', 'grad_W', 'grad_b')):
            assert_close_scaled(got, ref.float(), what=what)
        abs_terms = R.grad_t_abs_terms(*[v.double() for v in (x, ea, W, b, t0)], ei, n,
                                       go.double())
        err = (res[torch.float32][5].double() - res[torch.float64][5]).abs()
        assert bool((err <= 2e-5 * abs_terms).all())


def test_entry_points_reject_bad_arguments_without_a_device():
    """pygamd_gen_*: status 1 / 2 / 3 before any device work, 0 for a handle without rows."""
    import ctypes
    from _util import csr_arg
    from pytorch_geometric_amd import _build, _lib, _native
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    dev = ctypes.c_void_p(16)   # (never dereferenced: every call below is rejected or launches nothing)
    NONE, WIDE, LIN = _native.GEN_EDGE_NONE, _native.GEN_EDGE_WIDE, _native.GEN_EDGE_LINEAR

    def fwd(g, F=8, De=0, mode=NONE, ea=None, w=None, t_len=1, ld=8, ws=None, ws_bytes=0):
        return lib.pygamd_gen_forward(g, None, dev, ld, mode, ea, w, None, dev, t_len, 1e-7, 9, F,
                                      De, 0, dev, dev, ws, ws_bytes, None)

    def bwd(g, F=8, De=0, mode=NONE, ea=None, w=None, t_len=1, want=0, ge=None, gw=None,
            ws=None, ws_bytes=0):
        return lib.pygamd_gen_backward(g, None, dev, 8, mode, ea, w, None, dev, t_len, 1e-7, 0,
                                       dev, 7, F, De, want, dev, ge, gw, None, ws, ws_bytes, None)

    assert fwd(None) == 1 and bwd(None) == 1
    empty = dict(rowptr=dev, col=dev, idx_dtype=1, n_rows=0, hub_threshold=1024, hub_chunk=256)
    assert fwd(csr_arg(**empty)) == 0 and bwd(csr_arg(**empty)) == 0      # no rows: nothing to launch
    assert fwd(csr_arg(**dict(empty, idx_dtype=5))) == 1
    assert bwd(csr_arg(**dict(empty, n_hub=0, n_chunks=3))) == 1          # chunks without hub rows
    assert fwd(csr_arg(**empty), F=513) == 2 and bwd(csr_arg(**empty), F=64, De=33, mode=LIN) == 2
    assert fwd(csr_arg(**empty), F=512, De=16, mode=LIN) == 2             # F * De > 4096
    assert fwd(csr_arg(**empty), mode=3) == 1 and bwd(csr_arg(**empty), mode=-1) == 1
    assert fwd(csr_arg(**empty), De=3, mode=WIDE) == 1                    # De needs the linear mode
    assert fwd(csr_arg(**empty), De=0, mode=LIN) == 1
    assert fwd(csr_arg(**empty), t_len=5) == 1 and fwd(csr_arg(**empty), t_len=8) == 0
    assert fwd(csr_arg(**empty), ld=7) == 1                               # ld_src < F
    rows = dict(empty, n_rows=4)
    assert fwd(csr_arg(**rows), mode=WIDE) == 1                           # wide without edge_attr
    assert fwd(csr_arg(**rows), mode=NONE, ea=dev) == 1                   # edge_attr without a mode
    assert fwd(csr_arg(**rows), De=3, mode=LIN, ea=dev) == 1              # linear without a weight
    assert bwd(csr_arg(**rows), mode=WIDE, ea=dev, want=1) == 1           # wanted, nowhere to write
    assert bwd(csr_arg(**rows), mode=NONE, want=1, ge=dev) == 1           # nothing to differentiate
    assert bwd(csr_arg(**rows), De=3, mode=LIN, ea=dev, w=dev) == 1       # no grad_weight
    assert bwd(csr_arg(**rows), De=3, mode=LIN, ea=dev, w=dev, gw=dev) == 3   # partials need room
    hub = dict(rows, hub_rows=dev, hub_chunk_ptr=dev, n_hub=1, n_chunks=5)
    assert fwd(csr_arg(**hub)) == 3 and fwd(csr_arg(**hub), ws=dev, ws_bytes=5 * 4 * 8 * 4 - 1) == 3
    n = ctypes.c_size_t(0)
    assert lib.pygamd_gen_workspace_bytes(5, 8, 0, ctypes.byref(n)) == 0 and n.value == 5 * 4 * 8 * 4
    assert lib.pygamd_gen_workspace_bytes(0, 8, 3, ctypes.byref(n)) == 0 and n.value == 512 * 32 * 4
    assert lib.pygamd_gen_workspace_bytes(0, 8, 0, None) == 1
    assert lib.pygamd_gen_workspace_bytes(0, 1024, 0, ctypes.byref(n)) == 2
    assert lib.pygamd_gen_supported(512, 8) == 1 and lib.pygamd_gen_supported(512, 9) == 0
    assert lib.pygamd_gen_supported(513, 0) == 0 and lib.pygamd_gen_supported(64, 33) == 0
    assert _native.gen_supported(128, 32) and not _native.gen_supported(1024)


def test_operators_are_registered():
    import pytorch_geometric_amd.ops as ops
    assert 'gen_aggregate' in ops.OPS and 'gen_aggregate_backward' in ops.OPS
    schema = str(torch.ops.pyg_amd.gen_aggregate.default._schema)
    assert schema.startswith('pyg_amd::gen_aggregate(Tensor x_src, Tensor? edge_attr, Tensor? weight, '
                             'Tensor? bias, Tensor t, Tensor rowptr, Tensor col, Tensor? edge_id')
    assert schema.endswith('-> (Tensor, Tensor)')
