"""CGConv: what the host and the GPU tests share.  The recorded reference cases of
tests/golden/golden_cg_v1.pt (tests/golden/make_golden_cg.py) and the torch restatement of the
aggregate in the dtype of its inputs, in the reference's UNSPLIT form (``cat`` then ``Linear`` per
edge, cg_conv.py:93-98), so that the split of both ``Linear`` into destination, source and edge
columns the kernels of csrc/cg.hip rest on is itself under test:

    out[i] = x_dst[i] + aggr_{k: dst_k = i} sigmoid(lin_f(z_k)) * softplus(lin_s(z_k))
    z_k = cat[x_dst[dst_k], x_src[src_k], a_k]
"""
import os

import torch
import torch.nn.functional as F

CASES = ['defaults', 'no_bias', 'dim', 'dim_wide', 'mean', 'max', 'batch_norm', 'pair', 'pair_dim']
FUSED_CASES = [c for c in CASES if c != 'max']

_GOLDEN = []


def load_golden():
    """tests/golden/golden_cg_v1.pt, loaded once and never modified."""
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_cg_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def _lin(x, wb):
    w, b = wb
    out = x @ w.t()
    return out if b is None else out + b


def cg_aggregate(x_src, x_dst, edge_attr, lin_f, lin_s, edge_index, n_dst, aggr='add',
                 residual=True, flow='source_to_target'):
    """The aggregate (with the residual, unless ``residual`` is false) in the dtype of its inputs;
    ``lin_f``, ``lin_s = (W [F, F_dst + F_src + D], b | None)``, ``aggr`` in add / mean / max."""
    j, i = (0, 1) if flow == 'source_to_target' else (1, 0)
    src, dst = edge_index[j].long(), edge_index[i].long()
    z = [x_dst[dst], x_src[src]] + ([] if edge_attr is None else [edge_attr])
    z = torch.cat(z, dim=-1)
    msg = torch.sigmoid(_lin(z, lin_f)) * F.softplus(_lin(z, lin_s))
    width = msg.size(1)
    if aggr == 'max':
        out = msg.new_zeros(n_dst, width).scatter_reduce(
            0, dst.view(-1, 1).expand(-1, width), msg, 'amax', include_self=False)
    else:
        out = msg.new_zeros(n_dst, width).index_add(0, dst, msg)
        if aggr == 'mean':
            out = out / torch.bincount(dst, minlength=n_dst).clamp(min=1).to(out.dtype).view(-1, 1)
    return out + x_dst[:n_dst] if residual else out


def cg_layer(state, x_src, x_dst, edge_attr, edge_index, aggr='add', flow='source_to_target'):
    """The whole layer from a state dict (the reference's keys), in the dtype of its tensors;
    ``bn.*`` present: batch norm in training mode (biased batch statistics, eps 1e-5)"""
    lin_f = (state['lin_f.weight'], state.get('lin_f.bias'))
    lin_s = (state['lin_s.weight'], state.get('lin_s.bias'))
    n_dst = x_dst.size(0)
    bn = 'bn.weight' in state
    out = cg_aggregate(x_src, x_dst, edge_attr, lin_f, lin_s, edge_index, n_dst, aggr,
                       residual=not bn, flow=flow)
    if bn:
        mean, var = out.mean(dim=0), out.var(dim=0, unbiased=False)
        out = (out - mean) / torch.sqrt(var + 1e-5) * state['bn.weight'] + state['bn.bias']
        out = out + x_dst
    return out


def make_layer(case):
    from pytorch_geometric_amd.nn import CGConv
    layer = CGConv(case['channels'], **case['kwargs'])
    assert list(layer.state_dict()) == list(case['state'])
    layer.load_state_dict(case['state'], strict=True)
    layer.fuse = True    # the fused route wherever its conditions hold, whatever the switch says
    return layer.train()


def case_inputs(G, case, device, index_dtype=torch.int64, dtype=torch.float32):
    """``(xs, edge_index, edge_attr | None)`` of a recorded case as fresh leaves on ``device``"""
    pair = case['mode'] == 'pair'
    xs = [G['x'].detach().clone().to(device, dtype).requires_grad_(True)]
    if pair:
        width = case['channels'][1]
        xs.append(G['x_dst'][:, :width].detach().clone().to(device, dtype).requires_grad_(True))
    ei = (G['edge_index_pair'] if pair else G['edge_index']).to(device).to(index_dtype)
    ea = None
    if 'edge_attr' in case:
        ea = case['edge_attr'].detach().clone().to(device, dtype).requires_grad_(True)
    return xs, ei, ea


def check_restatement_case(G, name):
    """The restatement in float32 against one recorded case, at ``check_class_case``'s bounds"""
    case = G['cases'][name]
    xs, ei, ea = case_inputs(G, case, 'cpu')
    state = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v)
             for k, v in case['state'].items()}
    out = cg_layer(state, xs[0], xs[-1], ea, ei, aggr=case['kwargs'].get('aggr', 'add'))
    leaves = xs + ([] if ea is None else [ea])
    names = list(case['grad_params'])
    grads = torch.autograd.grad(out, leaves + [state[n] for n in names], case['grad_out'])
    _compare(name, case, out, grads, len(xs), ea is not None, names)


def _compare(name, case, out, grads, n_x, has_ea, names):
    from _util import assert_close
    assert_close(out, case['out'], what=f'{name} out')
    for g, ref in zip(grads[:n_x], case['grad_x']):
        assert_close(g, ref, what=f'{name} grad_x')
    if has_ea:
        assert_close(grads[n_x], case['grad_edge_attr'], what=f'{name} grad_edge_attr')
    for n, g in zip(names, grads[n_x + int(has_ea):]):
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'{name} grad {n}')


def check_class_case(G, name, device, index_dtype=torch.int64):
    """This package's class with the reference's state dict against one recorded case: ``out``,
    ``grad_x`` and ``grad_edge_attr`` at 1e-5, parameter gradients at 5e-5 (the tolerances of
    ``_resgated_ref.check_class_case``); the running statistics of a batch norm too."""
    from _util import assert_close
    case = G['cases'][name]
    layer = make_layer(case).to(device)
    xs, ei, ea = case_inputs(G, case, device, index_dtype)
    out = layer(xs[0] if len(xs) == 1 else (xs[0], xs[1]), ei, edge_attr=ea)
    params = [(n, p) for n, p in layer.named_parameters() if p.requires_grad]
    assert [n for n, _ in params] == list(case['grad_params']), name
    leaves = xs + ([] if ea is None else [ea])
    grads = torch.autograd.grad(out, leaves + [p for _, p in params], case['grad_out'].to(device))
    _compare(name, case, out, grads, len(xs), ea is not None, [n for n, _ in params])
    for key, ref in case.get('bn_after', {}).items():
        assert_close(layer.state_dict()[key], ref, what=f'{name} {key}')
    return layer


def make_stack():
    from pytorch_geometric_amd.nn import CGConv
    layers = torch.nn.ModuleList([CGConv(16, dim=3), CGConv(16)])
    for layer in layers:   # (as make_layer)
        layer.fuse = True
    return layers


def check_stack(G, device, index_dtype=torch.int64):
    """The two-layer stack against its record, judged relative to each tensor's scale at the
    project's 2e-5 (``assert_close_scaled``, the bound of deep-model gradients).  Two unnormalised
    sums in a row give outputs up to 5.4e3 and parameter gradients up to 1.3e4 whose entries are
    sums of hundreds of cancelling terms, so a per-element relative bound has no meaning here: the
    recorded float32 result ITSELF differs from the float64 restatement by up to 4.8e-6 of the
    tensor's scale (``1.lin_f.weight``: 1.7e-2 at a scale of 3.5e3; ``0.lin_f.weight``: 2.7e-3
    at 3.0e3, measured on the CPU), far past 5e-5 of a small entry."""
    from _util import assert_close_scaled
    case = G['stack']
    layers = make_stack()
    assert list(layers.state_dict()) == list(case['state'])
    layers.load_state_dict(case['state'], strict=True)
    layers = layers.to(device)
    x = G['x'].detach().clone().to(device).requires_grad_(True)
    ea = case['edge_attr'].detach().clone().to(device).requires_grad_(True)
    ei = G['edge_index'].to(device).to(index_dtype)
    h = layers[1](layers[0](x, ei, edge_attr=ea).relu(), ei)
    params = [(n, p) for n, p in layers.named_parameters() if p.requires_grad]
    assert [n for n, _ in params] == list(case['grad_params'])
    grads = torch.autograd.grad(h, [x, ea] + [p for _, p in params], case['grad_out'].to(device))
    assert_close_scaled(h, case['out'], what='stack out')
    assert_close_scaled(grads[0], case['grad_x'][0], what='stack grad_x')
    assert_close_scaled(grads[1], case['grad_edge_attr'], what='stack grad_edge_attr')
    for (n, _), g in zip(params, grads[2:]):
        assert_close_scaled(g, case['grad_params'][n], what=f'stack grad {n}')
    return layers
