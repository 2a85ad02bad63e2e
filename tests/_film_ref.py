"""FiLMConv: what the host and the GPU tests share.  The recorded reference cases of
tests/golden/golden_film_v1.pt (tests/golden/make_golden_film.py) and the torch restatement of the
layer in the dtype of its inputs, in the reference's UNSPLIT form (film_conv.py:128-161): one mask
per relation, then a gather of both ends, ``gamma_i * x_j + beta_i``, the activation and a scatter
— so that the stacked projections, the relation-sorted handle and the per-edge mean normaliser the
kernels of csrc/film.hip rest on are themselves under test:

    out[i] = act(gs_i * lin_skip(x_i) + bs_i)
             + sum_r aggr_{k: dst_k = i, type_k = r} act(gamma_{r,i} * lins[r](x_src)[src_k] + beta_{r,i})
"""
import os

import torch

CASES = ['r1_default', 'r3_mean', 'r3_add', 'r3_empty_relation', 'r3_out_of_range', 'pair_r2',
         'act_none', 'custom_nn', 'r2_max', 'act_tanh']
GENERIC_CASES = ['r2_max', 'act_tanh']
FUSED_CASES = [c for c in CASES if c not in GENERIC_CASES]
ACTS = {'relu': torch.relu, 'none': None, 'tanh': torch.tanh}

_GOLDEN = []


def load_golden():
    """tests/golden/golden_film_v1.pt, loaded once and never modified."""
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_film_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def aggregate(msg, dst, n_dst, aggr):
    """``msg [E, F]`` reduced onto ``dst``: add / sum, mean or max (0 for a row without messages)"""
    width = msg.size(1)
    if aggr == 'max':
        return msg.new_zeros(n_dst, width).scatter_reduce(
            0, dst.view(-1, 1).expand(-1, width), msg, 'amax', include_self=False)
    out = msg.new_zeros(n_dst, width).index_add(0, dst, msg)
    if aggr == 'mean':
        out = out / torch.bincount(dst, minlength=n_dst).clamp(min=1).to(out.dtype).view(-1, 1)
    return out


def film_messages(h, g, residual, edge_index, edge_type, R, n_dst, aggr='add', act=torch.relu,
                  flow='source_to_target'):
    """The per-relation loop on node-level inputs: ``h [n_src, R * F]`` (relation ``r`` reads its
    column block), ``g [>= n_dst, R * 2F]`` (block ``r`` = ``[beta_r | gamma_r]``), ``residual
    [n_dst, F]`` or None.  ``edge_type`` None: every edge has relation 0."""
    F = h.size(1) // R
    j, i = (0, 1) if flow == 'source_to_target' else (1, 0)
    out = h.new_zeros(n_dst, F) if residual is None else residual
    for r in range(R):
        ei = edge_index if edge_type is None else edge_index[:, edge_type == r]
        src, dst = ei[j].long(), ei[i].long()
        beta, gamma = g[:, r * 2 * F:(r + 1) * 2 * F].split(F, dim=-1)
        msg = gamma[dst] * h[src, r * F:(r + 1) * F] + beta[dst]
        if act is not None:
            msg = act(msg)
        out = out + aggregate(msg, dst, n_dst, aggr)
    return out


def _film_net(state, prefix, x):
    """a film net from its state-dict entries: ``Linear`` (bias optional) or the custom
    ``Sequential(Linear, Tanh, Linear)``"""
    if prefix + 'weight' in state:
        out = x @ state[prefix + 'weight'].t()
        bias = state.get(prefix + 'bias')
        return out if bias is None else out + bias
    hid = torch.tanh(x @ state[prefix + '0.weight'].t() + state[prefix + '0.bias'])
    return hid @ state[prefix + '2.weight'].t() + state[prefix + '2.bias']


def film_layer(state, x_src, x_dst, edge_index, edge_type, R, aggr='mean', act='relu',
               flow='source_to_target', n_dst=None):
    """The whole layer from a state dict (the reference's keys), in the dtype of its tensors"""
    fn = ACTS[act]
    n_dst = x_dst.size(0) if n_dst is None else n_dst
    h = torch.cat([x_src @ state[f'lins.{r}.weight'].t() for r in range(R)], dim=1)
    g = torch.cat([_film_net(state, f'films.{r}.', x_dst) for r in range(R)], dim=1)
    F = h.size(1) // R
    beta, gamma = _film_net(state, 'film_skip.', x_dst).split(F, dim=-1)
    skip = gamma * (x_dst @ state['lin_skip.weight'].t()) + beta
    if fn is not None:
        skip = fn(skip)
    return film_messages(h, g, skip[:n_dst], edge_index, edge_type if R > 1 else None, R, n_dst,
                         aggr=aggr, act=fn, flow=flow)


def make_nn(case):
    from torch.nn import Linear, Sequential, Tanh
    if case['hidden'] is None:
        return None
    ic = case['in_channels']
    width = ic if isinstance(ic, int) else ic[1]
    return Sequential(Linear(width, case['hidden']), Tanh(),
                      Linear(case['hidden'], 2 * case['out_channels']))


def make_layer(case):
    from pytorch_geometric_amd.nn import FiLMConv
    act = {'relu': torch.nn.ReLU, 'none': lambda: None, 'tanh': torch.nn.Tanh}[case['act']]()
    layer = FiLMConv(case['in_channels'], case['out_channels'],
                     num_relations=case['num_relations'], nn=make_nn(case), act=act,
                     aggr=case['aggr'])
    assert list(layer.state_dict()) == list(case['state'])
    layer.load_state_dict(case['state'], strict=True)
    layer.fuse = True    # the fused route wherever its conditions hold, whatever the switch says
    return layer.train()


def case_inputs(G, case, device, index_dtype=torch.int64, dtype=torch.float32):
    """``(xs, edge_index, edge_type | None)`` of a recorded case as fresh leaves on ``device``"""
    pair = case['mode'] == 'pair'
    names = ('x_pair_src', 'x_pair_dst') if pair else ('x', )
    xs = [G[n].detach().clone().to(device, dtype).requires_grad_(True) for n in names]
    ei = (G['edge_index_pair'] if pair else G['edge_index']).to(device).to(index_dtype)
    et = case['edge_type']
    return xs, ei, None if et is None else et.to(device).to(index_dtype)


def _compare(name, case, out, grads, n_x, names):
    from _util import assert_close
    assert_close(out, case['out'], what=f'{name} out')
    for g, ref in zip(grads[:n_x], case['grad_x']):
        assert_close(g, ref, what=f'{name} grad_x')
    for n, g in zip(names, grads[n_x:]):
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'{name} grad {n}')


def check_restatement_case(G, name):
    """The restatement in float32 against one recorded case, at ``check_class_case``'s bounds"""
    case = G['cases'][name]
    xs, ei, et = case_inputs(G, case, 'cpu')
    state = {k: v.detach().clone().requires_grad_(True) for k, v in case['state'].items()}
    out = film_layer(state, xs[0], xs[-1], ei, et, case['num_relations'], aggr=case['aggr'],
                     act=case['act'])
    names = list(case['grad_params'])
    grads = torch.autograd.grad(out, xs + [state[n] for n in names], case['grad_out'])
    _compare(name, case, out, grads, len(xs), names)


def check_class_case(G, name, device, index_dtype=torch.int64):
    """This package's class with the reference's state dict against one recorded case: ``out`` and
    ``grad_x`` at 1e-5, parameter gradients at 5e-5 (the tolerances of
    ``_cg_ref.check_class_case``)."""
    case = G['cases'][name]
    layer = make_layer(case).to(device)
    xs, ei, et = case_inputs(G, case, device, index_dtype)
    out = layer(xs[0] if len(xs) == 1 else (xs[0], xs[1]), ei, et)
    params = [(n, p) for n, p in layer.named_parameters() if p.requires_grad]
    assert [n for n, _ in params] == list(case['grad_params']), name
    grads = torch.autograd.grad(out, xs + [p for _, p in params], case['grad_out'].to(device))
    _compare(name, case, out, grads, len(xs), [n for n, _ in params])
    return layer


def make_stack():
    from pytorch_geometric_amd.nn import FiLMConv
    layers = torch.nn.ModuleList([FiLMConv(12, 16, num_relations=3),
                                  FiLMConv(16, 8, num_relations=3)])
    for layer in layers:   # (as make_layer)
        layer.fuse = True
    return layers


def check_stack(G, device, index_dtype=torch.int64):
    """The two-layer stack against its record, relative to each tensor's scale at the project's
    2e-5 (``assert_close_scaled``, the bound of deep-model gradients)."""
    from _util import assert_close_scaled
    case = G['stack']
    layers = make_stack()
    assert list(layers.state_dict()) == list(case['state'])
    layers.load_state_dict(case['state'], strict=True)
    layers = layers.to(device)
    x = G['x'].detach().clone().to(device).requires_grad_(True)
    ei = G['edge_index'].to(device).to(index_dtype)
    et = case['edge_type'].to(device).to(index_dtype)
    out = layers[1](layers[0](x, ei, et), ei, et)
    params = [(n, p) for n, p in layers.named_parameters() if p.requires_grad]
    assert [n for n, _ in params] == list(case['grad_params'])
    grads = torch.autograd.grad(out, [x] + [p for _, p in params], case['grad_out'].to(device))
    assert_close_scaled(out, case['out'], what='stack out')
    assert_close_scaled(grads[0], case['grad_x'][0], what='stack grad_x')
    for (n, _), g in zip(params, grads[1:]):
        assert_close_scaled(g, case['grad_params'][n], what=f'stack grad {n}')
    return layers
