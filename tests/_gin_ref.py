"""GINConv / GINEConv: what the host and the GPU tests share.  The recorded reference cases of
tests/golden/golden_gin_v1.pt (tests/golden/make_golden_gin.py) and the float64 restatement of the
NODE the kernels of csrc/gine.hip implement:

    out[i] = (1 + eps) * x_root[i] + sum_{k: dst_k = i} relu(x_src[src_k] + e_k)
    e_k = edge_attr[k]  (W is None)   or   W edge_attr[k] + b
"""
import os

import torch

CASES = ['gin', 'gin_eps', 'gin_pair', 'gin_pair_none', 'gine', 'gine_eps', 'gine_lin',
         'gine_lin_wide', 'gine_lin_pair', 'gine_pair_none']
GINE_CASES = [c for c in CASES if c.startswith('gine')]

_GOLDEN = []


def load_golden():
    """tests/golden/golden_gin_v1.pt, loaded once and never modified."""
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_gin_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def make_nn():
    return torch.nn.Sequential(torch.nn.Linear(16, 12), torch.nn.ReLU(), torch.nn.Linear(12, 8))


def gine_aggregate(x_src, x_root, eps, edge_attr, W, b, edge_index, n_dst, aggr='sum'):
    """The node in the dtype of its inputs; ``x_root`` (at least ``n_dst`` rows), ``eps``, ``W``
    and ``b`` may be None.  ``aggr='mean'`` (not a kernel route) divides the sum of the messages by
    the number of them."""
    src, dst = edge_index[0].long(), edge_index[1].long()
    e = edge_attr
    if W is not None:
        e = e @ W.t()
        if b is not None:
            e = e + b
    out = x_src.new_zeros(n_dst, x_src.size(1)).index_add(0, dst, (x_src[src] + e).relu())
    if aggr == 'mean':
        out = out / torch.bincount(dst, minlength=n_dst).clamp(min=1).to(out.dtype).unsqueeze(-1)
    if x_root is not None:
        out = out + (1 + (0 if eps is None else eps)) * x_root[:n_dst]
    return out


def gine_layer(x_src, x_dst, edge_attr, edge_index, state, n_dst, aggr='sum'):
    """GINEConv over ``nn = Sequential(Linear, ReLU, Linear)`` from a state dict, in the dtype of
    the inputs (``x_dst`` None: no self term)."""
    W, b = state.get('lin.weight'), state.get('lin.bias')
    h = gine_aggregate(x_src, x_dst, state['eps'], edge_attr, W, b, edge_index, n_dst, aggr)
    h = (h @ state['nn.0.weight'].t() + state['nn.0.bias']).relu()
    return h @ state['nn.2.weight'].t() + state['nn.2.bias']


def check_class_case(G, name, device, index_dtype=torch.int64):
    """This package's class with the reference's state dict against one recorded case: ``out``,
    ``grad_x`` and ``grad_edge_attr`` at 1e-5, parameter gradients at 5e-5 (the tolerances of
    ``_transformer_edge_ref.check_class_case``)."""
    from pytorch_geometric_amd.nn import GINConv, GINEConv
    from _util import assert_close
    case = G['cases'][name]
    gine = case['kind'] == 'gine'
    layer = (GINEConv if gine else GINConv)(make_nn(), **case['kwargs'])
    assert list(layer.state_dict()) == list(case['state']), name
    layer.load_state_dict(case['state'])
    layer = layer.to(device)
    mode = case['mode']
    xs = [G['x'].to(device).requires_grad_(True)]
    if mode == 'pair':
        xs.append(G['x_dst'].to(device).requires_grad_(True))
    ei = (G['edge_index'] if mode == 'one' else G['edge_index_pair']).to(device).to(index_dtype)
    size = None if mode == 'one' else (G['x'].size(0), G['x_dst'].size(0))
    x_in = xs[0] if mode == 'one' else (xs[0], xs[1] if mode == 'pair' else None)
    leaves = list(xs)
    if gine:
        ea = case['edge_attr'].to(device).requires_grad_(True)
        leaves.append(ea)
        out = layer(x_in, ei, edge_attr=ea, size=size)
    else:
        out = layer(x_in, ei, size=size)
    params = list(layer.named_parameters())
    assert [n for n, _ in params] == list(case['grad_params']), name
    grads = torch.autograd.grad(out, leaves + [p for _, p in params], case['grad_out'].to(device))
    assert_close(out, case['out'], what=f'{name} out')
    for g, ref in zip(grads[:len(xs)], case['grad_x']):
        assert_close(g, ref, what=f'{name} grad_x')
    if gine:
        assert_close(grads[len(xs)], case['grad_edge_attr'], what=f'{name} grad_edge_attr')
    for (n, _), g in zip(params, grads[len(leaves):]):
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'{name} grad {n}')
    return layer
