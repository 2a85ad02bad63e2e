"""GENConv: what the host and the GPU tests share.  The recorded reference cases of
tests/golden/golden_gen_v1.pt (tests/golden/make_golden_gen.py) and the float64 restatement of the
NODE the kernels of csrc/gen.hip implement:

    m_k    = relu(x_src[src_k] + e_k) + eps_msg,   e_k = 0 | edge_attr[k] | W edge_attr[k] + b
    out[i] = sum_{k: dst_k = i} alpha_k m_k,   alpha = softmax over the slots of i of t * m (per column)
"""
import os

import torch

CASES = ['defaults', 'learn_t', 't_half', 'softmax_sg', 'wide_edge', 'edge_dim', 'edge_dim_bias',
         'lin_src_dst', 'pair', 'pair_none', 'msg_norm', 'powermean', 'mean']
SOFTMAX_CASES = [c for c in CASES if c not in ('powermean', 'mean')]

_GOLDEN = []


def load_golden():
    """tests/golden/golden_gen_v1.pt, loaded once and never modified."""
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_gen_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def gen_message(x_src, edge_attr, W, b, src, eps_msg=1e-7):
    """``(m [E, F], pre [E, F])``: the message and the ReLU's argument, in the dtype of the inputs"""
    pre = x_src[src.long()]
    if edge_attr is not None:
        e = edge_attr
        if W is not None:
            e = e @ W.t()
            if b is not None:
                e = e + b
        pre = pre + e
    return pre.relu() + eps_msg, pre


def segment_softmax_sum(m, t, dst, n_dst, semi_grad=False):
    """``sum_k alpha_k m_k`` per destination with ``alpha`` the softmax of ``t * m`` (``t``: a
    float or a tensor of 1 or F values), the reference's formula (utils/_softmax.py): the maximum
    is subtracted and 1e-16 added to the sum.  Returns ``(out, alpha)``."""
    dst = dst.long()
    F = m.size(1)
    idx = dst.view(-1, 1).expand(-1, F)
    tt = t.reshape(1, -1) if isinstance(t, torch.Tensor) else t
    with torch.set_grad_enabled(torch.is_grad_enabled() and not semi_grad):
        logits = m * tt
        top = logits.new_zeros(n_dst, F).scatter_reduce(0, idx, logits.detach(), 'amax',
                                                        include_self=False)
        e = (logits - top[dst]).exp()
        alpha = e / (e.new_zeros(n_dst, F).index_add(0, dst, e)[dst] + 1e-16)
    return m.new_zeros(n_dst, F).index_add(0, dst, m * alpha), alpha


def gen_aggregate(x_src, edge_attr, W, b, t, edge_index, n_dst, eps_msg=1e-7, semi_grad=False):
    """The node in the dtype of its inputs (float32: the torch composition gather -> message ->
    SoftmaxAggregation; float64: the reference value)."""
    m, _ = gen_message(x_src, edge_attr, W, b, edge_index[0], eps_msg)
    return segment_softmax_sum(m, t, edge_index[1], n_dst, semi_grad)[0]


def grad_t_abs_terms(x_src, edge_attr, W, b, t, edge_index, n_dst, grad_out, eps_msg=1e-7):
    """``sum_k |g alpha_k m_k (m_k - out)|`` per column (summed over the columns for a scalar
    ``t``): what the cancelling sum ``grad_t`` is judged against.  float64 inputs."""
    m, _ = gen_message(x_src, edge_attr, W, b, edge_index[0], eps_msg)
    dst = edge_index[1].long()
    out, alpha = segment_softmax_sum(m, t, dst, n_dst)
    terms = (grad_out[dst] * alpha * m * (m - out[dst])).abs().sum(0)
    scalar = not isinstance(t, torch.Tensor) or t.numel() == 1
    return terms.sum() if scalar else terms


def make_layer(case):
    from pytorch_geometric_amd.nn import GENConv
    cin, cout = case['channels']
    layer = GENConv(cin, cout, **case['kwargs'])
    assert list(layer.state_dict()) == list(case['state'])
    layer.load_state_dict(case['state'])
    return layer


def check_class_case(G, name, device, index_dtype=torch.int64):
    """This package's class with the reference's state dict against one recorded case: ``out``,
    ``grad_x`` and ``grad_edge_attr`` at 1e-5, parameter gradients at 5e-5 (the tolerances of
    ``_gin_ref.check_class_case``)."""
    from _util import assert_close
    case = G['cases'][name]
    layer = make_layer(case).to(device)
    mode = case['mode']
    xs = [G['x'].detach().clone().to(device).requires_grad_(True)]
    if mode == 'pair':
        xs.append(G['x_dst'].detach().clone().to(device).requires_grad_(True))
    ei = (G['edge_index'] if mode == 'one' else G['edge_index_pair']).to(device).to(index_dtype)
    size = None if mode == 'one' else (G['x'].size(0), G['x_dst'].size(0))
    x_in = xs[0] if mode == 'one' else (xs[0], xs[1] if mode == 'pair' else None)
    leaves = list(xs)
    ea = None
    if 'edge_attr' in case:
        ea = case['edge_attr'].detach().clone().to(device).requires_grad_(True)
        leaves.append(ea)
    out = layer(x_in, ei, edge_attr=ea, size=size)
    params = [(n, p) for n, p in layer.named_parameters() if p.requires_grad]
    assert [n for n, _ in params] == list(case['grad_params']), name
    grads = torch.autograd.grad(out, leaves + [p for _, p in params], case['grad_out'].to(device))
    assert_close(out, case['out'], what=f'{name} out')
    for g, ref in zip(grads[:len(xs)], case['grad_x']):
        assert_close(g, ref, what=f'{name} grad_x')
    if ea is not None:
        assert_close(grads[len(xs)], case['grad_edge_attr'], what=f'{name} grad_edge_attr')
    for (n, _), g in zip(params, grads[len(leaves):]):
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'{name} grad {n}')
    return layer


def make_stack(block='res+'):
    from pytorch_geometric_amd.nn import DeepGCNLayer, GENConv
    return torch.nn.ModuleList([
        DeepGCNLayer(GENConv(16, 16, learn_t=True, norm='layer'), torch.nn.LayerNorm(16),
                     torch.nn.ReLU(), block=block, dropout=0.0) for _ in range(2)])


def check_stack(G, device, index_dtype=torch.int64):
    from _util import assert_close
    case = G['stack']
    layers = make_stack()
    assert list(layers.state_dict()) == list(case['state'])
    layers.load_state_dict(case['state'])
    layers = layers.to(device)
    x = G['x'].detach().clone().to(device).requires_grad_(True)
    ei = G['edge_index'].to(device).to(index_dtype)
    h = x
    for layer in layers:
        h = layer(h, ei)
    params = [(n, p) for n, p in layers.named_parameters() if p.requires_grad]
    assert [n for n, _ in params] == list(case['grad_params'])
    grads = torch.autograd.grad(h, [x] + [p for _, p in params], case['grad_out'].to(device))
    assert_close(h, case['out'], what='stack out')
    assert_close(grads[0], case['grad_x'][0], atol=5e-5, rtol=5e-5, what='stack grad_x')
    for (n, _), g in zip(params, grads[1:]):
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'stack grad {n}')
    return layers
