"""TransformerConv with edge features: what the host and the GPU tests of the fused-edge route
share.  The layer's restatement is ``_transformer_ref.conv`` (it takes ``edge_attr``); this module
adds the recorded cases of tests/golden/golden_transformer_edge_v1.pt, which also hold the
gradient of ``edge_attr``, and the float64 restatement of the NODE the kernels implement:

    s[k,h]         = scale <q[i,h,:], key[j,h,:]> + <b[i,h,:], a[k,:]>
    alpha          = softmax over the destination's edges (maximum subtracted, 1e-16 on the denominator)
    out_nodes[i,h] = sum_k alpha[k,h] value[j,h,:]       z[i,h] = sum_k alpha[k,h] a[k,:]
"""
import math
import os

import torch

CASES = ['e', 'e_wide', 'e_mean', 'e_beta', 'e_noroot', 'e_nobias', 'e_pair', 'e_attention']

_GOLDEN = []


def load_golden():
    """tests/golden/golden_transformer_edge_v1.pt, loaded once and never modified."""
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_transformer_edge_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def case_inputs(G, case):
    xs = [G['x']] + ([G['x_dst']] if case['pair'] else [])
    ei = G['edge_index_pair'] if case['pair'] else G['edge_index']
    return xs, ei, G['edge_attr'][:, :case['kwargs']['edge_dim']].contiguous()


def attend_edge(q, k, v, a, b, edge_index, n_dst, scale=None):
    """(out_nodes [n_dst, H, C], z [n_dst, H, De], alpha [E, H] in edge order) for q, b with at
    least n_dst rows, k, v [N_src, H, C] and a [E, De]."""
    H, C = q.shape[1:]
    scale = 1.0 / math.sqrt(C) if scale is None else scale
    src, dst = edge_index[0].long(), edge_index[1].long()
    s = scale * (q[dst] * k[src]).sum(-1) + (b[dst] * a.unsqueeze(1)).sum(-1)
    top = s.new_full((n_dst, H), float('-inf')).scatter_reduce(
        0, dst.view(-1, 1).expand_as(s), s.detach(), 'amax', include_self=True)
    num = (s - top[dst]).exp()
    den = s.new_zeros(n_dst, H).index_add(0, dst, num) + 1e-16
    alpha = num / den[dst]
    out = v.new_zeros(n_dst, H, C).index_add(0, dst, alpha.unsqueeze(-1) * v[src])
    z = a.new_zeros(n_dst, H, a.size(1)).index_add(0, dst, alpha.unsqueeze(-1) * a.unsqueeze(1))
    return out, z, alpha


def check_class_case(G, name, device, fuse_edge=True, index_dtype=torch.int64):
    """This package's TransformerConv with the reference's state dict against one recorded case,
    at the tolerances of ``_transformer_ref.check_class_case``: ``out`` / ``grad_x`` /
    ``grad_edge_attr`` / attention weights at 1e-5, parameter gradients at 5e-5."""
    from pytorch_geometric_amd.nn import TransformerConv
    from _util import assert_close
    case = G['cases'][name]
    kw = dict(case['kwargs'])
    layer = TransformerConv(kw.pop('in_channels'), **kw)
    assert list(layer.state_dict()) == list(case['state']), name
    layer.load_state_dict(case['state'])
    layer = layer.to(device).eval()
    layer.fuse_edge = fuse_edge
    xs, ei, ea = case_inputs(G, case)
    xs = [t.to(device).requires_grad_(True) for t in xs]
    ea = ea.to(device).requires_grad_(True)
    res = layer(tuple(xs) if case['pair'] else xs[0], ei.to(device).to(index_dtype), edge_attr=ea,
                return_attention_weights=True if 'attention' in case else None)
    out, att = res if 'attention' in case else (res, None)
    params = list(layer.named_parameters())
    # (without root_weight lin_skip exists but is unused: no gradient here, none recorded)
    grads = torch.autograd.grad(out, xs + [ea] + [p for _, p in params],
                                case['grad_out'].to(device), allow_unused=True)
    nx = len(xs)
    assert_close(out, case['out'], what=f'{name} out')
    for g, ref in zip(grads[:nx], case['grad_x']):
        assert_close(g, ref, what=f'{name} grad_x')
    assert_close(grads[nx], case['grad_edge_attr'], what=f'{name} grad_edge_attr')
    got = {n: g for (n, _), g in zip(params, grads[nx + 1:]) if g is not None}
    assert list(got) == list(case['grad_params']), name
    for n, g in got.items():
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'{name} grad {n}')
    if att is not None:
        assert torch.equal(att[0].cpu().long(), case['attention'][0]), f'{name}: edge list'
        assert_close(att[1], case['attention'][1], what=f'{name} attention')
    return layer
