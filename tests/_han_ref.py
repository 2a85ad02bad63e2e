"""A plain-torch restatement of ``HANConv`` (torch_geometric/nn/conv/han_conv.py:34-183) and of its
node-level attention step on a stacked graph, evaluated in the dtype of its inputs (float64 in the
tests).  No package code: ``index_add_`` / ``scatter_reduce`` on CPU tensors."""
import torch
import torch.nn.functional as F


def attend(x_all, a_src, a_dst, col, row, types, slope, relu=True, mask=None):
    """``(out [n_rows, H * D], alpha [E, H])`` of the attention step on the stacked edge list
    ``(col, row)`` in the caller's edge order: ``x_all [S, H, D]``, ``a_src [n_cols, H]``, ``a_dst
    [n_rows, H]``, ``types = (row_begin, src_begin, val_shift)``.  The softmax is the reference's
    (maximum subtracted, 1e-16 on the denominator), so -inf / NaN / +inf scores behave as there.
    ``relu``: ``torch.relu`` on the result, or — ``mask`` given — the result times that mask."""
    row_begin, src_begin, val_shift = types
    col, row = col.long(), row.long()
    n_rows, H = a_dst.shape
    D = x_all.size(2)
    shift = torch.zeros_like(col)
    for e, s in enumerate(val_shift):   # the edge type of an edge is that of its column
        shift[(col >= src_begin[e]) & (col < src_begin[e + 1])] = s
    s = F.leaky_relu(a_src[col] + a_dst[row], slope)
    idx = row.view(-1, 1).expand(-1, H)
    top = s.new_full((n_rows, H), float('-inf')).scatter_reduce(0, idx, s.detach(), 'amax',
                                                                include_self=True)
    num = (s - top[row]).exp()
    den = s.new_zeros(n_rows, H).index_add_(0, row, num) + 1e-16
    alpha = num / den[row]
    msg = x_all[col + shift] * alpha.unsqueeze(-1)
    out = x_all.new_zeros(n_rows, H, D).index_add_(0, row, msg).reshape(n_rows, H * D)
    if mask is not None:
        out = out * mask.to(out.dtype)
    elif relu:
        out = torch.relu(out)
    return out, alpha


def group(xs, q, k_w, k_b):
    """han_conv.py:15-31"""
    if len(xs) == 0:
        return None, None
    out = torch.stack(xs)
    if out.numel() == 0:
        return out.view(0, out.size(-1)), None
    score = (q * torch.tanh(out @ k_w.t() + k_b).mean(1)).sum(-1)
    attn = F.softmax(score, dim=0)
    return torch.sum(attn.view(len(xs), 1, -1) * out, dim=0), attn


def layer(state, x_dict, edge_index_dict, heads, slope=0.2, flow='source_to_target'):
    """``(out_dict, beta_dict)`` of the layer with parameters ``state`` (the reference's state-dict
    keys; tensors that may require grad) in the dtype of the inputs.  ``flow='target_to_source'``
    is what ``propagate`` makes of the reference's call: row 1 of ``edge_index`` names the sending
    nodes (the edge type's destination type) and row 0 the aggregating ones."""
    W = state['q'].size(-1)
    H, D = heads, W // heads
    xn = {t: (x @ state[f'proj.{t}.weight'].t() + state[f'proj.{t}.bias']).view(-1, H, D)
          for t, x in x_dict.items()}
    outs = {t: [] for t in x_dict}
    for et, ei in edge_index_dict.items():
        key = '__'.join(et)
        x_src, x_dst = xn[et[0]], xn[et[-1]]
        a_src = (x_src * state[f'lin_src.{key}']).sum(-1)
        a_dst = (x_dst * state[f'lin_dst.{key}']).sum(-1)
        ei = ei.long()
        if flow == 'source_to_target':
            send, a_send, a_recv, j, i = x_src, a_src, a_dst, ei[0], ei[1]
        else:
            send, a_send, a_recv, j, i = x_dst, a_dst, a_src, ei[1], ei[0]
        types = ((0, a_recv.size(0)), (0, a_send.size(0)), (0, ))
        out, _ = attend(send, a_send, a_recv, j, i, types, slope)
        outs[et[-1]].append(out)
    out_dict, beta_dict = {}, {}
    for t, xs in outs.items():
        out_dict[t], beta_dict[t] = group(xs, state['q'], state['k_lin.weight'],
                                          state['k_lin.bias'])
    return out_dict, beta_dict


def to64(tree):
    if isinstance(tree, dict):
        return {k: to64(v) for k, v in tree.items()}
    return tree.double() if tree.dtype.is_floating_point else tree


def load_golden():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_han_v1.pt')
    return torch.load(path, weights_only=True)


def check_class_case(G, name, device, check, fuse=None, index_dtype=torch.int64):
    """The package's ``HANConv`` on one recorded case: outputs, ``beta`` and every gradient through
    ``check(got, want, what=...)``; parameters the call does not use take no gradient."""
    from pytorch_geometric_amd.nn import HANConv
    case = G['cases'][name]
    conv = HANConv(**case['kwargs']).eval()
    conv.load_state_dict(case['state'], strict=True)
    conv = conv.to(device)
    if fuse is not None:
        conv.fuse = fuse
    xs = {t: v.to(device).requires_grad_(True) for t, v in case['x_dict'].items()}
    eis = {et: ei.to(device=device, dtype=index_dtype)
           for et, ei in case['edge_index_dict'].items()}
    out, beta = conv(xs, eis, return_semantic_attention_weights=True)
    assert list(out) == list(case['x_dict']) and list(beta) == list(out)
    assert [t for t in out if out[t] is None] == case['none']
    for t in case['none']:
        assert beta[t] is None
    for t, want in case['out'].items():
        check(out[t], want, what=f'{name} out[{t}]')
        if t in case['beta']:
            check(beta[t], case['beta'][t], what=f'{name} beta[{t}]')
        else:
            assert beta[t] is None and want.size(0) == 0
    diff = [t for t in case['out'] if out[t].requires_grad]
    params = list(conv.named_parameters())
    grads = torch.autograd.grad([out[t] for t in diff],
                                list(xs.values()) + [p for _, p in params],
                                [case['grad_out'][t].to(device) for t in diff], allow_unused=True)
    for t, g in zip(xs, grads):
        if t in case['grad_x']:
            check(g, case['grad_x'][t], what=f'{name} grad_x[{t}]')
        else:
            assert g is None or not bool(g.any()), f'{name} grad_x[{t}]'
    for (n, _), g in zip(params, grads[len(xs):]):
        if n in case['grad_params']:
            check(g, case['grad_params'][n], what=f'{name} grad {n}')
        else:
            assert g is None or not bool(g.any()), f'{name} grad {n}'
    return conv
