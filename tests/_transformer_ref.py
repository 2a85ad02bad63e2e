"""TransformerConv in plain torch — a restatement of

    s[i<-j, h] = <q[i,h,:], key[j,h,:] (+ e[k,h,:])> / sqrt(C)
    alpha      = softmax_j(s)           (maximum subtracted, 1e-16 on the denominator)
    out[i,h,:] = sum_j alpha[i<-j,h] * (value[j,h,:] (+ e[k,h,:]))

and of the layer around it (projections, head concat / mean, skip connection, beta gate), in
whatever dtype the inputs have.  tests/test_transformer_host.py pins it to the reference's recorded
results (tests/golden/golden_transformer_v1.pt); the GPU tests use it in float64 at other shapes."""
import math

import torch


def attend(q, k, v, edge_index, n_dst, e=None):
    """(out [n_dst, H, C], alpha [E, H] in edge order) for q [>= n_dst, H, C] and k, v
    [N_src, H, C]; e [E, H, C] = the projected edge features, added to key and value."""
    H, C = q.shape[1:]
    src, dst = edge_index[0].long(), edge_index[1].long()
    k_j, v_j = k[src], v[src]
    if e is not None:
        k_j, v_j = k_j + e, v_j + e
    s = (q[dst] * k_j).sum(-1) / math.sqrt(C)
    top = s.new_full((n_dst, H), float('-inf')).scatter_reduce(
        0, dst.view(-1, 1).expand_as(s), s.detach(), 'amax', include_self=True)
    num = (s - top[dst]).exp()
    den = s.new_zeros(n_dst, H).index_add(0, dst, num) + 1e-16
    alpha = num / den[dst]
    out = v.new_zeros(n_dst, H, C).index_add(0, dst, alpha.unsqueeze(-1) * v_j)
    return out, alpha


def conv(x, edge_index, p, heads, out_channels, concat=True, root_weight=True, edge_attr=None,
         **_):
    """One TransformerConv layer from a state dict ``p`` (keys ``lin_key.weight`` ... as the
    reference names them; ``lin_beta.weight`` present = gated skip).  ``x`` is a tensor or a
    (source, destination) pair.  Returns (out, alpha in edge order)."""
    def lin(name, v):
        out = v @ p[f'{name}.weight'].t()
        b = p.get(f'{name}.bias')
        return out if b is None else out + b

    H, C = heads, out_channels
    x_src, x_dst = x if isinstance(x, (tuple, list)) else (x, x)
    q = lin('lin_query', x_dst).view(-1, H, C)
    k = lin('lin_key', x_src).view(-1, H, C)
    v = lin('lin_value', x_src).view(-1, H, C)
    e = None if edge_attr is None else lin('lin_edge', edge_attr).view(-1, H, C)
    out, alpha = attend(q, k, v, edge_index, q.size(0), e)
    out = out.reshape(-1, H * C) if concat else out.mean(1)
    if root_weight:
        x_r = lin('lin_skip', x_dst)
        if 'lin_beta.weight' in p:
            gate = (torch.cat([out, x_r, out - x_r], dim=-1) @ p['lin_beta.weight'].t()).sigmoid()
            out = gate * x_r + (1 - gate) * out
        else:
            out = out + x_r
    return out, alpha


# ---- the recorded cases, shared by the host and the GPU tests -------------------------------------
_GOLDEN = []


def load_golden():
    """tests/golden/golden_transformer_v1.pt, loaded once and never modified."""
    import os
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_transformer_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def case_inputs(G, case):
    xs = [G['x']] + ([G['x_dst']] if case['pair'] else [])
    ei = G['edge_index_pair'] if case['pair'] else G['edge_index']
    ea = G['edge_attr'] if case['edge_attr'] else None
    return xs, ei, ea


def check_class_case(G, name, device, fuse=True, index_dtype=torch.int64):
    """This package's TransformerConv with the reference's state dict against one recorded case:
    ``out`` / ``grad_x`` at 1e-5, parameter gradients at 5e-5 (the tolerances of
    test_gpu_layers._run_layer), attention weights at 1e-5."""
    from pytorch_geometric_amd.nn import TransformerConv
    from _util import assert_close
    case = G['cases'][name]
    kw = dict(case['kwargs'])
    layer = TransformerConv(kw.pop('in_channels'), **kw)
    assert list(layer.state_dict()) == list(case['state']), name
    layer.load_state_dict(case['state'])
    layer = layer.to(device).eval()
    layer.fuse = fuse
    xs, ei, ea = case_inputs(G, case)
    xs = [t.to(device).requires_grad_(True) for t in xs]
    res = layer(tuple(xs) if case['pair'] else xs[0], ei.to(device).to(index_dtype),
                edge_attr=None if ea is None else ea.to(device),
                return_attention_weights=True if 'attention' in case else None)
    out, att = res if 'attention' in case else (res, None)
    params = list(layer.named_parameters())
    # (without root_weight lin_skip exists but is unused: no gradient here, none recorded)
    grads = torch.autograd.grad(out, xs + [p for _, p in params], case['grad_out'].to(device),
                                allow_unused=True)
    params = [(n, p) for (n, p), g in zip(params, grads[len(xs):]) if g is not None]
    grads = [g for g in grads if g is not None]
    assert_close(out, case['out'], what=f'{name} out')
    for g, ref in zip(grads, case['grad_x']):
        assert_close(g, ref, what=f'{name} grad_x')
    assert [n for n, _ in params] == list(case['grad_params']), name
    for (n, _), g in zip(params, grads[len(xs):]):
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'{name} grad {n}')
    if att is not None:
        assert torch.equal(att[0].cpu().long(), case['attention'][0]), f'{name}: edge list'
        assert_close(att[1], case['attention'][1], what=f'{name} attention')
    return layer
