"""HGTConv in plain torch, written from the formula, in whatever dtype the inputs have.  For edge
type e = (s, r, d) of the call with metadata position idx(e), head h and D = out_channels / H:

    [k | q | v]_t  = x_t @ W_kqv[t]^T + b_kqv[t]                          per node type t
    K_e[j, h]      = k_s[j, h] @ W_k[h * T + idx(e)],   V_e likewise      (the relation transform)
    s[i <- j, h]   = <q_d[i, h], K_e[j, h]> * p_rel[e][h] / sqrt(D)
    alpha          = softmax over ALL incoming edges of (d, i), across edge types
                     (maximum subtracted, 1e-16 on the denominator)
    o_d[i, h]      = sum alpha * V_e[j, h]
    out_d          = gelu(o_d) @ W_out[d]^T + b_out[d],  mixed as sigmoid(skip_d) * out_d +
                     (1 - sigmoid(skip_d)) * x_d where the widths agree

for the node types of ``x_dict`` that are a destination in the metadata.  tests/test_hgt_host.py
pins it to the reference's recorded results (tests/golden/golden_hgt_v1.pt); the GPU tests use it
in float64 at other shapes."""
import math
import os

import torch


def relation(ks, vs, widx, wk, wv, heads):
    """The packed ``kv [S, 2 * F]``: ``ks[e]`` / ``vs[e]`` ``[n_e, F]`` through the matrices
    ``h * T + widx[e]`` of ``wk`` / ``wv [H * T, D, D]``, stacked in the order given."""
    H, D = heads, wk.size(-1)
    T = wk.size(0) // H
    rows = []
    for k, v, i in zip(ks, vs, widx):
        mk, mv = wk.view(H, T, D, D)[:, i], wv.view(H, T, D, D)[:, i]
        rows.append(torch.cat([torch.einsum('nhd,hde->nhe', k.reshape(-1, H, D), mk).flatten(1),
                               torch.einsum('nhd,hde->nhe', v.reshape(-1, H, D), mv).flatten(1)],
                              dim=1))
    return torch.cat(rows, dim=0)


def conv(x_dict, edge_index_dict, p, out_channels, metadata, heads, **_):
    """One HGTConv layer from a state dict ``p`` with the reference's names."""
    W, H = out_channels, heads
    D = W // H
    node_types, edge_types = metadata
    edge_types = [tuple(et) for et in edge_types]
    T = len(edge_types)
    kqv = {t: x_dict[t] @ p[f'kqv_lin.lins.{t}.weight'].t() + p[f'kqv_lin.lins.{t}.bias']
           for t in node_types if t in x_dict}
    wk, wv = p['k_rel.weight'].view(H, T, D, D), p['v_rel.weight'].view(H, T, D, D)
    out = {}
    for d in kqv:
        if d not in {et[-1] for et in edge_types}:
            continue
        q = kqv[d][:, W:2 * W].reshape(-1, H, D)
        n = q.size(0)
        scores, values, index = [], [], []
        for e, et in enumerate(edge_types):
            if et[-1] != d or et not in edge_index_dict:
                continue
            src, dst = edge_index_dict[et][0].long(), edge_index_dict[et][1].long()
            k = torch.einsum('nhd,hde->nhe', kqv[et[0]][:, :W].reshape(-1, H, D), wk[:, e])
            v = torch.einsum('nhd,hde->nhe', kqv[et[0]][:, 2 * W:].reshape(-1, H, D), wv[:, e])
            prior = p['p_rel.' + '__'.join(et)].view(1, H)
            scores.append((q[dst] * k[src]).sum(-1) * prior / math.sqrt(D))
            values.append(v[src])
            index.append(dst)
        o = q.new_zeros(n, H, D)
        if scores:
            s, v, i = torch.cat(scores), torch.cat(values), torch.cat(index)
            top = s.new_full((n, H), float('-inf')).scatter_reduce(
                0, i.view(-1, 1).expand_as(s), s.detach(), 'amax', include_self=True)
            num = (s - top[i]).exp()
            den = s.new_zeros(n, H).index_add(0, i, num) + 1e-16
            o = o.index_add(0, i, (num / den[i]).unsqueeze(-1) * v)
        y = torch.nn.functional.gelu(o.reshape(n, W)) @ p[f'out_lin.lins.{d}.weight'].t() \
            + p[f'out_lin.lins.{d}.bias']
        if y.size(-1) == x_dict[d].size(-1):
            a = p[f'skip.{d}'].sigmoid()
            y = a * y + (1 - a) * x_dict[d]
        out[d] = y
    return out


# ---- the recorded cases, shared by the host and the GPU tests -------------------------------------
_GOLDEN = []


def load_golden():
    """tests/golden/golden_hgt_v1.pt, loaded once and never modified."""
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_hgt_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def check_gradients(name, params, grads, recorded, assert_close, **tol):
    """Every recorded parameter gradient is reproduced; a parameter the reference's call left
    without a gradient has none here either, or zeros (e.g. the relation matrices' prior of an
    edge type that is not in the call)."""
    for (n, _), g in zip(params, grads):
        if n in recorded:
            assert g is not None, f'{name}: no gradient for {n}'
            assert_close(g, recorded[n], what=f'{name} grad {n}', **tol)
        else:
            assert g is None or not bool(g.any()), f'{name}: unexpected gradient for {n}'


def check_class_case(G, name, device, fuse=True, index_dtype=torch.int64):
    """This package's HGTConv with the reference's state dict against one recorded case, at the
    tolerances of ``_transformer_ref.check_class_case``: outputs and input gradients at 1e-5,
    parameter gradients at 5e-5."""
    from pytorch_geometric_amd.nn import HGTConv
    from _util import assert_close
    case = G['cases'][name]
    layer = HGTConv(**case['kwargs'])
    assert list(layer.state_dict()) == list(case['state']), name
    layer.load_state_dict(case['state'], strict=True)
    layer = layer.to(device).eval()
    layer.fuse = fuse
    xs = {t: v.to(device).requires_grad_(True) for t, v in case['x_dict'].items()}
    eis = {et: ei.to(device).to(index_dtype) for et, ei in case['edge_index_dict'].items()}
    out = layer(xs, eis)
    assert list(out) == list(case['out']), f'{name}: output keys {list(out)}'
    params = list(layer.named_parameters())
    grads = torch.autograd.grad([out[t] for t in out], list(xs.values()) + [p for _, p in params],
                                [case['grad_out'][t].to(device) for t in out], allow_unused=True)
    for t in out:
        assert_close(out[t], case['out'][t], what=f'{name} out[{t}]')
    for t, g in zip(xs, grads):
        assert_close(g, case['grad_x'][t], what=f'{name} grad_x[{t}]')
    check_gradients(name, params, grads[len(xs):], case['grad_params'], assert_close,
                    atol=5e-5, rtol=5e-5)
    return layer
