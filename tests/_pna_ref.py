"""PNAConv / DegreeScalerAggregation: what the host and the GPU tests share.  The recorded reference
cases of tests/golden/golden_pna_v1.pt (tests/golden/make_golden_pna.py) and a restatement, in the
dtype of its inputs (float64 in the tests), of the NODE the kernels of csrc/pna.hip implement,

    m_k = p_dst[dst_k] + p_src[src_k] + Wc edge_attr[k]
    mean / min / max / std over the slots of every destination, exactly 0 for an empty one
    std = sqrt(max(var, 1e-5)), 0 where that is <= sqrt(1e-5)

of the degree scalers and of the whole layer from a state dict.
"""
import math
import os

import torch

CASES = ['identity', 'amplification', 'attenuation', 'towers4', 'towers4_divide', 'edge3', 'edge9',
         'train_norm', 'linear_scalers', 'single', 'deep', 'sum_var']
GENERIC_CASES = ['deep', 'sum_var']          # pre_layers = 2; sum and var aggregators

_GOLDEN = []


def load_golden():
    """tests/golden/golden_pna_v1.pt, loaded once and never modified."""
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_pna_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def aggregate(msg, dst, n_dst, aggrs):
    """``[n_dst, W]`` per aggregator out of sum / mean / min / max / var / std over per-edge rows
    ``msg [E, W]``; ``var = mean(x^2) - mean(x)^2`` as the reference forms it"""
    dst = dst.long()
    W = msg.size(1)
    cnt = torch.bincount(dst, minlength=n_dst).clamp(min=1).to(msg.dtype).view(-1, 1)
    index = dst.view(-1, 1).expand(-1, W)

    def reduce(src, how):
        if how == 'sum':
            return msg.new_zeros(n_dst, W).scatter_reduce(0, index, src, how, include_self=False)
        # min / max start from NaN, not 0: scatter_reduce's backward counts the initial value among
        # the ties when it EQUALS the result (an extremum of exactly 0, common on a dyadic grid)
        # and drops that share of the gradient.  Empty rows are set to 0 afterwards.
        has = torch.bincount(dst, minlength=n_dst).view(-1, 1) > 0
        out = msg.new_full((n_dst, W), float('nan')).scatter_reduce(0, index, src, how,
                                                                    include_self=False)
        return torch.where(has, out, torch.zeros_like(out))

    outs = []
    for a in aggrs:
        if a == 'sum':
            outs.append(reduce(msg, 'sum'))
        elif a == 'mean':
            outs.append(reduce(msg, 'sum') / cnt)
        elif a in ('min', 'max'):
            outs.append(reduce(msg, 'a' + a))
        else:
            mean = reduce(msg, 'sum') / cnt
            var = reduce(msg * msg, 'sum') / cnt - mean * mean
            if a == 'std':
                std = var.clamp(min=1e-5).sqrt()
                var = std.masked_fill(std <= math.sqrt(1e-5), 0.0)
            outs.append(var)
    return outs


def pna_aggregate(p_src, p_dst, edge_attr, Wc, edge_index, n_dst, stats):
    """the node: a tuple of ``[n_dst, W]`` in the order of ``stats``"""
    src, dst = edge_index[0].long(), edge_index[1].long()
    msg = p_dst[dst] + p_src[src]
    if Wc is not None:
        msg = msg + edge_attr @ Wc.t()
    return tuple(aggregate(msg, dst, n_dst, stats))


def scale(out, deg, scalers, avg_lin, avg_log):
    """``out [N, ..., F]`` under the scalers, concatenated on the last dimension; ``deg``
    broadcasts against ``out``"""
    outs = []
    for s in scalers:
        if s == 'identity':
            outs.append(out)
        elif s == 'amplification':
            outs.append(out * (torch.log(deg + 1) / avg_log))
        elif s == 'attenuation':
            outs.append(out * (avg_log / torch.log(deg.clamp(min=1) + 1)))
        elif s == 'linear':
            outs.append(out * (deg / avg_lin))
        else:
            assert s == 'inverse_linear'
            outs.append(out * (avg_lin / deg.clamp(min=1)))
    return torch.cat(outs, dim=-1)


def scaler_problem():
    """300 rows of width 7 over 40 groups, some of them empty; every aggregator and scaler"""
    from _util import gen, random_graph
    ei = random_graph(60, 40, 300, 5)
    index = ei[1][ei[1] % 6 != 0]                                # degree-0 rows
    x = torch.randn(index.numel(), 7, generator=gen(6))
    hist = torch.bincount(torch.bincount(index, minlength=40))
    aggrs = ['mean', 'min', 'max', 'std', 'sum', 'var']
    scalers = ['identity', 'amplification', 'attenuation', 'linear', 'inverse_linear']
    return x, index, hist, aggrs, scalers


def _mlp(h, state, prefix):
    k = 0
    while f'{prefix}.{k}.weight' in state:
        if k:
            h = h.relu()
        h = h @ state[f'{prefix}.{k}.weight'].t() + state[f'{prefix}.{k}.bias']
        k += 2
    return h


def pna_layer(x, edge_attr, edge_index, state, kw, n_dst=None):
    """PNAConv (act = relu) from a state dict and its constructor arguments ``kw``, in the dtype of
    the inputs; ``edge_index[1]`` are the destinations"""
    T = kw.get('towers', 1)
    Fi = x.size(1) // T if kw.get('divide_input') else x.size(1)
    n_dst = x.size(0) if n_dst is None else n_dst
    xt = x.view(-1, T, Fi) if kw.get('divide_input') else x.view(-1, 1, Fi).repeat(1, T, 1)
    src, dst = edge_index[0].long(), edge_index[1].long()
    parts = [xt[dst], xt[src]]
    if kw.get('edge_dim'):
        e = edge_attr @ state['edge_encoder.weight'].t() + state['edge_encoder.bias']
        parts.append(e.view(-1, 1, Fi).repeat(1, T, 1))
    h = torch.cat(parts, dim=-1)
    msg = torch.stack([_mlp(h[:, t], state, f'pre_nns.{t}') for t in range(T)], dim=1)
    outs = aggregate(msg.reshape(-1, T * Fi), dst, n_dst, kw['aggregators'])
    out = torch.cat([o.view(n_dst, T, Fi) for o in outs], dim=-1)
    deg = torch.bincount(dst, minlength=n_dst).to(x.dtype).view(-1, 1, 1)
    out = scale(out, deg, kw['scalers'], state['aggr_module.avg_deg_lin'],
                state['aggr_module.avg_deg_log'])
    out = torch.cat([xt[:n_dst], out], dim=-1)
    out = torch.cat([_mlp(out[:, t], state, f'post_nns.{t}') for t in range(T)], dim=1)
    return out @ state['lin.weight'].t() + state['lin.bias']


def make_layer(G, name):
    """this package's class with the recorded state dict of case ``name`` (strict load)"""
    from pytorch_geometric_amd.nn import PNAConv
    case = G['cases'][name]
    layer = PNAConv(G['x'].size(1), case['out'].size(1), deg=G['deg'], **case['kwargs'])
    assert list(layer.state_dict()) == list(case['state']), name
    layer.load_state_dict(case['state'], strict=True)
    return layer


def check_class_case(G, name, device, index_dtype=torch.int64, tol=2e-5):
    """This package's class against one recorded case: ``out`` and every gradient by
    ``assert_close_scaled`` at ``tol``."""
    from _util import assert_close_scaled
    case = G['cases'][name]
    layer = make_layer(G, name).to(device)
    x = G['x'].to(device).requires_grad_(True)
    ei = G['edge_index'].to(device).to(index_dtype)
    leaves = [x]
    ea = None
    if 'edge_attr' in case:
        ea = case['edge_attr'].to(device).requires_grad_(True)
        leaves.append(ea)
    out = layer(x, ei, ea)
    params = list(layer.named_parameters())
    assert [n for n, _ in params] == list(case['grad_params']), name
    grads = torch.autograd.grad(out, leaves + [p for _, p in params], case['grad_out'].to(device))
    assert_close_scaled(out, case['out'], tol=tol, what=f'{name} out')
    assert_close_scaled(grads[0], case['grad_x'], tol=tol, what=f'{name} grad_x')
    if ea is not None:
        assert_close_scaled(grads[1], case['grad_edge_attr'], tol=tol,
                            what=f'{name} grad_edge_attr')
    for (n, _), g in zip(params, grads[len(leaves):]):
        assert_close_scaled(g, case['grad_params'][n], tol=tol, what=f'{name} grad {n}')
    return layer
