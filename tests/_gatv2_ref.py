"""GATv2 in plain torch — a restatement of

    s[i<-j, h] = sum_c att[h,c] * leaky_relu(x_l[j,h,c] + x_r[i,h,c] (+ e[k,h,c]))
    alpha      = softmax_j(s)           (maximum subtracted, 1e-16 on the denominator)
    out[i,h,:] = sum_j alpha[i<-j,h] * x_l[j,h,:]

and of the layer / model around it (projections, self-loops, head concat / mean, residual, bias),
in whatever dtype the inputs have.  tests/test_gatv2_host.py pins it to the reference's recorded
results (tests/golden/golden_gatv2_v1.pt); the GPU tests use it in float64 at other shapes."""
import torch
import torch.nn.functional as F


def attend(x_l, x_r, att, edge_index, n_dst, slope=0.2, e=None):
    """(out [n_dst, H, C], alpha [E, H] in edge order) for x_l [N_src, H, C], x_r [>= n_dst, H, C],
    att [H, C] (any shape with H * C entries)."""
    H, C = x_l.shape[1:]
    src, dst = edge_index[0].long(), edge_index[1].long()
    pre = x_l[src] + x_r[dst]
    if e is not None:
        pre = pre + e
    s = (att.reshape(1, H, C) * F.leaky_relu(pre, slope)).sum(-1)
    top = s.new_full((n_dst, H), float('-inf')).scatter_reduce(
        0, dst.view(-1, 1).expand_as(s), s.detach(), 'amax', include_self=True)
    num = (s - top[dst]).exp()
    den = s.new_zeros(n_dst, H).index_add(0, dst, num) + 1e-16
    alpha = num / den[dst]
    out = x_l.new_zeros(n_dst, H, C).index_add(0, dst, alpha.unsqueeze(-1) * x_l[src])
    return out, alpha


def with_self_loops(edge_index, edge_attr, n):
    """remove_self_loops + add_self_loops(fill_value='mean'): the loop of node i carries the mean of
    the attributes of its remaining incoming edges."""
    keep = edge_index[0] != edge_index[1]
    ei = edge_index[:, keep]
    loops = torch.arange(n, dtype=ei.dtype, device=ei.device)
    if edge_attr is not None:
        ea = edge_attr[keep]
        total = ea.new_zeros(n, ea.size(1)).index_add(0, ei[1].long(), ea)
        count = ea.new_zeros(n).index_add(0, ei[1].long(), ea.new_ones(ea.size(0)))
        edge_attr = torch.cat([ea, total / count.clamp(min=1).view(-1, 1)])
    return torch.cat([ei, torch.stack([loops, loops])], dim=1), edge_attr


def conv(x, edge_index, p, heads, out_channels, concat=True, negative_slope=0.2,
         add_self_loops=True, edge_attr=None, prefix='', **_):
    """One GATv2Conv layer from a state dict ``p`` (keys ``lin_l.weight`` ... as the reference
    names them; ``lin_r`` absent = shared weights).  ``x`` is a tensor or a (source, destination)
    pair.  Returns (out, edge_index used, alpha in that edge order)."""
    def lin(name, v):
        out = v @ p[f'{prefix}{name}.weight'].t()
        b = p.get(f'{prefix}{name}.bias')
        return out if b is None else out + b

    H, C = heads, out_channels
    x_src, x_dst = x if isinstance(x, (tuple, list)) else (x, x)
    x_l = lin('lin_l', x_src).view(-1, H, C)
    x_r = lin('lin_r' if f'{prefix}lin_r.weight' in p else 'lin_l', x_dst).view(-1, H, C)
    if add_self_loops:
        edge_index, edge_attr = with_self_loops(edge_index, edge_attr,
                                                min(x_l.size(0), x_r.size(0)))
    e = None if edge_attr is None else lin('lin_edge', edge_attr).view(-1, H, C)
    out, alpha = attend(x_l, x_r, p[f'{prefix}att'], edge_index, x_r.size(0), negative_slope, e)
    out = out.reshape(-1, H * C) if concat else out.mean(1)
    if f'{prefix}res.weight' in p:
        out = out + lin('res', x_dst)
    if f'{prefix}bias' in p:
        out = out + p[f'{prefix}bias']
    return out, edge_index, alpha


def gat_model(x, edge_index, p, hidden_channels, num_layers, out_channels, heads, **_):
    """GAT(v2=True): hidden layers concatenate heads of width hidden // heads and are followed by
    ReLU; the output layer averages its heads."""
    for i in range(num_layers):
        last = i == num_layers - 1
        width = out_channels if last else hidden_channels // heads
        x, _, _ = conv(x, edge_index, p, heads, width, concat=not last, prefix=f'convs.{i}.')
        if not last:
            x = x.relu()
    return x


# ---- the recorded cases, shared by the host and the GPU tests -------------------------------------
_GOLDEN = []


def load_golden():
    """tests/golden/golden_gatv2_v1.pt, loaded once and never modified."""
    import os
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_gatv2_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def case_inputs(G, case):
    xs = [G['x']] + ([G['x_dst']] if case['pair'] else [])
    ei = G['edge_index_pair'] if case['pair'] else G['edge_index']
    ea = G['edge_attr'] if case['edge_attr'] else None
    return xs, ei, ea


def check_class_case(G, name, device, fuse=True, index_dtype=torch.int64):
    """This package's GATv2Conv with the reference's state dict against one recorded case:
    ``out`` / ``grad_x`` at 1e-5, parameter gradients at 5e-5 (the tolerances of
    test_gpu_layers._run_layer), attention weights at 1e-5."""
    from pytorch_geometric_amd.nn import GATv2Conv
    from _util import assert_close
    case = G['cases'][name]
    kw = dict(case['kwargs'])
    layer = GATv2Conv(kw.pop('in_channels'), **kw)
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
    grads = torch.autograd.grad(out, xs + [p for _, p in params], case['grad_out'].to(device))
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


def check_model_case(G, device, fuse=True):
    """GAT(v2=True) against the recorded model: 2e-5 for ``out`` / ``grad_x``, 1e-4 for parameter
    gradients (test_gpu_layers._run_model)."""
    from pytorch_geometric_amd.nn import GAT, GATv2Conv
    from _util import assert_close
    case = G['model']
    model = GAT(**case['kwargs'])
    assert all(type(c) is GATv2Conv for c in model.convs)
    assert list(model.state_dict()) == list(case['state'])
    model.load_state_dict(case['state'])
    model = model.to(device).eval()
    for c in model.convs:
        c.fuse = fuse
    x = G['x'].to(device).requires_grad_(True)
    out = model(x, G['edge_index'].to(device))
    params = list(model.named_parameters())
    grads = torch.autograd.grad(out, [x] + [p for _, p in params], case['grad_out'].to(device))
    assert_close(out, case['out'], atol=2e-5, what='model out')
    assert_close(grads[0], case['grad_x'][0], atol=2e-5, what='model grad_x')
    for (n, _), g in zip(params, grads[1:]):
        assert_close(g, case['grad_params'][n], atol=1e-4, rtol=1e-4, what=f'model grad {n}')
    return model
