"""A plain-torch restatement of ``HeteroConv`` over bipartite ``SAGEConv``
(nn/conv/hetero_conv.py:13-172 calling nn/conv/sage_conv.py:118-152 once per edge type):
``index_add_`` aggregation, the ``clamp(min=1)`` degree of the mean, ``lin_l`` (with its bias) on the
aggregate plus ``lin_r`` on the destination features, and the six group modes.  It runs in float32
or float64 on the CPU — whatever dtype the features and parameters come in — and knows nothing of
this package.  ``tests/test_hetero_conv_host.py`` pins it to the reference's recorded results; the
GPU tests then compare the kernels against it."""
import torch


def param_key(edge_type, name):
    """The state-dict key of ``name`` (``lin_l.weight`` ...) of the conv of ``edge_type``."""
    return f"convs.<{'___'.join(edge_type)}>.{name}"


def aggregate(x_src, edge_index, num_dst, aggr):
    """``aggr`` in mean / sum of the source rows per destination; empty rows give zeros."""
    src, dst = edge_index[0].long(), edge_index[1].long()
    out = x_src.new_zeros(num_dst, x_src.size(1))
    out.index_add_(0, dst, x_src[src])
    if aggr == 'mean':
        deg = x_src.new_zeros(num_dst).index_add_(0, dst, x_src.new_ones(dst.numel()))
        out = out / deg.clamp(min=1).unsqueeze(-1)
    return out


def sage_conv(x_src, x_dst, edge_index, aggr, w_l, b_l, w_r):
    out = aggregate(x_src, edge_index, x_dst.size(0), 'sum' if aggr == 'add' else aggr) @ w_l.t()
    if b_l is not None:
        out = out + b_l
    if w_r is not None:
        out = out + x_dst @ w_r.t()
    return out


def group(xs, aggr):
    if aggr is None:
        return torch.stack(xs, dim=1)
    if len(xs) == 1:
        return xs[0]
    if aggr == 'cat':
        return torch.cat(xs, dim=-1)
    stacked = torch.stack(xs, dim=0)
    if aggr == 'sum':
        return stacked.sum(0)
    if aggr == 'mean':
        return stacked.mean(0)
    if aggr == 'min':
        return stacked.min(0)[0]
    if aggr == 'max':
        return stacked.max(0)[0]
    raise ValueError(aggr)


def hetero_conv(edge_types, x_dict, edge_index_dict, params, conv_aggr, group_aggr):
    """``edge_types``: the layer's edge types in order; ``params``: ``{state-dict key: tensor}``
    (a missing ``lin_l.bias`` / ``lin_r.weight`` is a conv built without it); ``conv_aggr``: one
    name or ``{edge_type: name}``.  Edge types absent from ``edge_index_dict`` are skipped; the
    result is keyed by destination type in order of first appearance."""
    outs = {}
    for et in edge_types:
        if et not in edge_index_dict:
            continue
        aggr = conv_aggr[et] if isinstance(conv_aggr, dict) else conv_aggr
        out = sage_conv(x_dict[et[0]], x_dict[et[-1]], edge_index_dict[et], aggr,
                        params[param_key(et, 'lin_l.weight')],
                        params.get(param_key(et, 'lin_l.bias')),
                        params.get(param_key(et, 'lin_r.weight')))
        outs.setdefault(et[-1], []).append(out)
    return {d: group(xs, group_aggr) for d, xs in outs.items()}
