"""The two primitives ``MessagePassing`` needs to compute host tensors, in plain torch: the softmax
by index and the aggregation modules' formulas.  The layers with a ``propagate`` fallback reach
them through ``edge_updater`` / ``propagate``; the operators themselves (``utils.softmax``,
``utils.scatter``, an aggregation module called directly) keep raising on host tensors."""
from typing import Optional

import torch
from torch import Tensor

from ..utils import softmax as _device_softmax
from .aggr import (DegreeScalerAggregation, MaxAggregation, MeanAggregation, MinAggregation,
                   MultiAggregation, PowerMeanAggregation, SoftmaxAggregation, StdAggregation,
                   SumAggregation, VarAggregation)


def _per_row(index: Tensor, like: Tensor) -> Tensor:
    """``index [E]`` shaped to broadcast over the trailing dimensions of ``like [E, ...]``"""
    return index.view(-1, *[1] * (like.dim() - 1))


def softmax(src: Tensor, index: Tensor, ptr: Optional[Tensor] = None,
            num_nodes: Optional[int] = None) -> Tensor:
    """``utils.softmax`` over dimension 0 for the conv layers: device tensors go there unchanged;
    host tensors take the reference's formula (torch_geometric/utils/_softmax.py:82-88: detached
    maximum subtracted, ``1e-16`` on the denominator)."""
    if src.is_cuda:
        return _device_softmax(src, index, ptr, num_nodes)
    index = index.long()
    if num_nodes is None:
        num_nodes = int(index.max()) + 1 if index.numel() > 0 else 0
    shape = (num_nodes, ) + src.shape[1:]
    top = src.new_full(shape, float('-inf')).scatter_reduce(
        0, _per_row(index, src).expand_as(src), src.detach(), 'amax', include_self=True)
    num = (src - top.index_select(0, index)).exp()
    den = src.new_zeros(shape).index_add_(0, index, num) + 1e-16
    return num / den.index_select(0, index)


def aggregate(module: torch.nn.Module, msg: Tensor, index: Tensor, n: int) -> Tensor:
    """``module`` over per-edge rows ``msg [E, ...]`` with destinations ``index`` out of ``n``"""
    index = index.long()
    kind = type(module)
    if kind is DegreeScalerAggregation:
        out = aggregate(module.aggr, msg, index, n)
        return module.scale(out, torch.bincount(index, minlength=n))
    if kind is MultiAggregation:
        return module.combine([aggregate(a, msg, index, n) for a in module.aggrs])
    if kind is StdAggregation:
        std = aggregate(module.var_aggr, msg, index, n).clamp(min=1e-5).sqrt()
        return std.masked_fill(std <= 1e-5 ** 0.5, 0.0)
    shape = (n, ) + msg.shape[1:]
    where = _per_row(index, msg).expand_as(msg)

    def reduce(src, how):
        return src.new_zeros(shape).scatter_reduce(0, where, src, how, include_self=False)

    def count():
        return _per_row(torch.bincount(index, minlength=n).clamp(min=1).to(msg.dtype), msg)

    if kind in (SumAggregation, MeanAggregation):
        out = msg.new_zeros(shape).index_add_(0, index, msg)
        return out if kind is SumAggregation else out / count()
    if kind in (MaxAggregation, MinAggregation):
        return reduce(msg, 'amax' if kind is MaxAggregation else 'amin')
    if kind is VarAggregation:
        mean = reduce(msg, 'sum') / count()
        sq = msg.detach() if module.semi_grad else msg
        return reduce(sq * sq, 'sum') / count() - mean * mean
    if kind is SoftmaxAggregation:
        t = module.t.view(1, -1) if isinstance(module.t, Tensor) else module.t
        with torch.set_grad_enabled(torch.is_grad_enabled() and not module.semi_grad):
            logits = msg * t
            top = reduce(logits.detach(), 'amax')
            e = (logits - top.index_select(0, index)).exp()
            alpha = e / (reduce(e, 'sum').index_select(0, index) + 1e-16)
        return reduce(msg * alpha, 'sum')
    if kind is PowerMeanAggregation:
        p = module.p.view(1, -1) if isinstance(module.p, Tensor) else module.p
        if not isinstance(p, Tensor) and p == 1:
            return reduce(msg, 'sum') / count()
        lo, hi = module.min_value, module.max_value
        out = reduce(msg.clamp(min=lo, max=hi).pow(p), 'sum') / count()
        return out.clamp(min=lo, max=hi).pow(1. / p)
    raise NotImplementedError(f"the host route has no aggregation '{kind.__name__}'")
