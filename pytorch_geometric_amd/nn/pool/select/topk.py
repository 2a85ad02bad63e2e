"""``topk`` and :class:`SelectTopK` (torch_geometric/nn/pool/select/topk.py).

Routes of the ``ratio`` selection:

* fused (csrc/pool.hip, ``pygamd_topk_select``) — float32 (or half / bfloat16, widened: the order
  of the scores does not change) device scores with a NON-DECREASING int32 / int64 device ``batch``
  vector, or none, and no graph longer than ``_native.TOPK_MAX_NODES``: ONE launch over the cached
  by-graph handle of the batch tensor (:mod:`pytorch_geometric_amd._norm`: the norm layers of the
  same step share it).  ``k`` is the reference's own expression in the scores' dtype; the number of
  kept nodes and the largest graph are taken in one host read;
* generic — everything else (host tensors, other dtypes, an unsorted ``batch``, a longer graph,
  ``fuse=False``): the reference's expression with ``torch.sort(..., descending=True,
  stable=True)``.

Both order a graph's nodes by score descending, then node index ascending; any NaN ranks above
every number and ``-0.0 == +0.0``.  ``min_score`` selects with ``nonzero`` on either route."""
from typing import Callable, Optional, Union

import torch
from torch import Tensor

from .... import _native, _norm
from ...inits import uniform
from .._fuse import LOW as _LOW
from .._fuse import fuse_default
from .base import Select, SelectOutput


def _native_f32(*tensors) -> bool:
    return all(t.is_cuda for t in tensors) and tensors[0].dtype == torch.float32


def _group_max(x: Tensor, batch: Tensor) -> Tensor:
    """``scatter(x, batch, reduce='max')``: empty groups give 0"""
    if _native_f32(x, batch):
        from ....utils import scatter
        return scatter(x.detach(), batch, reduce='max')
    size = int(batch.max()) + 1 if batch.numel() > 0 else 0
    return x.new_zeros(size).scatter_reduce(0, batch.long(), x.detach(), 'amax',
                                            include_self=False)


def group_softmax(x: Tensor, batch: Tensor) -> Tensor:
    """``softmax(x, batch)`` of the reference (utils/_softmax.py:82-88)"""
    if _native_f32(x, batch):
        from ....utils import softmax
        return softmax(x, batch)
    index = batch.long()
    out = (x - _group_max(x, batch).index_select(0, index)).exp()
    size = int(batch.max()) + 1 if batch.numel() > 0 else 0
    total = out.new_zeros(size).index_add_(0, index, out) + 1e-16
    return out / total.index_select(0, index)


def num_selected(ratio: Union[float, int], num_nodes: Tensor, dtype: torch.dtype) -> Tensor:
    """``k`` per graph: the reference's expression (topk.py:31-34), in the scores' dtype"""
    if ratio >= 1:
        return num_nodes.new_full((num_nodes.size(0), ), int(ratio)).to(torch.long)
    return (float(ratio) * num_nodes.to(dtype)).ceil().to(torch.long)


def _topk_generic(x: Tensor, ratio: Union[float, int], batch: Tensor) -> Tensor:
    size = int(batch.max()) + 1 if batch.numel() > 0 else 0
    num_nodes = torch.bincount(batch.long(), minlength=size).to(batch.dtype)
    k = num_selected(ratio, num_nodes, x.dtype)
    # (one NaN for all: a device sort ranks a NaN with the sign bit set below every number)
    x = torch.where(x != x, torch.full_like(x, float('nan')), x).view(-1)
    x, x_perm = torch.sort(x, descending=True, stable=True)
    batch = batch[x_perm]
    batch, batch_perm = torch.sort(batch, descending=False, stable=True)
    arange = torch.arange(x.size(0), dtype=torch.long, device=x.device)
    ptr = torch.zeros(size + 1, dtype=torch.long, device=x.device)
    ptr[1:] = num_nodes.cumsum(0)
    batch = batch.long()
    mask = (arange - ptr[batch]) < k[batch]
    return x_perm[batch_perm[mask]]


def select_fusable(x: Tensor, batch: Optional[Tensor]) -> bool:
    """the fused route's conditions that need no read"""
    if not (isinstance(x, Tensor) and x.is_cuda and x.dim() == 1
            and x.dtype in (torch.float32, ) + _LOW):
        return False
    if batch is None:
        return True
    return (batch.is_cuda and batch.dim() == 1 and batch.numel() == x.numel()
            and batch.dtype in (torch.int32, torch.int64))


def topk_fused(x: Tensor, ratio: Union[float, int], batch: Optional[Tensor]) -> Optional[Tensor]:
    """``perm`` by the select kernel, or None when the batch vector turns out not to be sorted or
    a graph is past the kernel's envelope."""
    if batch is None:
        handle = _norm.single_graph_handle(x.numel(), x.device)
    else:
        handle = _norm.batch_handle(batch, None)
        if not handle.is_sorted:
            return None
    ptr = handle.ptr
    if ptr.numel() < 2:
        return torch.empty(0, dtype=torch.long, device=x.device)
    num_nodes = ptr[1:] - ptr[:-1]
    k = num_selected(ratio, num_nodes, x.dtype)
    kept = torch.minimum(k, num_nodes.to(torch.long)).clamp_(min=0)
    out_ptr = torch.zeros(ptr.numel(), dtype=torch.long, device=x.device)
    torch.cumsum(kept, 0, out=out_ptr[1:])
    # ONE read: the number of kept nodes and the largest graph
    total, longest = torch.stack([out_ptr[-1], num_nodes.max().to(torch.long)]).tolist()
    if longest > _native.TOPK_MAX_NODES:
        return None
    # (no weight: the layers take score[perm] from the gather-scale kernel, with its gradient)
    return _native.topk_select(x.detach().float(), ptr, k, out_ptr, total, longest,
                               want_weight=False)[0]


def topk(x: Tensor, ratio: Optional[Union[float, int]], batch: Tensor,
         min_score: Optional[float] = None, tol: float = 1e-7, *,
         fuse: Optional[bool] = None) -> Tensor:
    r"""The indices of the nodes ``torch_geometric.nn.pool.select.topk.topk`` keeps
    (topk.py:13-48): with ``min_score`` the nodes whose score exceeds ``min(min_score, the graph's
    maximum - tol)``, in node order; otherwise of every graph its ``ceil(ratio * n)`` (``ratio <
    1``) or ``int(ratio)`` best nodes, graph by graph, ordered by score descending, then node index
    ascending.  ``fuse`` (keyword only; None: ``PYGAMD_FUSE_POOL`` or the measured default) allows
    the one-launch select kernel where it applies."""
    if min_score is not None:
        scores_max = _group_max(x, batch).index_select(0, batch.long()) - tol
        scores_min = scores_max.clamp(max=min_score)
        return (x > scores_min).nonzero().view(-1)
    if ratio is None:
        raise ValueError("At least one of the 'ratio' and 'min_score' parameters must be "
                         "specified")
    if fuse is None:
        fuse = fuse_default('topk')
    if fuse and select_fusable(x, batch):
        out = topk_fused(x, ratio, batch)
        if out is not None:
            return out
    if batch is None:
        batch = torch.zeros(x.size(0), dtype=torch.long, device=x.device)
    return _topk_generic(x, ratio, batch)


class SelectTopK(Select):
    r"""Selects the top-:math:`k` nodes by a learnt projection score, with the constructor
    arguments, the parameter (``weight [1, in_channels]``), its initialisation and the ``__repr__``
    of ``torch_geometric.nn.pool.select.SelectTopK`` (topk.py:51-150): ``y = act(X p / |p|)``
    and the best ``k`` nodes per graph, or with ``min_score`` ``y = softmax(X p)`` per graph and
    the nodes above the threshold.  ``fuse`` routes the selection as :func:`topk` does."""

    def __init__(self, in_channels: int, ratio: Union[int, float] = 0.5,
                 min_score: Optional[float] = None, act: Union[str, Callable] = 'tanh'):
        super().__init__()
        if ratio is None and min_score is None:
            raise ValueError(f"At least one of the 'ratio' and 'min_score' parameters must be "
                             f"specified in '{self.__class__.__name__}'")
        from ...models.basic_gnn import activation_resolver
        self.in_channels = in_channels
        self.ratio = ratio
        self.min_score = min_score
        self.act = activation_resolver(act)
        self.weight = torch.nn.Parameter(torch.empty(1, in_channels))
        self.fuse = fuse_default('topk')
        self.reset_parameters()

    def reset_parameters(self):
        uniform(self.in_channels, self.weight)

    def score(self, x: Tensor, batch: Optional[Tensor] = None) -> Tensor:
        """the score of every node (topk.py:127-133)"""
        x = x.view(-1, 1) if x.dim() == 1 else x
        score = (x * self.weight).sum(dim=-1)
        if self.min_score is None:
            return self.act(score / self.weight.norm(p=2, dim=-1))
        if batch is None:
            batch = torch.zeros(x.size(0), dtype=torch.long, device=x.device)
        return group_softmax(score, batch)

    def pick(self, score: Tensor, batch: Optional[Tensor] = None) -> Tensor:
        """the kept nodes of a score vector"""
        if self.min_score is not None and batch is None:
            batch = torch.zeros(score.size(0), dtype=torch.long, device=score.device)
        return topk(score, self.ratio, batch, self.min_score, fuse=self.fuse)

    def forward(self, x: Tensor, batch: Optional[Tensor] = None) -> SelectOutput:
        score = self.score(x, batch)
        node_index = self.pick(score, batch)
        return SelectOutput(
            node_index=node_index,
            num_nodes=x.size(0),
            cluster_index=torch.arange(node_index.size(0), device=x.device),
            num_clusters=node_index.size(0),
            weight=score[node_index],
        )

    def __repr__(self) -> str:
        if self.min_score is None:
            arg = f'ratio={self.ratio}'
        else:
            arg = f'min_score={self.min_score}'
        return f'{self.__class__.__name__}({self.in_channels}, {arg})'
