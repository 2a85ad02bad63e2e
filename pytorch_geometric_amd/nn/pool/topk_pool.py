from typing import Callable, Optional, Tuple, Union

import torch
from torch import Tensor

from ._fuse import LOW as _LOW
from ._fuse import fuse_default
from .connect import FilterEdges
from .select import SelectOutput, SelectTopK


def scale_rows(x: Tensor, score: Tensor, perm: Tensor, multiplier: float,
               fuse: bool) -> Tuple[Tensor, Tensor]:
    """``(multiplier * (x[perm] * score[perm].view(-1, 1)), score[perm])`` (topk_pool.py:118-122).
    Fused (csrc/pool.hip through ``GatherScaleFunction``): float32 (or half / bfloat16, widened)
    device ``x [N, F]`` with its ``[N]`` scores and an int64 ``perm``."""
    if (fuse and x.is_cuda and x.dim() == 2 and x.size(1) >= 1 and x.dtype == score.dtype
            and x.dtype in (torch.float32, ) + _LOW and score.is_cuda and score.dim() == 1
            and score.numel() == x.size(0) and perm.is_cuda and perm.dtype == torch.int64):
        from ..._functions import GatherScaleFunction
        low = x.dtype if x.dtype in _LOW else None
        with torch.autocast('cuda', enabled=False):
            out, weight = GatherScaleFunction.apply(x.float(), score.float(), perm,
                                                    float(multiplier))
        if low is not None:
            out, weight = out.to(low), weight.to(low)
        return out, weight
    weight = score[perm]
    out = x[perm] * weight.view(-1, 1)
    return (multiplier * out if multiplier != 1 else out), weight


class HierarchicalPooling(torch.nn.Module):
    """What :class:`TopKPooling` and :class:`SAGPooling` share: the ``fuse`` switch over the
    select and connect modules and the forward from the nodes' attention input on."""

    @property
    def fuse(self) -> bool:
        return self.select.fuse

    @fuse.setter
    def fuse(self, value: bool) -> None:
        self.select.fuse = self.connect.fuse = bool(value)

    def _pool(self, x: Tensor, attn: Tensor, edge_index: Tensor, edge_attr: Optional[Tensor],
              batch: Optional[Tensor]):
        score = self.select.score(attn, batch)
        perm = self.select.pick(score, batch)
        x, weight = scale_rows(x, score, perm, self.multiplier, self.fuse)
        num = perm.size(0)
        select_out = SelectOutput(perm, score.size(0), torch.arange(num, device=perm.device), num,
                                  weight)
        if batch is None:
            batch = edge_index.new_zeros(score.size(0))
        connect_out = self.connect(select_out, edge_index, edge_attr, batch)
        return (x, connect_out.edge_index, connect_out.edge_attr, connect_out.batch, perm, weight)


class TopKPooling(HierarchicalPooling):
    r""":math:`\mathrm{top}_k` pooling with the constructor arguments, the ``forward`` arguments,
    the six-tuple result ``(x, edge_index, edge_attr, batch, perm, score)``, the parameter
    (``select.weight``) and the ``__repr__`` of ``torch_geometric.nn.TopKPooling``
    (torch_geometric/nn/pool/topk_pool.py:11-136):

    .. math:: \mathbf{y} = \sigma(\mathbf{X}\mathbf{p} / \|\mathbf{p}\|), \quad \mathbf{i} =
              \mathrm{top}_k(\mathbf{y}), \quad \mathbf{X}^{\prime} = (\mathbf{X} \odot
              \mathbf{y})_{\mathbf{i}}, \quad \mathbf{A}^{\prime} = \mathbf{A}_{\mathbf{i},\mathbf{i}}

    (``min_score``: :math:`\mathbf{y} = \mathrm{softmax}(\mathbf{X}\mathbf{p})` per graph and
    :math:`\mathbf{i} = \mathbf{y}_i > \tilde{\alpha}`).  Routes:

    * fused (csrc/pool.hip): the per-graph select in one launch over the cached by-graph handle of
      the ``batch`` tensor, the gather of the kept rows with both multiplications in one launch
      (two with the memset in the backward) and the edge filter in three; each step falls back on
      its own when its conditions do not hold (:func:`~.select.topk`, :func:`scale_rows`,
      :func:`~.connect.filter_adj`);
    * generic: the reference's expressions, for host tensors, other dtypes, an unsorted
      ``batch``, graphs of more than 1,024 nodes and ``fuse = False``.

    Both order a graph's nodes by score descending, then node index ascending.  ``fuse`` is a
    per-layer attribute initialised from ``PYGAMD_FUSE_POOL`` (read at import) or, when that is
    unset, from the layer's measured default (:mod:`._fuse`, profiles/hier_pool.md: on)."""

    def __init__(self, in_channels: int, ratio: Union[int, float] = 0.5,
                 min_score: Optional[float] = None, multiplier: float = 1.,
                 nonlinearity: Union[str, Callable] = 'tanh'):
        super().__init__()
        self.in_channels = in_channels
        self.ratio = ratio
        self.min_score = min_score
        self.multiplier = multiplier
        self.select = SelectTopK(in_channels, ratio, min_score, nonlinearity)
        self.connect = FilterEdges()
        self.fuse = fuse_default('TopKPooling')
        self.reset_parameters()

    def reset_parameters(self):
        self.select.reset_parameters()

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Optional[Tensor] = None,
                batch: Optional[Tensor] = None, attn: Optional[Tensor] = None
                ) -> Tuple[Tensor, Tensor, Optional[Tensor], Optional[Tensor], Tensor, Tensor]:
        attn = x if attn is None else attn
        return self._pool(x, attn, edge_index, edge_attr, batch)

    def __repr__(self) -> str:
        if self.min_score is None:
            ratio = f'ratio={self.ratio}'
        else:
            ratio = f'min_score={self.min_score}'
        return (f'{self.__class__.__name__}({self.in_channels}, {ratio}, '
                f'multiplier={self.multiplier})')
