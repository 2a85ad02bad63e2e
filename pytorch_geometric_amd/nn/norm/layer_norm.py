from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from ... import _norm
from .graph_norm import FUSE_NORM


class LayerNorm(torch.nn.Module):
    r"""Layer normalisation over each graph of a mini-batch (``mode='graph'``) or over each node
    (``mode='node'``) with the constructor arguments, the state-dict keys (``weight``, ``bias``;
    none with ``affine=False``) and the ``__repr__`` of ``torch_geometric.nn.norm.LayerNorm``
    (torch_geometric/nn/norm/layer_norm.py:15-116).

    ``mode='graph'`` takes one mean and one variance per graph over all its nodes and channels.
    As in the reference, a call WITHOUT a batch vector divides by ``std + eps`` and a call with
    one by ``sqrt(var + eps)`` (layer_norm.py:87-88, 105).  Its routes are those of
    :class:`GraphNorm`: the fused kernels of csrc/graph_norm.hip for float device inputs with
    ``in_channels <= 512`` and a non-decreasing ``batch``, the reference's scatters otherwise
    (``fuse``, from ``PYGAMD_FUSE_NORM``).  ``mode='node'`` is ``F.layer_norm``.  An unknown mode
    raises at ``forward``, as in the reference."""

    def __init__(self, in_channels: int, eps: float = 1e-5, affine: bool = True,
                 mode: str = 'graph', device=None):
        super().__init__()
        self.in_channels = in_channels
        self.eps = eps
        self.affine = affine
        self.mode = mode
        if affine:
            self.weight = torch.nn.Parameter(torch.empty(in_channels, device=device))
            self.bias = torch.nn.Parameter(torch.empty(in_channels, device=device))
        else:
            self.register_parameter('weight', None)
            self.register_parameter('bias', None)
        self.fuse = FUSE_NORM
        self.reset_parameters()

    def reset_parameters(self):
        if self.weight is not None:
            with torch.no_grad():
                self.weight.fill_(1.0)
                self.bias.fill_(0.0)

    def forward(self, x: Tensor, batch: Optional[Tensor] = None,
                batch_size: Optional[int] = None) -> Tensor:
        if self.mode == 'graph':
            if _norm.fusable(x, batch, self.fuse) and x.size(1) == self.in_channels:
                out = _norm.fused(x, batch, batch_size, self.weight, self.bias, None, self.eps,
                                  'graph')
                if out is not None:
                    return out
            return _norm.layer_norm_graph_generic(x, batch, batch_size, self.weight, self.bias,
                                                  self.eps)
        if self.mode == 'node':
            return F.layer_norm(x, (self.in_channels, ), self.weight, self.bias, self.eps)
        raise ValueError(f"Unknownn normalization mode: {self.mode}")

    def __repr__(self):
        return (f'{self.__class__.__name__}({self.in_channels}, '
                f'affine={self.affine}, mode={self.mode})')
