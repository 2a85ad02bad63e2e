from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor


class BatchNorm(torch.nn.Module):
    r"""Batch normalisation over all nodes of a mini-batch: ``torch.nn.BatchNorm1d`` held as
    ``self.module``, with the constructor arguments, the state-dict keys (``module.*``) and the
    ``__repr__`` of ``torch_geometric.nn.norm.BatchNorm``
    (torch_geometric/nn/norm/batch_norm.py:11-94).  ``allow_single_element`` lets a batch of one
    row pass in training mode by normalising it with the running statistics.  No kernel of this
    package: it exists so that ``norm='batch_norm'`` resolves."""

    def __init__(self, in_channels: int, eps: float = 1e-5, momentum: Optional[float] = 0.1,
                 affine: bool = True, track_running_stats: bool = True,
                 allow_single_element: bool = False, device=None):
        super().__init__()
        if allow_single_element and not track_running_stats:
            raise ValueError("'allow_single_element' requires 'track_running_stats' to be set "
                             "to `True`")
        self.module = torch.nn.BatchNorm1d(in_channels, eps, momentum, affine,
                                           track_running_stats, device=device)
        self.in_channels = in_channels
        self.allow_single_element = allow_single_element

    def reset_running_stats(self):
        self.module.reset_running_stats()

    def reset_parameters(self):
        self.module.reset_parameters()

    def forward(self, x: Tensor) -> Tensor:
        bn = self.module
        if self.allow_single_element and x.size(0) <= 1:
            return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False,
                                0.0, bn.eps)
        return bn(x)

    def __repr__(self):
        return f'{self.__class__.__name__}({self.module.extra_repr()})'
