import os
from typing import Optional

import torch
from torch import Tensor

from ... import _norm

# PYGAMD_FUSE_NORM=0: GraphNorm and LayerNorm layers start with ``fuse = False`` (read at import)
FUSE_NORM = os.environ.get('PYGAMD_FUSE_NORM', '1').strip() not in ('', '0')


class GraphNorm(torch.nn.Module):
    r"""Graph normalisation with the constructor arguments, the state-dict keys (``weight``,
    ``bias``, ``mean_scale``) and the ``__repr__`` of ``torch_geometric.nn.norm.GraphNorm``
    (torch_geometric/nn/norm/graph_norm.py:12-79):

    .. math:: \mathbf{x}^{\prime}_i = \frac{\mathbf{x} - \alpha \odot \textrm{E}[\mathbf{x}]}
              {\sqrt{\textrm{Var}[\mathbf{x} - \alpha \odot \textrm{E}[\mathbf{x}]] + \epsilon}}
              \odot \gamma + \beta

    with mean and variance per graph of the mini-batch and per channel.  ``batch=None`` is one
    graph of all rows.  Routes:

    * fused (csrc/graph_norm.hip): float device inputs with ``in_channels <= 512`` and a
      non-decreasing ``batch`` vector.  One launch forward, two backward (three and four when a
      graph is longer than the kernel's threshold); only ``x`` and the per-graph statistics are
      kept for the backward.  The by-graph handle is cached per ``batch`` tensor, so the norm
      layers of one step share it.  Half and bfloat16 inputs are widened to float32 and the
      result handed back in their dtype outside autocast;
    * generic: the reference's two scatters and two index selects, for host tensors, other
      dtypes, wider inputs, an unsorted ``batch`` and ``fuse = False``.

    ``fuse`` is a per-layer attribute initialised from the environment switch
    ``PYGAMD_FUSE_NORM`` (read at import, default ``1``)."""

    def __init__(self, in_channels: int, eps: float = 1e-5, device=None):
        super().__init__()
        self.in_channels = in_channels
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.empty(in_channels, device=device))
        self.bias = torch.nn.Parameter(torch.empty(in_channels, device=device))
        self.mean_scale = torch.nn.Parameter(torch.empty(in_channels, device=device))
        self.fuse = FUSE_NORM
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            self.weight.fill_(1.0)
            self.bias.fill_(0.0)
            self.mean_scale.fill_(1.0)

    def forward(self, x: Tensor, batch: Optional[Tensor] = None,
                batch_size: Optional[int] = None) -> Tensor:
        if _norm.fusable(x, batch, self.fuse) and x.size(1) == self.in_channels:
            out = _norm.fused(x, batch, batch_size, self.weight, self.bias, self.mean_scale,
                              self.eps, 'channel')
            if out is not None:
                return out
        return _norm.graph_norm_generic(x, batch, batch_size, self.weight, self.bias,
                                        self.mean_scale, self.eps)

    def __repr__(self):
        return f'{self.__class__.__name__}({self.in_channels})'
