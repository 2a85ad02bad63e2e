from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.utils.checkpoint import checkpoint


class DeepGCNLayer(torch.nn.Module):
    r"""The skip-connection wrapper of DeepGCN / DeeperGCN with the constructor arguments and
    ``__repr__`` of ``torch_geometric.nn.models.DeepGCNLayer``
    (torch_geometric/nn/models/deepgcn.py:10-120).  ``block``:

    * ``res+``: norm -> act -> dropout -> conv, then ``x + h``;
    * ``res`` / ``dense`` / ``plain``: conv -> norm -> act, then ``x + h`` / ``cat([x, h])`` /
      ``h``, then dropout.

    ``ckpt_grad`` recomputes the convolution in the backward instead of keeping its activations
    (only while its input requires a gradient).  The first positional argument of ``forward`` is
    ``x``; everything else is handed to ``conv``.  Pure torch."""

    BLOCKS = ('res+', 'res', 'dense', 'plain')

    def __init__(self, conv: Optional[torch.nn.Module] = None,
                 norm: Optional[torch.nn.Module] = None, act: Optional[torch.nn.Module] = None,
                 block: str = 'res+', dropout: float = 0., ckpt_grad: bool = False):
        super().__init__()
        self.conv, self.norm, self.act = conv, norm, act
        self.block = block.lower()
        assert self.block in self.BLOCKS
        self.dropout = dropout
        self.ckpt_grad = ckpt_grad

    def reset_parameters(self):
        self.conv.reset_parameters()
        self.norm.reset_parameters()

    def _conv(self, h: Tensor, args, kwargs) -> Tensor:
        if self.conv is not None and self.ckpt_grad and h.requires_grad:
            return checkpoint(self.conv, h, *args, use_reentrant=True, **kwargs)
        return self.conv(h, *args, **kwargs)

    def _norm_act(self, h: Tensor) -> Tensor:
        if self.norm is not None:
            h = self.norm(h)
        return h if self.act is None else self.act(h)

    def forward(self, *args, **kwargs) -> Tensor:
        x, args = args[0], args[1:]
        if self.block == 'res+':
            h = F.dropout(self._norm_act(x), p=self.dropout, training=self.training)
            return x + self._conv(h, args, kwargs)
        h = self._norm_act(self._conv(x, args, kwargs))
        if self.block == 'res':
            h = x + h
        elif self.block == 'dense':
            h = torch.cat([x, h], dim=-1)
        return F.dropout(h, p=self.dropout, training=self.training)

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}(block={self.block})'
