import os
from typing import List, Optional, Tuple, Union

import torch
from torch import Tensor

from ... import _native
from ..._functions import GenAggregateFunction
from ...edge_index import as_edge_index
from ..aggr import Aggregation, MultiAggregation, SoftmaxAggregation
from ..dense.linear import Linear
from ..inits import reset
from ..norm import MessageNorm
from .message_passing import _FLOATS, _LOW, MessagePassing, _n_dst

# PYGAMD_FUSE_GEN=0: GENConv layers start with ``fuse = False`` (read at import)
FUSE_GEN = os.environ.get('PYGAMD_FUSE_GEN', '1') not in ('', '0')


class MLP(torch.nn.Sequential):
    """``Linear -> norm -> ReLU -> Dropout`` per hidden layer and a closing ``Linear``, with the
    module indices (and so the state-dict keys ``N.weight`` ...) of the reference's helper
    (torch_geometric/nn/conv/gen_conv.py:21-41); ``norm`` in ``batch | layer | instance | None``."""

    def __init__(self, channels: List[int], norm: Optional[str] = None, bias: bool = True,
                 dropout: float = 0.):
        mods = []
        last = len(channels) - 1
        for i in range(1, len(channels)):
            mods.append(Linear(channels[i - 1], channels[i], bias=bias))
            if i == last:
                break
            if norm == 'batch':
                mods.append(torch.nn.BatchNorm1d(channels[i], affine=True))
            elif norm == 'layer':
                mods.append(torch.nn.LayerNorm(channels[i], elementwise_affine=True))
            elif norm == 'instance':
                mods.append(torch.nn.InstanceNorm1d(channels[i], affine=False))
            elif norm:
                raise NotImplementedError(f'Normalization layer "{norm}" not supported.')
            mods.append(torch.nn.ReLU())
            mods.append(torch.nn.Dropout(dropout))
        super().__init__(*mods)


class GENConv(MessagePassing):
    r"""The generalized graph convolution of DeeperGCN with the constructor arguments, defaults,
    state-dict keys (``aggr_module.t`` / ``aggr_module.p``, ``lin_src.*``, ``lin_edge.*``,
    ``lin_dst.*``, ``lin_aggr_out.*``, ``mlp.N.*``, ``msg_norm.scale``), ``__repr__`` and forward
    semantics of ``torch_geometric.nn.GENConv`` (torch_geometric/nn/conv/gen_conv.py:44-243):

    .. math:: x_i' = \mathrm{MLP}\big(x_i + \mathrm{AGG}(\{\mathrm{ReLU}(x_j + e_{ji}) + \epsilon
              : j \in N(i)\})\big)

    ``aggr`` is ``softmax`` (default; ``softmax_sg`` = with ``semi_grad``), ``powermean``
    (``power``), any other aggregation or a list of them; ``aggr_kwargs`` overrides the
    aggregation's arguments.  ``x`` is a tensor, ``(x_src, x_dst)`` or ``(x_src, None)``.  Routes:

    * fused (device tensors, float32 after widening, 2-D ``x``, ``fuse`` true,
      ``flow='source_to_target'``, ``type(aggr_module) is SoftmaxAggregation``, ``edge_attr``
      absent, of width ``out_channels`` or with ``lin_edge``, and
      ``_native.gen_supported(out_channels, edge_dim or 0)``): ``propagate`` is ONE kernel per
      direction (``GenAggregateFunction``, csrc/gen.hip).  The message is rebuilt per slot in
      registers and every column keeps its own running softmax: nothing of size ``E x F`` is
      formed or saved.  ``lin_src``, ``msg_norm``, ``+ lin_dst(x_dst)`` and the MLP stay in torch,
      in the reference's order;
    * generic gather -> ``message`` -> ``aggr_module`` for everything else (host tensors,
      ``powermean``, ``add`` / ``mean`` / ``max``, lists, ``target_to_source``, ``fuse = False``,
      ``F > 512``, ``edge_dim > 32`` or ``F * edge_dim > 4096``).

    Half and bfloat16 device inputs are widened to float32 and the aggregate handed back in
    their dtype outside autocast.  ``fuse`` is a per-layer attribute initialised from the
    environment switch ``PYGAMD_FUSE_GEN`` (read at import, default ``1``)."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int,
                 aggr: Optional[Union[str, List[str], Aggregation]] = 'softmax', t: float = 1.0,
                 learn_t: bool = False, p: float = 1.0, learn_p: bool = False,
                 msg_norm: bool = False, learn_msg_scale: bool = False, norm: str = 'batch',
                 num_layers: int = 2, expansion: int = 2, eps: float = 1e-7, bias: bool = False,
                 edge_dim: Optional[int] = None, **kwargs):
        semi_grad = aggr == 'softmax_sg'
        aggr = {'softmax_sg': 'softmax', 'power': 'powermean'}.get(aggr, aggr) \
            if isinstance(aggr, str) else aggr
        if 'aggr_kwargs' not in kwargs:
            if aggr == 'softmax':
                kwargs['aggr_kwargs'] = dict(t=t, learn=learn_t, semi_grad=semi_grad)
            elif aggr == 'powermean':
                kwargs['aggr_kwargs'] = dict(p=p, learn=learn_p)
        name = aggr
        if isinstance(aggr, (list, tuple)):
            name = [str(a) for a in aggr]
            aggr = MultiAggregation(list(aggr), **(kwargs.pop('aggr_kwargs', None) or {}))
        elif isinstance(aggr, Aggregation):
            name = str(aggr)
        super().__init__(aggr=aggr, **kwargs)
        self.aggr = name

        self.in_channels = in_channels
        self.out_channels = out_channels
        self.eps = eps
        self.edge_dim = edge_dim
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        if in_channels[0] != out_channels:
            self.lin_src = Linear(in_channels[0], out_channels, bias=bias)
        if edge_dim is not None and edge_dim != out_channels:
            self.lin_edge = Linear(edge_dim, out_channels, bias=bias)
        aggr_out = out_channels
        if isinstance(self.aggr_module, MultiAggregation):
            aggr_out = self.aggr_module.get_out_channels(out_channels)
        if aggr_out != out_channels:
            self.lin_aggr_out = Linear(aggr_out, out_channels, bias=bias)
        if in_channels[1] != out_channels:
            self.lin_dst = Linear(in_channels[1], out_channels, bias=bias)
        hidden = [out_channels * expansion] * (num_layers - 1)
        self.mlp = MLP([out_channels] + hidden + [out_channels], norm=norm, bias=bias)
        if msg_norm:
            self.msg_norm = MessageNorm(learn_msg_scale)
        self.fuse = FUSE_GEN

    def reset_parameters(self):
        super().reset_parameters()
        reset(self.mlp)
        for name in ('msg_norm', 'lin_src', 'lin_edge', 'lin_aggr_out', 'lin_dst'):
            if hasattr(self, name):
                getattr(self, name).reset_parameters()

    # -- the fused route of propagate --------------------------------------------------------------
    def _fusable(self, x_src: Tensor, edge_attr: Optional[Tensor]) -> bool:
        if not (self.fuse and x_src.is_cuda and x_src.dim() == 2 and x_src.dtype in _FLOATS
                and self.flow == 'source_to_target'
                and type(self.aggr_module) is SoftmaxAggregation):
            return False
        F = x_src.size(1)
        De = 0
        if edge_attr is not None:
            if not (isinstance(edge_attr, Tensor) and edge_attr.is_cuda and edge_attr.dim() == 2
                    and edge_attr.dtype in _FLOATS):
                return False
            De = edge_attr.size(1) if hasattr(self, 'lin_edge') else 0
            if edge_attr.size(1) != (self.lin_edge.in_channels if De else F):
                return False
        mod = self.aggr_module
        if mod.channels not in (1, F):
            return False
        return _native.gen_supported(F, De)

    def _fused(self, x_src: Tensor, edge_index, edge_attr: Optional[Tensor], n_dst: int) -> Tensor:
        graph = as_edge_index(edge_index, x_src.size(0), n_dst)
        weight = bias = None
        if edge_attr is not None:
            edge_attr = edge_attr.float()
            if hasattr(self, 'lin_edge'):
                weight = self.lin_edge.weight.float()
                bias = None if self.lin_edge.bias is None else self.lin_edge.bias.float()
        mod = self.aggr_module
        if isinstance(mod.t, Tensor):
            t = mod.t.float()
        else:
            t = torch.full((1, ), float(mod.t), dtype=torch.float32, device=x_src.device)
        return GenAggregateFunction.apply(x_src.float(), edge_attr, weight, bias, t, graph, n_dst,
                                          float(self.eps), bool(mod.semi_grad))

    def forward(self, x: Union[Tensor, Tuple[Tensor, Optional[Tensor]]], edge_index,
                edge_attr: Optional[Tensor] = None, size=None) -> Tensor:
        if isinstance(x, Tensor):
            x = (x, x)
        if hasattr(self, 'lin_src'):
            x = (self.lin_src(x[0]), x[1])
        x_src = x[0]
        if self._fusable(x_src, edge_attr):
            low = x_src.dtype if x_src.dtype in _LOW else None
            out = self._fused(x_src, edge_index, edge_attr,
                              _n_dst(self, x_src, x[1], edge_index, size))
            if low is not None and not torch.is_autocast_enabled():
                out = out.to(low)
        else:
            out = self.propagate(edge_index, x=x, edge_attr=edge_attr, size=size)
        if hasattr(self, 'lin_aggr_out'):
            out = self.lin_aggr_out(out)
        n = out.size(0)  # (destinations may be a prefix of x_dst's rows)
        if hasattr(self, 'msg_norm'):
            h = x[1] if x[1] is not None else x[0]
            out = self.msg_norm(h[:n], out)
        x_dst = x[1]
        if x_dst is not None:
            if hasattr(self, 'lin_dst'):
                x_dst = self.lin_dst(x_dst)
            out = out + x_dst[:n]
        return self.mlp(out)

    def message(self, x_j: Tensor, edge_attr: Optional[Tensor]) -> Tensor:
        if edge_attr is not None and hasattr(self, 'lin_edge'):
            edge_attr = self.lin_edge(edge_attr)
        if edge_attr is not None:
            assert x_j.size(-1) == edge_attr.size(-1)
        msg = x_j if edge_attr is None else x_j + edge_attr
        return msg.relu() + self.eps

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, {self.out_channels}, '
                f'aggr={self.aggr})')

