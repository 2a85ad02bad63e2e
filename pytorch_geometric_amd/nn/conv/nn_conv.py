from typing import Callable, Optional, Tuple, Union

import torch
from torch import Tensor
from torch.nn import Parameter

from ... import _native
from ..._functions import MixtureConvFunction, linear
from ...edge_index import as_edge_index
from ..dense.linear import Linear
from ..inits import reset, zeros
from . import gmm_conv
from .gmm_conv import device_floats, fold_mean, stock_flow
from .message_passing import _LOW, MessagePassing, _n_dst

_LINEARS = (torch.nn.Linear, Linear)


def _hooked(module: torch.nn.Module) -> bool:
    return bool(module._forward_hooks or module._forward_pre_hooks)


class NNConv(MessagePassing):
    r"""The edge-conditioned convolution (the MPNN layer of "Neural Message Passing for Quantum
    Chemistry") with the constructor arguments, state-dict keys (``nn.*``, ``lin.weight``,
    ``bias``) and forward semantics of ``torch_geometric.nn.NNConv``
    (torch_geometric/nn/conv/nn_conv.py:13-126):

    .. math:: x_i' = \Theta x_i + \sum_{j \in N(i)} x_j \cdot h_\Theta(e_{ij})

    with ``h`` the edge network ``nn``: ``[E, D] -> [E, F_src * out_channels]``.  ``x`` is a tensor
    or a ``(x_src, x_dst)`` pair; ``in_channels = -1`` (lazy initialisation) is refused.  Routes:

    * fused: when ``nn`` ends in an affine map — it is a ``torch.nn.Linear`` / this package's
      ``Linear``, or a ``torch.nn.Sequential`` whose last child is one, of ``F * M`` outputs, and
      neither carries forward hooks — the per-edge matrix is ``reshape(W_last h_e + b_last)`` with
      ``h = nn[:-1](edge_attr)`` (the raw ``edge_attr`` for a bare ``Linear``), i.e. a mixture of
      ``K' = in_features + 1`` fixed ``[F, M]`` matrices with the coefficients ``[h | 1]``.  The
      propagate is then ``MixtureConvFunction`` (csrc/mixture.hip): the weighted rows are summed
      per destination FIRST and transformed after, and the reference's ``[E, F, M]`` never exists,
      forward or backward.  Further conditions: device tensors (float32 after widening), ``fuse``
      true, ``flow='source_to_target'``, ``aggr`` in add / sum / mean (the reciprocal in-degree is
      folded into the coefficients for ``mean``), ``_native.mixture_supported(max(F, M), K')`` and
      the byte rule ``K' * N_dst <= E * M`` and ``K' * N_src <= E * F``: the per-node planes
      ``[N_dst, K' * F]`` and ``[N_src, K' * M]`` are then no larger than the ``[E, F, M]`` tensor
      they replace.  The byte rule is a count of bytes, not a measurement;
    * the reference's gather -> ``message`` -> aggregate for everything else (``aggr='max'``, an
      edge network that ends in an activation, host tensors, ...) — and whenever the message flow
      is observed or replaced: a propagate, message or aggregate hook, explain mode, or a subclass
      with its own ``message``, ``aggregate``, ``update`` or ``propagate``.

    Half and bfloat16 device inputs are widened to float32 and the result handed back in their
    dtype outside autocast.  ``fuse`` is a per-layer attribute initialised from the environment
    switch ``PYGAMD_FUSE_MIXTURE`` (read at import, default ``1``)."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, nn: Callable,
                 aggr: str = 'add', root_weight: bool = True, bias: bool = True, **kwargs):
        super().__init__(aggr=aggr, **kwargs)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.nn = nn
        self.root_weight = root_weight
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        if in_channels[0] <= 0 or in_channels[1] <= 0:
            raise ValueError("lazy initialisation (in_channels=-1) is not supported")
        self.in_channels_l = in_channels[0]
        if root_weight:
            self.lin = Linear(in_channels[1], out_channels, bias=False,
                              weight_initializer='uniform')
        else:
            self.lin = None
        if bias:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.fuse = gmm_conv.FUSE_MIXTURE
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        reset(self.nn)
        if self.lin is not None:
            self.lin.reset_parameters()
        zeros(self.bias)

    def _edge_network(self):
        """``(head | None, last)`` when ``nn`` ends in an affine map of ``F * M`` outputs that
        nobody observes, else None"""
        net, head = self.nn, None
        if isinstance(net, torch.nn.Sequential) and len(net) > 0:
            if _hooked(net):
                return None
            head, net = (net[:-1] if len(net) > 1 else None), net[-1]
        if not isinstance(net, _LINEARS) or _hooked(net):
            return None
        if net.weight.dim() != 2 or net.weight.size(0) != self.in_channels_l * self.out_channels:
            return None
        return head, net

    def _fusable_shapes(self, n_src: int, n_dst: int, E: int) -> bool:
        """the conditions of the fused route that need no tensor: the switches, the edge network,
        the kernels' envelope and the byte rule"""
        if not (self.fuse and self.flow == 'source_to_target'
                and self.aggr in ('add', 'sum', 'mean') and stock_flow(self, NNConv)):
            return False
        found = self._edge_network()
        if found is None:
            return False
        F, M = self.in_channels_l, self.out_channels
        K = found[1].weight.size(1) + 1
        if K * n_dst > E * M or K * n_src > E * F:
            return False
        return _native.mixture_supported(max(F, M), K)

    def _fusable(self, x_src, x_dst, edge_index, edge_attr, size) -> bool:
        if not (device_floats(x_src, edge_attr) and (x_dst is None or device_floats(x_dst))
                and x_src.size(1) == self.in_channels_l):
            return False
        E = edge_attr.size(0)
        return self._fusable_shapes(x_src.size(0), _n_dst(self, x_src, x_dst, edge_index, size), E)

    def forward(self, x: Union[Tensor, Tuple[Tensor, Optional[Tensor]]], edge_index,
                edge_attr: Optional[Tensor] = None, size=None) -> Tensor:
        if isinstance(x, Tensor):
            x = (x, x)
        if self._fusable(x[0], x[1], edge_index, edge_attr, size):
            return self._forward_fused(x[0], x[1], edge_index, edge_attr, size)
        out = self.propagate(edge_index, x=x, edge_attr=edge_attr, size=size)
        if x[1] is not None and self.lin is not None:
            out = out + self.lin(x[1])
        if self.bias is not None:
            out = out + self.bias
        return out

    def _forward_fused(self, x_src: Tensor, x_dst: Optional[Tensor], edge_index,
                       edge_attr: Tensor, size) -> Tensor:
        F, M = self.in_channels_l, self.out_channels
        head, last = self._edge_network()
        low = x_src.dtype if x_src.dtype in _LOW else None
        xs = x_src.float()
        n_dst = _n_dst(self, x_src, x_dst, edge_index, size)
        graph = as_edge_index(edge_index, xs.size(0), n_dst)
        h = edge_attr if head is None else head(edge_attr)
        with torch.autocast('cuda', enabled=False):
            h = h.float()
            weight = last.weight.float().view(F, M, -1).permute(2, 0, 1)
            if last.bias is not None:
                h = torch.cat([h, h.new_ones(h.size(0), 1)], dim=1)
                weight = torch.cat([weight, last.bias.float().view(1, F, M)])
            out = MixtureConvFunction.apply(xs, fold_mean(h, graph, self.aggr), weight, graph,
                                            n_dst)
            if x_dst is not None and self.lin is not None:
                xd = xs if x_dst is x_src else x_dst.float()
                out = out + linear(xd, self.lin.weight.float())[:n_dst]
            if self.bias is not None:
                out = out + self.bias.float()
        if low is not None and not torch.is_autocast_enabled():
            out = out.to(low)
        return out

    def message(self, x_j: Tensor, edge_attr: Tensor) -> Tensor:
        weight = self.nn(edge_attr)
        weight = weight.view(-1, self.in_channels_l, self.out_channels)
        return torch.matmul(x_j.unsqueeze(1), weight).squeeze(1)

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, {self.out_channels}, '
                f'aggr={self.aggr}, nn={self.nn})')
