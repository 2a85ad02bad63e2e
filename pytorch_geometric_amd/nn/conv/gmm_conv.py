import os
from typing import Optional, Tuple, Union

import torch
from torch import Tensor
from torch.nn import Parameter

from ... import _native
from ..._functions import MixtureConvFunction, linear
from ...edge_index import as_edge_index
from ..dense.linear import Linear
from ..inits import glorot, zeros
from .gcn_conv import _FLOW_HOOKS
from .message_passing import _FLOATS, _LOW, MessagePassing, _n_dst

# PYGAMD_FUSE_MIXTURE=0: GMMConv and NNConv layers start with ``fuse = False`` (read at import).
# The default is 1: fused is faster at all three shapes of profiles/mixture_conv.md.
FUSE_MIXTURE = os.environ.get('PYGAMD_FUSE_MIXTURE', '1') not in ('', '0')


def stock_flow(layer: MessagePassing, base: type) -> bool:
    """nobody observes or replaces the message flow of ``layer``, an instance of ``base`` or of a
    subclass (``ResGatedGraphConv._stock_flow``'s test)"""
    kind = type(layer)
    for name in ('message', 'aggregate', 'update', 'propagate'):
        if getattr(kind, name) is not getattr(base, name):
            return False
    if getattr(layer, 'explain', False):
        return False
    return not any(getattr(layer, name, None) for name in _FLOW_HOOKS)


def device_floats(*tensors) -> bool:
    """every tensor is a two-dimensional float32 / half / bfloat16 device tensor"""
    return all(isinstance(t, Tensor) and t.is_cuda and t.dim() == 2 and t.dtype in _FLOATS
               for t in tensors)


def fold_mean(coef: Tensor, graph, aggr: str) -> Tensor:
    """``coef [E, K]`` with the reciprocal in-degree of every edge's destination folded in for the
    mean aggregation (a sum of such messages is the mean; destinations without edges keep 0)"""
    if aggr != 'mean':
        return coef
    inv = graph.by_dst().inv_degree()
    return coef * inv[graph.edge_index[1].long()].unsqueeze(1)


class GMMConv(MessagePassing):
    r"""The Gaussian mixture model convolution (MoNet) with the constructor arguments, state-dict
    keys (``g``, ``mu``, ``sigma``, ``root.weight``, ``bias``) and forward semantics of
    ``torch_geometric.nn.GMMConv`` (torch_geometric/nn/conv/gmm_conv.py:13-202):

    .. math:: x_i' = \frac{1}{|N(i)|} \sum_{j \in N(i)} \sum_{k=1}^K w_k(e_{ij}) \odot \Theta_k x_j,
        \quad w_k(e) = \exp(-\tfrac12 (e - \mu_k)^T \Sigma_k^{-1} (e - \mu_k))

    ``x`` is a tensor or a ``(x_src, x_dst)`` pair; ``in_channels = -1`` (lazy initialisation) is
    refused.  Routes:

    * fused (device tensors, float32 after widening, ``fuse`` true, ``flow='source_to_target'``,
      ``aggr`` in add / sum / mean, ``separate_gaussians=False`` and
      ``_native.mixture_supported(F_src, kernel_size)``): the Gaussian weights are tensor code at
      ``[E, K]`` (the reciprocal in-degree folded in for ``mean``) and the propagate is
      ``MixtureConvFunction`` with ``weight = g.view(F, K, M).permute(1, 0, 2)``: the weighted rows
      are summed per destination FIRST (csrc/mixture.hip, one gathered row of ``F`` floats per
      edge) and transformed after, so the reference's ``[E, K, M]`` never exists, forward or
      backward.  The root product and the bias are added outside;
    * the reference's gather -> ``message`` -> aggregate for everything else — and whenever the
      message flow is observed or replaced: a propagate, message or aggregate hook, explain mode,
      or a subclass with its own ``message``, ``aggregate``, ``update`` or ``propagate``.

    Half and bfloat16 device inputs are widened to float32 and the result handed back in their
    dtype outside autocast.  ``fuse`` is a per-layer attribute initialised from the environment
    switch ``PYGAMD_FUSE_MIXTURE`` (read at import, default ``1``)."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, dim: int,
                 kernel_size: int, separate_gaussians: bool = False, aggr: str = 'mean',
                 root_weight: bool = True, bias: bool = True, **kwargs):
        super().__init__(aggr=aggr, **kwargs)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.dim = dim
        self.kernel_size = kernel_size
        self.separate_gaussians = separate_gaussians
        self.root_weight = root_weight
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        if in_channels[0] <= 0 or in_channels[1] <= 0:
            raise ValueError("lazy initialisation (in_channels=-1) is not supported")
        self.rel_in_channels = in_channels[0]
        self.g = Parameter(torch.empty(in_channels[0], out_channels * kernel_size))
        if not separate_gaussians:
            self.mu = Parameter(torch.empty(kernel_size, dim))
            self.sigma = Parameter(torch.empty(kernel_size, dim))
        else:
            self.mu = Parameter(torch.empty(in_channels[0], out_channels, kernel_size, dim))
            self.sigma = Parameter(torch.empty(in_channels[0], out_channels, kernel_size, dim))
        if root_weight:
            self.root = Linear(in_channels[1], out_channels, bias=False,
                               weight_initializer='glorot')
        else:
            self.root = None
        if bias:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.fuse = FUSE_MIXTURE
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        glorot(self.g)
        glorot(self.mu)
        glorot(self.sigma)
        if self.root is not None:
            self.root.reset_parameters()
        zeros(self.bias)

    def _fusable(self, x_src: Tensor, x_dst, edge_attr) -> bool:
        if not stock_flow(self, GMMConv):
            return False
        if not (self.fuse and self.flow == 'source_to_target' and not self.separate_gaussians
                and self.aggr in ('add', 'sum', 'mean') and device_floats(x_src, edge_attr)
                and (x_dst is None or device_floats(x_dst))
                and x_src.size(1) == self.rel_in_channels and edge_attr.size(1) == self.dim):
            return False
        return _native.mixture_supported(self.rel_in_channels, self.kernel_size)

    def forward(self, x: Union[Tensor, Tuple[Tensor, Optional[Tensor]]], edge_index,
                edge_attr: Optional[Tensor] = None, size=None) -> Tensor:
        if isinstance(x, Tensor):
            x = (x, x)
        if self._fusable(x[0], x[1], edge_attr):
            return self._forward_fused(x[0], x[1], edge_index, edge_attr, size)
        if not self.separate_gaussians:
            out = self.propagate(edge_index, x=(torch.matmul(x[0], self.g), x[1]),
                                 edge_attr=edge_attr, size=size)
        else:
            out = self.propagate(edge_index, x=x, edge_attr=edge_attr, size=size)
        if x[1] is not None and self.root is not None:
            out = out + self.root(x[1])
        if self.bias is not None:
            out = out + self.bias
        return out

    def gaussian(self, edge_attr: Tensor, mu: Optional[Tensor] = None,
                 sigma: Optional[Tensor] = None) -> Tensor:
        """``w [E, K]`` of gmm_conv.py:160-163 (``mu``, ``sigma``: the parameters in another dtype)"""
        EPS = 1e-15
        (E, D), K = edge_attr.size(), self.kernel_size
        mu = self.mu if mu is None else mu
        sigma = self.sigma if sigma is None else sigma
        gaussian = -0.5 * (edge_attr.view(E, 1, D) - mu.view(1, K, D)).pow(2)
        gaussian = gaussian / (EPS + sigma.view(1, K, D).pow(2))
        return torch.exp(gaussian.sum(dim=-1))

    def _forward_fused(self, x_src: Tensor, x_dst: Optional[Tensor], edge_index,
                       edge_attr: Tensor, size) -> Tensor:
        F, M, K = self.rel_in_channels, self.out_channels, self.kernel_size
        low = x_src.dtype if x_src.dtype in _LOW else None
        xs = x_src.float()
        n_dst = _n_dst(self, x_src, x_dst, edge_index, size)
        graph = as_edge_index(edge_index, xs.size(0), n_dst)
        with torch.autocast('cuda', enabled=False):
            coef = self.gaussian(edge_attr.float(), self.mu.float(), self.sigma.float())
            coef = fold_mean(coef, graph, self.aggr)
            weight = self.g.float().view(F, K, M).permute(1, 0, 2)
            out = MixtureConvFunction.apply(xs, coef, weight, graph, n_dst)
            if x_dst is not None and self.root is not None:
                xd = xs if x_dst is x_src else x_dst.float()
                out = out + linear(xd, self.root.weight.float())[:n_dst]
            if self.bias is not None:
                out = out + self.bias.float()
        if low is not None and not torch.is_autocast_enabled():
            out = out.to(low)
        return out

    def message(self, x_j: Tensor, edge_attr: Tensor) -> Tensor:
        EPS = 1e-15
        F, M = self.rel_in_channels, self.out_channels
        (E, D), K = edge_attr.size(), self.kernel_size
        if not self.separate_gaussians:
            return (x_j.view(E, K, M) * self.gaussian(edge_attr).view(E, K, 1)).sum(dim=-2)
        gaussian = -0.5 * (edge_attr.view(E, 1, 1, 1, D) - self.mu.view(1, F, M, K, D)).pow(2)
        gaussian = gaussian / (EPS + self.sigma.view(1, F, M, K, D).pow(2))
        gaussian = torch.exp(gaussian.sum(dim=-1))  # [E, F, M, K]
        gaussian = gaussian * self.g.view(1, F, M, K)
        gaussian = gaussian.sum(dim=-1)  # [E, F, M]
        return (x_j.view(E, F, 1) * gaussian).sum(dim=-2)  # [E, M]

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, {self.out_channels}, '
                f'dim={self.dim})')
