import os
from typing import List, Optional, Tuple, Union

import torch
from torch import Tensor
from torch.nn import Parameter

from ... import _native
from ..._functions import SplineConvFunction, linear
from ...edge_index import as_edge_index
from ...utils import spline_basis, spline_weighting
from ..dense.linear import Linear
from ..inits import uniform, zeros
from .gmm_conv import stock_flow
from .message_passing import MessagePassing, _n_dst

# PYGAMD_FUSE_SPLINE=0: SplineConv layers start with ``fuse = False`` (read at import).  The
# default is 1: the rule and the figures behind it are in profiles/spline_conv.md.
FUSE_SPLINE = os.environ.get('PYGAMD_FUSE_SPLINE', '1') not in ('', '0')


def _repeat(value, dim: int) -> list:
    """utils/repeat.py of the reference: a scalar ``dim`` times, a list cut or padded with its
    last entry to ``dim``"""
    if not isinstance(value, (list, tuple)):
        return [value] * dim
    value = list(value)
    return value[:dim] + [value[-1]] * (dim - len(value))


class SplineConv(MessagePassing):
    r"""The spline-based convolution (SplineCNN) with the constructor arguments, buffers
    (``kernel_size``, ``is_open_spline``), parameter names (``weight [K, F_in, F_out]``,
    ``lin.weight``, ``bias``), lazy ``-1`` channels and forward semantics of
    ``torch_geometric.nn.SplineConv`` (torch_geometric/nn/conv/spline_conv.py:21-168):

    .. math:: x_i' = \frac{1}{|N(i)|} \sum_{j \in N(i)} \sum_{s < S} B_s(e_{ij})\,
        x_j \Theta_{w_s(e_{ij})} + x_i \Theta_{root} + b

    with ``S = (degree + 1)^dim`` B-spline basis products per edge out of ``K = prod kernel_size``
    weight matrices.  ``x`` is a tensor or a ``(x_src, x_dst)`` pair.  The reference needs
    pyg-lib's ``spline_basis`` / ``spline_weighting`` and warns on host tensors; this layer brings
    both and does not warn.  Routes:

    * fused (float32 device tensors, ``fuse`` true, ``flow='source_to_target'``, ``aggr`` in add
      / sum / mean, ``_native.spline_supported(F_in, F_out, K, S)``): ``SplineConvFunction`` —
      one dense product ``H = x_src @ weight`` for all ``K`` bins, then ONE launch over the
      destinations that rebuilds a slot's ``S`` pairs in registers, gathers ``S`` rows of
      ``F_out`` floats and applies ``1 / deg``, ``lin(x_i)`` and the bias in its epilogue
      (csrc/spline.hip).  The backward bins the output gradient per source in LDS and takes two
      dense products; nothing of size ``[E, S]`` or wider exists;
    * the reference's gather -> ``message`` -> aggregate for everything else (``aggr='max'``, host
      tensors, other dtypes, shapes outside the envelope) — and whenever the message flow is
      observed or replaced.  ``message`` is ``spline_weighting(x_j, weight, *spline_basis(...))``
      from :mod:`pytorch_geometric_amd.utils`.

    ``fuse`` is a per-layer attribute initialised from the environment switch
    ``PYGAMD_FUSE_SPLINE`` (read at import, default ``1``)."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, dim: int,
                 kernel_size: Union[int, List[int]], is_open_spline: Union[bool, List[bool]] = True,
                 degree: int = 1, aggr: str = 'mean', root_weight: bool = True,
                 bias: bool = True, **kwargs):
        super().__init__(aggr=aggr, **kwargs)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.dim = dim
        self.degree = degree
        self.root_weight = root_weight
        kernel_size = torch.tensor(_repeat(kernel_size, dim), dtype=torch.long)
        self.register_buffer('kernel_size', kernel_size)
        self.register_buffer('is_open_spline',
                             torch.tensor(_repeat(is_open_spline, dim), dtype=torch.uint8))
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.K = kernel_size.prod().item()
        if in_channels[0] > 0:
            self.weight = Parameter(torch.empty(self.K, in_channels[0], out_channels))
        else:
            self.weight = torch.nn.parameter.UninitializedParameter()
        if root_weight and in_channels[1] > 0:
            self.lin = Linear(in_channels[1], out_channels, bias=False,
                              weight_initializer='uniform')
        else:
            self.register_module('lin', None)   # (lazy: made by the first forward)
        if in_channels[0] <= 0 or (root_weight and in_channels[1] <= 0):
            self._hook = self.register_forward_pre_hook(self.initialize_parameters)
        if bias:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.fuse = FUSE_SPLINE
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        if not isinstance(self.weight, torch.nn.parameter.UninitializedParameter):
            uniform(self.weight.size(0) * self.weight.size(1), self.weight)
        if self.lin is not None:
            self.lin.reset_parameters()
        zeros(self.bias)

    @torch.no_grad()
    def initialize_parameters(self, module, input):
        x = input[0]
        x_src, x_dst = (x, x) if isinstance(x, Tensor) else (x[0], x[1])
        if isinstance(self.weight, torch.nn.parameter.UninitializedParameter):
            self.weight.materialize((self.K, x_src.size(-1), self.out_channels),
                                    device=x_src.device)
            uniform(self.weight.size(0) * self.weight.size(1), self.weight)
        if self.root_weight and self.lin is None and x_dst is not None:
            self.lin = Linear(x_dst.size(-1), self.out_channels, bias=False,
                              weight_initializer='uniform').to(x_dst.device)
        module._hook.remove()
        delattr(module, '_hook')

    def _fusable(self, x_src: Tensor, x_dst, edge_attr) -> bool:
        if not stock_flow(self, SplineConv):
            return False
        tensors = [x_src, edge_attr, self.weight] + ([] if x_dst is None else [x_dst])
        if not (self.fuse and self.flow == 'source_to_target'
                and self.aggr in ('add', 'sum', 'mean') and not torch.is_autocast_enabled()
                and all(isinstance(t, Tensor) and t.is_cuda and t.dim() == 2 + (t is self.weight)
                        and t.dtype == torch.float32 for t in tensors)
                and x_src.size(1) == self.weight.size(1) and edge_attr.size(1) == self.dim
                and self.degree in (1, 2, 3)):
            return False
        return _native.spline_supported(self.weight.size(1), self.out_channels, self.K,
                                        (self.degree + 1) ** self.dim)

    def forward(self, x: Union[Tensor, Tuple[Tensor, Optional[Tensor]]], edge_index,
                edge_attr: Optional[Tensor] = None, size=None) -> Tensor:
        if isinstance(x, Tensor):
            x = (x, x)
        rooted = x[1] is not None and self.root_weight
        if self._fusable(x[0], x[1], edge_attr):
            n_dst = _n_dst(self, x[0], x[1], edge_index, size)
            graph = as_edge_index(edge_index, x[0].size(0), n_dst)
            root = linear(x[1], self.lin.weight)[:n_dst] if rooted else None
            return SplineConvFunction.apply(
                x[0], edge_attr, self.weight, root, self.bias, self.kernel_size,
                self.is_open_spline, self.degree, graph, n_dst, self.aggr == 'mean')
        out = self.propagate(edge_index, x=x, edge_attr=edge_attr, size=size)
        if rooted:
            out = out + self.lin(x[1])[:out.size(0)]
        if self.bias is not None:
            out = out + self.bias
        return out

    def message(self, x_j: Tensor, edge_attr: Tensor) -> Tensor:
        basis, index = spline_basis(edge_attr, self.kernel_size, self.is_open_spline, self.degree)
        return spline_weighting(x_j, self.weight, basis.to(x_j.dtype), index)

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, {self.out_channels}, '
                f'dim={self.dim})')
