"""What the layers made of linear propagation steps share (APPNP, SGConv, SSGConv, TAGConv, LGConv,
GCN2Conv): the normalisation of their edge list, the choice between their two routes and the step
itself.

* fused — float32 device tensors, ``aggr`` given as ``'add'`` / ``'sum'``, the stock ``message`` /
  ``aggregate`` / ``update``, nobody hooked into the message flow, edge weights that take no
  gradient, ``fuse`` true: every step is ONE launch of csrc/hop.hip whose row epilogue does the
  layer's combination (``HopFunction`` / ``HopsFunction``);
* generic — everything else: the reference's loop over ``propagate`` and torch arithmetic.

``fuse`` is a per-layer attribute initialised from ``PYGAMD_FUSE_HOPS`` (read at import) or, when
that is unset, from the layer class's measured default."""
import os
from typing import Optional

import torch
from torch import Tensor

from ... import _native
from ..._functions import HopFunction, HopsFunction, spmm_node
from ...edge_index import EdgeIndex, as_edge_index
from ...utils import add_remaining_self_loops
from .gcn_conv import gcn_norm, linear_message_flow
from .message_passing import MessagePassing

# PYGAMD_FUSE_HOPS (read at import): 0 / 1 start every layer of this module with ``fuse`` off / on;
# unset, a layer starts with its class's ``FUSE_DEFAULT`` — on where the fused step was at least as
# fast as the loop at every shape measured (profiles/propagate_hops.md)
_SWITCH = os.environ.get('PYGAMD_FUSE_HOPS')
FUSE_HOPS = None if _SWITCH is None else _SWITCH not in ('', '0')


def _gcn_norm_any(edge_index: Tensor, edge_weight: Optional[Tensor], n: int,
                  add_self_loops: bool, flow: str, dtype):
    """:func:`gcn_norm` (``improved=False``) where the edge list lives: on the device its degree
    sum is the package's scatter kernel, for host tensors the same steps run in plain torch."""
    if edge_index.is_cuda:
        return gcn_norm(edge_index, edge_weight, n, False, add_self_loops, flow, dtype)
    if flow not in ('source_to_target', 'target_to_source'):
        raise ValueError(f"invalid flow '{flow}'")
    if add_self_loops:
        edge_index, edge_weight = add_remaining_self_loops(edge_index, edge_weight, 1.0, n)
    if edge_weight is None:
        edge_weight = torch.ones(edge_index.size(1), dtype=dtype or torch.float32)
    receiver = edge_index[1] if flow == 'source_to_target' else edge_index[0]
    deg = torch.zeros(n, dtype=edge_weight.dtype).scatter_add(0, receiver.long(), edge_weight)
    inv_sqrt = deg.pow(-0.5)
    inv_sqrt = torch.where(torch.isinf(inv_sqrt), torch.zeros_like(inv_sqrt), inv_sqrt)
    return edge_index, inv_sqrt[edge_index[0]] * edge_weight * inv_sqrt[edge_index[1]]


def _gcn_norm_sorted(edge_index: Tensor, edge_weight: Optional[Tensor], n: int,
                     add_self_loops: bool, flow: str):
    """:func:`gcn_norm` (``improved=False``) for the fused route, whose first step sorts the
    self-looped edge list anyway: the degree is the segment sum of the weights over that sorted
    handle — in slot order, no atomics, so the normalised weights are bitwise repeatable — and
    the handle is the one the steps walk (``as_edge_index`` keeps it with the tensor)."""
    if add_self_loops:
        edge_index, edge_weight = add_remaining_self_loops(edge_index, edge_weight, 1.0, n)
    if edge_weight is None:
        edge_weight = torch.ones(edge_index.size(1), dtype=torch.float32,
                                 device=edge_index.device)
    fwd = as_edge_index(edge_index, n, n, flip=flow == 'target_to_source').by_dst()
    deg = _native.multi_reduce_csr(fwd.ptr, fwd.perm, edge_weight.view(-1, 1), ('sum', ))['sum']
    inv_sqrt = deg.view(-1).pow(-0.5)
    inv_sqrt = torch.where(torch.isinf(inv_sqrt), torch.zeros_like(inv_sqrt), inv_sqrt)
    return edge_index, inv_sqrt[edge_index[0]] * edge_weight * inv_sqrt[edge_index[1]]


class HopLayer(MessagePassing):
    """Base of the layers whose body is ``x <- A x`` combined with earlier iterates."""

    FUSE_DEFAULT = True

    def __init__(self, **kwargs):
        kwargs.setdefault('aggr', 'add')
        super().__init__(**kwargs)
        self.fuse = type(self).FUSE_DEFAULT if FUSE_HOPS is None else FUSE_HOPS

    # -- normalisation ---------------------------------------------------------------------------
    def _gcn_norm(self, x: Tensor, edge_index, edge_weight: Optional[Tensor],
                  add_self_loops: bool, cache: Optional[str] = None):
        """``gcn_norm`` of the layer's edge list (``improved=False``, as all six layers call it);
        ``cache``: the attribute that keeps the result across calls when ``self.cached``.  A
        handle keeps its normalised form itself (``EdgeIndex.derived``)."""
        n = x.size(self.node_dim)
        if isinstance(edge_index, EdgeIndex):
            handle = edge_index
            if handle.sparse_size != (n, n):
                raise ValueError(f"'{type(self).__name__}' needs a square graph over the {n} "
                                 f"rows of 'x' (got sparse_size={handle.sparse_size})")

            def build():
                ei, w = gcn_norm(handle.edge_index, edge_weight, n, False, add_self_loops,
                                 self.flow, x.dtype)
                return EdgeIndex(ei, (n, n), validate=False), w

            if edge_weight is not None:  # values (and maybe a graph of gradients) differ per call
                return build()
            return handle.derived(('gcn_norm', False, add_self_loops, self.flow), build)
        if cache is not None and getattr(self, cache) is not None:
            return getattr(self, cache)
        if self.hop_route(x, edge_index, edge_weight) == 'fused':
            out = _gcn_norm_sorted(edge_index, edge_weight, n, add_self_loops, self.flow)
        else:
            out = _gcn_norm_any(edge_index, edge_weight, n, add_self_loops, self.flow, x.dtype)
        if cache is not None and self.cached:
            setattr(self, cache, out)
        return out

    # -- routes ----------------------------------------------------------------------------------
    def hop_route(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None) -> str:
        """``'fused'`` or ``'generic'``: the route a call with these arguments takes."""
        if not self.fuse or not isinstance(x, Tensor):
            return 'generic'
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.size(1) >= 1):
            return 'generic'
        if not (isinstance(self.aggr, str) and self.aggr in ('add', 'sum')):
            return 'generic'
        if not isinstance(edge_index, Tensor) or not edge_index.is_cuda:
            return 'generic'
        if isinstance(edge_index, EdgeIndex) and self.flow != 'source_to_target':
            return 'generic'
        if edge_weight is not None and (edge_weight.requires_grad or not edge_weight.is_cuda
                                        or edge_weight.dtype != torch.float32
                                        or edge_weight.dim() != 1):
            return 'generic'
        return 'fused' if linear_message_flow(self, HopLayer) else 'generic'

    def _graph(self, x: Tensor, edge_index) -> EdgeIndex:
        n = x.size(0)
        return as_edge_index(edge_index, n, n, flip=self.flow == 'target_to_source')

    def _step(self, graph: EdgeIndex, x: Tensor, w: Optional[Tensor], a: float = 1.0,
              y: Optional[Tensor] = None, b: float = 0.0, z: Optional[Tensor] = None,
              c: float = 0.0) -> Tensor:
        return HopFunction.apply(x, w, y, z, graph, a, b, c)

    def _steps(self, graph: EdgeIndex, x: Tensor, w: Optional[Tensor], K: int, a: float = 1.0,
               b: float = 0.0, tied: bool = False, d0: float = 0.0, d: float = 0.0,
               want_sum: bool = False):
        """``x_K`` (or ``(x_K, s)``) of ``K`` steps ``x_k = a A x_{k-1} + b x_0``"""
        if K == 0:
            return (x, x * d0) if want_sum else x
        return HopsFunction.apply(x, None, w, graph, K, a, b, d0, d, want_sum, tied)

    # -- the generic route's pieces ----------------------------------------------------------------
    def _can_fuse(self, kwargs) -> bool:
        x = kwargs.get('x')
        if isinstance(x, Tensor) and not x.is_cuda:
            return False  # host tensors: gather -> message -> aggregate in plain torch
        return super()._can_fuse(kwargs)

    def message(self, x_j: Tensor, edge_weight: Optional[Tensor]) -> Tensor:
        return x_j if edge_weight is None else edge_weight.view(-1, 1) * x_j

    def message_and_aggregate(self, graph: EdgeIndex, x: Tensor,
                              edge_weight: Optional[Tensor]) -> Tensor:
        return spmm_node(x, edge_weight, graph, {'add': 'sum'}.get(self.aggr, self.aggr), 'coo')
