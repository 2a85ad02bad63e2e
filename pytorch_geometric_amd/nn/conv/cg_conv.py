import os
from typing import Optional, Tuple, Union

import torch
import torch.nn.functional as F_
from torch import Tensor
from torch.nn import BatchNorm1d, Linear

from ... import _native
from ..._functions import CGAggregateFunction, linear
from ...edge_index import as_edge_index
from .gmm_conv import device_floats, stock_flow
from .message_passing import _LOW, MessagePassing, _n_dst

# PYGAMD_FUSE_CG: which edge modes of CGConv start with ``fuse = True`` (read at import): ``1``
# all, ``0`` none, or a comma list of ``none`` (dim = 0), ``linear`` (raw edge features, the
# edge matrices in registers) and ``wide`` (the dense edge terms).  The default is the set of
# modes whose fused training step was measured faster than the generic one: all three, by 1.62
# (none), 1.93 (linear) and 1.81 (wide) at the shapes of profiles/cg_conv.md.
CG_MODES = ('none', 'linear', 'wide')
_DEFAULT_FUSE_CG = 'none,linear,wide'


def _parse_modes(value: str) -> Tuple[str, ...]:
    value = value.strip().lower()
    if value in ('', '0'):
        return ()
    if value == '1':
        return CG_MODES
    return tuple(m for m in CG_MODES if m in [v.strip() for v in value.split(',')])


FUSE_CG = _parse_modes(os.environ.get('PYGAMD_FUSE_CG', _DEFAULT_FUSE_CG))


class CGConv(MessagePassing):
    r"""The crystal graph convolution (CGCNN) with the constructor arguments, state-dict keys
    (``lin_f.*``, ``lin_s.*``, ``bn.*``), ``__repr__`` and forward semantics of
    ``torch_geometric.nn.CGConv`` (torch_geometric/nn/conv/cg_conv.py:12-101):

    .. math:: x_i' = x_i + \mathrm{aggr}_{j \in N(i)} \sigma(z_{ij} W_f + b_f) \odot
        \mathrm{softplus}(z_{ij} W_s + b_s), \quad z_{ij} = [x_i, x_j, e_{ij}]

    ``channels`` is an int or a ``(src, dst)`` pair, ``x`` a tensor or a ``(x_src, x_dst)`` pair;
    the columns of both weights are ``[x_i (dst) | x_j (src) | edge]``.  Routes:

    * fused (device tensors, float32 after widening, ``fuse`` true, ``flow='source_to_target'``,
      ``aggr`` in add / sum / mean, ``channels[1] <= 512`` and ``edge_attr`` present exactly when
      ``dim > 0``): both ``Linear`` are split into their destination, source and edge columns.
      The node columns become node-level products — with one ``x`` in both roles ONE ``[N, 4F]``
      projection with stacked weights, whose gradient is ONE plane — and ``propagate`` is one
      kernel forward and two backward (``CGAggregateFunction``, csrc/cg.hip) that gather one
      ``2F`` row per edge and recompute the sigmoid and the softplus in the backward.  The edge
      columns: where ``_native.cg_supported(F, dim)`` (``dim <= 32`` and ``F * dim <= 2048``) the
      kernels rebuild the edge terms per slot from the RAW features with both ``[F, dim]``
      matrices in registers and nothing of size ``E x F`` exists.  Past that envelope (CGCNN's
      own 41 Gaussian-expanded distances at ``F = 64``) the layer forms ONE dense product
      ``edge_attr @ [Wf_e ; Ws_e]^T`` of size ``E x 2F``, and the backward its gradient: two
      ``E x 2F`` planes, against the reference's ``E x (2F + dim)`` cat, four pre- and
      post-activations and product, none of which is formed.  Without ``batch_norm`` the residual
      rides in the kernel's epilogue; with it ``BatchNorm1d`` runs on the kernel's output (in
      float32 too: a layer moved to half has its batch norm's parameters and statistics widened
      for the call and the running statistics written back) and the residual is added after;
    * the reference's gather -> ``message`` -> aggregate for everything else (host tensors,
      float64 tensors, ``fuse = False``, ``target_to_source``, ``max`` and other aggregations,
      ``channels[1] > 512``) — and whenever the message flow is observed or replaced: a propagate, message or
      aggregate hook, explain mode, or a subclass with its own ``message``, ``aggregate``,
      ``update`` or ``propagate``.

    ``edge_attr`` without ``dim`` and ``dim`` without ``edge_attr`` are refused on both routes.
    Half and bfloat16 device inputs are widened to float32 and the result handed back in their
    dtype outside autocast.  ``fuse`` is a per-layer attribute initialised from the environment
    switch ``PYGAMD_FUSE_CG`` (read at import): true if the layer's edge mode (``edge_mode``:
    ``'none'``, ``'linear'`` or ``'wide'``) is one the switch names."""

    def __init__(self, channels: Union[int, Tuple[int, int]], dim: int = 0, aggr: str = 'add',
                 batch_norm: bool = False, bias: bool = True, **kwargs):
        super().__init__(aggr=aggr, **kwargs)
        self.channels = channels
        self.dim = dim
        self.batch_norm = batch_norm
        if isinstance(channels, int):
            channels = (channels, channels)
        self.lin_f = Linear(sum(channels) + dim, channels[1], bias=bias)
        self.lin_s = Linear(sum(channels) + dim, channels[1], bias=bias)
        self.bn = BatchNorm1d(channels[1]) if batch_norm else None
        self._widths = (int(channels[0]), int(channels[1]))
        self.fuse = self.edge_mode in FUSE_CG
        self.reset_parameters()

    @property
    def edge_mode(self) -> str:
        """how the fused route takes the edge columns: ``'none'``, ``'linear'`` or ``'wide'``"""
        if self.dim == 0:
            return 'none'
        return 'linear' if _native_envelope(self._widths[1], self.dim) else 'wide'

    def reset_parameters(self):
        super().reset_parameters()
        self.lin_f.reset_parameters()
        self.lin_s.reset_parameters()
        if self.bn is not None:
            self.bn.reset_parameters()

    def _fusable(self, x_src, x_dst, edge_attr) -> bool:
        if not stock_flow(self, CGConv):
            return False
        if not (self.fuse and self.flow == 'source_to_target'
                and self.aggr in ('add', 'sum', 'mean') and device_floats(x_src, x_dst)
                and x_src.size(1) == self._widths[0] and x_dst.size(1) == self._widths[1]
                and self._widths[1] <= 512):
            return False
        return self.dim == 0 or (device_floats(edge_attr) and edge_attr.size(1) == self.dim)

    def forward(self, x: Union[Tensor, Tuple[Tensor, Tensor]], edge_index,
                edge_attr: Optional[Tensor] = None) -> Tensor:
        if isinstance(x, Tensor):
            x = (x, x)
        if (edge_attr is not None) != (self.dim > 0):
            raise ValueError(f"'edge_attr' is given exactly when dim > 0 (dim = {self.dim}, "
                             f"edge_attr {'given' if edge_attr is not None else 'missing'})")
        if self._fusable(x[0], x[1], edge_attr):
            return self._forward_fused(x[0], x[1], edge_index, edge_attr)
        out = self.propagate(edge_index, x=x, edge_attr=edge_attr)
        out = out if self.bn is None else self.bn(out)
        return out + x[1]

    def _forward_fused(self, x_src: Tensor, x_dst: Tensor, edge_index,
                       edge_attr: Optional[Tensor]) -> Tensor:
        Fs, F = self._widths
        low = x_src.dtype if x_src.dtype in _LOW else None
        xs = x_src.float()
        xd = xs if x_dst is x_src else x_dst.float()
        n_dst = _n_dst(self, x_src, x_dst, edge_index, None)
        graph = as_edge_index(edge_index, xs.size(0), n_dst)
        with torch.autocast('cuda', enabled=False):
            wf, ws = self.lin_f.weight.float(), self.lin_s.weight.float()
            # Linear(F + Fs + dim, F) on cat([x_i, x_j, a]) = (dst columns) x_i + (src columns) x_j
            # + (edge columns) a, for both transforms at once: [Wf ; Ws] is [2F, F + Fs + dim]
            w = torch.cat([wf, ws])
            bias = None
            if self.lin_f.bias is not None:
                bias = torch.cat([self.lin_f.bias.float(), self.lin_s.bias.float()])
            if xd is xs:
                # ONE [N, 4F] projection [P | Q] (the kernels read its halves in place)
                w4 = torch.cat([w[:, :F], w[:, F:F + Fs]])
                bias4 = None if bias is None else torch.cat([bias, bias.new_zeros(2 * F)])
                p = linear(xs, w4, bias4)
                q = None
            else:
                p = linear(xd, w[:, :F].contiguous(), bias)
                q = linear(xs, w[:, F:F + Fs].contiguous(), None)
            ea = w_f = w_s = terms = None
            if self.dim > 0:
                if _native.cg_supported(F, self.dim):
                    ea = edge_attr.float()
                    w_f, w_s = wf[:, F + Fs:].contiguous(), ws[:, F + Fs:].contiguous()
                else:  # the one E x 2F plane of this route (and its gradient in the backward)
                    terms = linear(edge_attr.float(), w[:, F + Fs:].contiguous(), None)
            residual = None if self.bn is not None else xd[:n_dst]
            out = CGAggregateFunction.apply(p, q, ea, w_f, w_s, terms, residual, graph, n_dst,
                                            self.aggr == 'mean')
            if self.bn is not None:
                out = self._bn_float32(out) + xd[:n_dst]
        if low is not None and not torch.is_autocast_enabled():
            out = out.to(low)
        return out

    def _bn_float32(self, out: Tensor) -> Tensor:
        """``self.bn`` on the float32 ``out``; parameters and statistics held in half or bfloat16
        are widened for the call, as the weights are, and the updated running statistics copied
        back in their dtype (``num_batches_tracked`` is the module's own tensor)"""
        bn = self.bn
        state = dict(bn.state_dict(keep_vars=True))
        low = [k for k, v in state.items() if v.dtype in _LOW]
        if not low:
            return bn(out)
        state.update({k: state[k].float() for k in low})
        out = torch.func.functional_call(bn, state, (out, ))
        with torch.no_grad():
            for k in low:
                if k.startswith('running_'):
                    getattr(bn, k).copy_(state[k])
        return out

    def message(self, x_i: Tensor, x_j: Tensor, edge_attr: Optional[Tensor]) -> Tensor:
        if edge_attr is None:
            z = torch.cat([x_i, x_j], dim=-1)
        else:
            z = torch.cat([x_i, x_j, edge_attr], dim=-1)
        return self.lin_f(z).sigmoid() * F_.softplus(self.lin_s(z))

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}({self.channels}, dim={self.dim})'


def _native_envelope(F: int, De: int) -> bool:
    """``_native.cg_supported`` without loading the library (a layer is constructed on machines
    that have none): the envelope of include/pyg_amd.h"""
    return F <= 512 and 1 <= De <= 32 and F * De <= 2048
