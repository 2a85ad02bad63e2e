import os
from typing import Any, Callable, Dict, List, Optional, Union

import torch
from torch import Tensor
from torch.nn import ModuleList, Sequential

from ... import _native
from ..._functions import PnaAggregateFunction, linear
from ...edge_index import EdgeIndex, as_edge_index
from ..aggr.scaler import DegreeScalerAggregation, degree_scale
from ..dense.linear import Linear
from ..inits import reset
from .message_passing import _FLOATS, _LOW, MessagePassing

# PYGAMD_FUSE_PNA=0: PNAConv layers start with ``fuse = False`` (read at import)
FUSE_PNA = os.environ.get('PYGAMD_FUSE_PNA', '1') not in ('', '0')


class PNAConv(MessagePassing):
    r"""The Principal Neighbourhood Aggregation operator with the constructor arguments,
    state-dict keys (``aggr_module.avg_deg_lin``, ``aggr_module.avg_deg_log``, ``edge_encoder.*``,
    ``pre_nns.{t}.{k}.*``, ``post_nns.{t}.{k}.*``, ``lin.*``), ``__repr__``,
    ``get_degree_histogram`` and forward semantics of ``torch_geometric.nn.PNAConv``
    (torch_geometric/nn/conv/pna_conv.py:18-213): per tower ``t`` the message ``pre_nns[t]([x_i,
    x_j, edge_encoder(e_ji)])``, aggregated by every aggregator, scaled by every degree scaler
    (:class:`DegreeScalerAggregation`), concatenated with ``x_i``, sent through ``post_nns[t]``,
    and the towers through ``lin``.  Routes:

    * fused (device tensors, float32 after widening, ``fuse`` true, ``pre_layers == 1``,
      ``flow='source_to_target'``, aggregators out of mean / min / max / std and
      ``_native.pna_supported(towers * F_in, edge_dim or 0)``): the message is linear, so it splits
      into ``P_dst[i] + P_src[j] + Wc e_ji``.  ``P_src | P_dst`` is ONE dense transform of ``x``
      (``divide_input``: with a block-diagonal weight), ``Wc = C_t W_enc`` is formed in torch, and
      ONE kernel per direction (``PnaAggregateFunction``, csrc/pna.hip) yields every statistic
      from one gathered row per edge: nothing of size ``E x towers * F_in`` is formed or saved.
      Degrees come from the handle's row pointer;
    * generic gather -> ``message`` -> ``aggregate`` for everything else, host tensors included,
      with the towers flattened to ``[E, towers * F_in]``.

    Half and bfloat16 device inputs are widened to float32 and the result handed back in their
    dtype outside autocast.  ``fuse`` is a per-layer attribute initialised from the environment
    switch ``PYGAMD_FUSE_PNA`` (read at import, default ``1``)."""

    def __init__(self, in_channels: int, out_channels: int, aggregators: List[str],
                 scalers: List[str], deg: Tensor, edge_dim: Optional[int] = None,
                 towers: int = 1, pre_layers: int = 1, post_layers: int = 1,
                 divide_input: bool = False, act: Union[str, Callable, None] = 'relu',
                 act_kwargs: Optional[Dict[str, Any]] = None, train_norm: bool = False,
                 **kwargs):
        from ..models.basic_gnn import activation_resolver
        aggr = DegreeScalerAggregation(aggregators, scalers, deg, train_norm)
        super().__init__(aggr=aggr, node_dim=0, **kwargs)
        if divide_input:
            assert in_channels % towers == 0
        assert out_channels % towers == 0
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.aggregators = [a.lower() if isinstance(a, str) else a for a in aggregators]
        self.edge_dim = edge_dim
        self.towers = towers
        self.pre_layers = pre_layers
        self.divide_input = divide_input
        self.F_in = in_channels // towers if divide_input else in_channels
        self.F_out = self.out_channels // towers

        if self.edge_dim is not None:
            self.edge_encoder = Linear(edge_dim, self.F_in)
        self.pre_nns = ModuleList()
        self.post_nns = ModuleList()
        for _ in range(towers):
            modules = [Linear((3 if edge_dim else 2) * self.F_in, self.F_in)]
            for _ in range(pre_layers - 1):
                modules += [activation_resolver(act, **(act_kwargs or {}))]
                modules += [Linear(self.F_in, self.F_in)]
            self.pre_nns.append(Sequential(*modules))
            width = (len(aggregators) * len(scalers) + 1) * self.F_in
            modules = [Linear(width, self.F_out)]
            for _ in range(post_layers - 1):
                modules += [activation_resolver(act, **(act_kwargs or {}))]
                modules += [Linear(self.F_out, self.F_out)]
            self.post_nns.append(Sequential(*modules))
        self.lin = Linear(out_channels, out_channels)
        self.fuse = FUSE_PNA
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        if self.edge_dim is not None:
            self.edge_encoder.reset_parameters()
        for nn in self.pre_nns:
            reset(nn)
        for nn in self.post_nns:
            reset(nn)
        self.lin.reset_parameters()

    # -- the fused route --------------------------------------------------------------------------
    def _fusable(self, x: Tensor, edge_attr: Optional[Tensor]) -> bool:
        if not (self.fuse and x.is_cuda and x.dim() == 2 and x.dtype in _FLOATS
                and self.pre_layers == 1 and self.flow == 'source_to_target'):
            return False
        if not all(isinstance(a, str) and a in _native.PNA_STATS for a in self.aggregators) \
                or len(set(self.aggregators)) != len(self.aggregators):
            return False
        if bool(self.edge_dim) != isinstance(edge_attr, Tensor):
            return False
        if edge_attr is not None and not (edge_attr.is_cuda and edge_attr.dim() == 2
                                          and edge_attr.dtype in _FLOATS
                                          and edge_attr.size(1) == self.edge_dim):
            return False
        return _native.pna_supported(self.towers * self.F_in, self.edge_dim or 0)

    def _split_weights(self):
        """``(packed [2 W, in_channels], bias [2 W], Wc [W, edge_dim] | None)``: the rows of
        ``P_src`` then those of ``P_dst``, every constant folded into the bias of ``P_dst``."""
        Fi, T = self.F_in, self.towers
        first = [nn[0] for nn in self.pre_nns]
        A = [m.weight[:, :Fi].float() for m in first]
        B = [m.weight[:, Fi:2 * Fi].float() for m in first]
        bias = [m.bias.float() for m in first]
        Wc = None
        if self.edge_dim:
            C = [m.weight[:, 2 * Fi:].float() for m in first]
            w_enc, b_enc = self.edge_encoder.weight.float(), self.edge_encoder.bias.float()
            Wc = torch.cat([c @ w_enc for c in C], dim=0)
            bias = [b + c @ b_enc for b, c in zip(bias, C)]
        if self.divide_input:
            packed = torch.cat([torch.block_diag(*B), torch.block_diag(*A)], dim=0)
        else:
            packed = torch.cat(B + A, dim=0)
        bias = torch.cat([packed.new_zeros(T * Fi)] + bias)
        return packed, bias, Wc

    def _fused(self, x: Tensor, edge_index, edge_attr: Optional[Tensor]) -> Tensor:
        T, Fi = self.towers, self.F_in
        W = T * Fi
        n_dst = edge_index.num_dst_nodes if isinstance(edge_index, EdgeIndex) else x.size(0)
        graph = as_edge_index(edge_index, x.size(0), n_dst)
        packed, bias, Wc = self._split_weights()
        P = linear(x, packed, bias)
        ea = None if edge_attr is None else edge_attr.float()
        stats = PnaAggregateFunction.apply(P[:, :W], P[:, W:], ea, Wc, graph, n_dst,
                                           tuple(self.aggregators))
        ptr = graph.by_dst().ptr
        deg = (ptr[1:] - ptr[:-1]).to(torch.float32).view(-1, 1, 1)
        # [N, W] per statistic -> [N, T, A * F_in] -> the scalers on the last dimension
        out = torch.cat([s.view(n_dst, T, Fi) for s in stats], dim=-1)
        mod = self.aggr_module
        return degree_scale(out, deg, mod.scaler, mod.avg_deg_lin, mod.avg_deg_log)

    # -- the generic route -------------------------------------------------------------------------
    def _materialised(self, x: Tensor, edge_index, edge_attr: Optional[Tensor]) -> Tensor:
        """``[N, T, S * A * F_in]`` from per-edge messages through ``propagate``"""
        T, Fi = self.towers, self.F_in
        xt = x.view(-1, T, Fi) if self.divide_input else x.view(-1, 1, Fi).repeat(1, T, 1)
        out = self.propagate(edge_index, x=xt, edge_attr=edge_attr)
        # [N, S * A * W] with the towers inside every block -> towers outermost
        blocks = out.size(1) // (T * Fi)
        return out.view(-1, blocks, T, Fi).transpose(1, 2).reshape(-1, T, blocks * Fi)

    def forward(self, x: Tensor, edge_index, edge_attr: Optional[Tensor] = None) -> Tensor:
        low = x.dtype if x.is_cuda and x.dtype in _LOW else None
        if self._fusable(x, edge_attr):
            x = x.float()
            out = self._fused(x, edge_index, edge_attr)
        else:
            out = self._materialised(x, edge_index, edge_attr)
        T, Fi = self.towers, self.F_in
        xt = x.view(-1, T, Fi) if self.divide_input else x.view(-1, 1, Fi).expand(-1, T, -1)
        out = torch.cat([xt[:out.size(0)].to(out.dtype), out], dim=-1)
        if low is not None and out.dtype != low and not torch.is_autocast_enabled():
            out = out.to(low)
        outs = [nn(out[:, t]) for t, nn in enumerate(self.post_nns)]
        return self.lin(torch.cat(outs, dim=1))

    def message(self, x_i: Tensor, x_j: Tensor, edge_attr: Optional[Tensor]) -> Tensor:
        if edge_attr is not None:
            e = self.edge_encoder(edge_attr).view(-1, 1, self.F_in).repeat(1, self.towers, 1)
            h = torch.cat([x_i, x_j, e], dim=-1)
        else:
            h = torch.cat([x_i, x_j], dim=-1)
        hs = [nn(h[:, t]) for t, nn in enumerate(self.pre_nns)]
        return torch.cat(hs, dim=1)        # the towers flattened: [E, T * F_in]

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, {self.out_channels}, '
                f'towers={self.towers}, edge_dim={self.edge_dim})')

    @staticmethod
    def get_degree_histogram(loader) -> Tensor:
        r"""The in-degree histogram over every graph of ``loader`` (objects with ``edge_index`` and
        ``num_nodes``), for the ``deg`` argument (pna_conv.py:195-213)."""
        hist = torch.zeros(1, dtype=torch.long)
        for data in loader:
            deg = torch.bincount(data.edge_index[1].long(), minlength=data.num_nodes)
            count = torch.bincount(deg, minlength=hist.numel())
            hist = hist.to(count.device)
            if count.numel() > hist.numel():
                count[:hist.size(0)] += hist
                hist = count
            else:
                hist += count
        return hist

