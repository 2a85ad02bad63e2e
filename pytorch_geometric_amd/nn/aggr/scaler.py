from typing import Any, Dict, List, Optional, Union

import torch
from torch import Tensor

from .base import Aggregation
from .fused import MultiAggregation, _resolve

SCALERS = ('identity', 'amplification', 'attenuation', 'linear', 'inverse_linear')


def degree_scale(out: Tensor, deg: Tensor, scalers, avg_deg_lin: Tensor,
                 avg_deg_log: Tensor) -> Tensor:
    """``out [N, F]`` under every scaler in turn, concatenated on the last dimension, for the
    degrees ``deg [N, 1]`` in the dtype of ``out`` (torch_geometric/nn/aggr/scaler.py:90-109; the
    two dividing scalers clamp the degree at one)."""
    outs = []
    for scaler in scalers:
        if scaler == 'identity':
            scaled = out
        elif scaler == 'amplification':
            scaled = out * (torch.log(deg + 1) / avg_deg_log)
        elif scaler == 'attenuation':
            scaled = out * (avg_deg_log / torch.log(deg.clamp(min=1) + 1))
        elif scaler == 'linear':
            scaled = out * (deg / avg_deg_lin)
        elif scaler == 'inverse_linear':
            scaled = out * (avg_deg_lin / deg.clamp(min=1))
        else:
            raise ValueError(f"Unknown scaler '{scaler}'")
        outs.append(scaled)
    return torch.cat(outs, dim=-1) if len(outs) > 1 else outs[0]


class DegreeScalerAggregation(Aggregation):
    r"""One or more aggregations whose result is transformed by one or more degree scalers, as in
    "Principal Neighbourhood Aggregation for Graph Nets", with the constructor arguments, the
    buffers (parameters with ``train_norm``) ``avg_deg_lin`` / ``avg_deg_log`` and the errors of
    ``torch_geometric.nn.aggr.DegreeScalerAggregation`` (torch_geometric/nn/aggr/scaler.py:13-109).
    ``deg`` is the histogram of in-degrees of the training set.  A list of aggregations goes
    through this package's :class:`MultiAggregation` (one multi-reduce kernel for the fusable
    ones); inputs are two-dimensional, like the package's other aggregations, and the degrees are
    counted from ``index``."""

    def __init__(self, aggr: Union[str, List[str], Aggregation], scaler: Union[str, List[str]],
                 deg: Tensor, train_norm: bool = False,
                 aggr_kwargs: Optional[List[Dict[str, Any]]] = None):
        super().__init__()
        if isinstance(aggr, (str, Aggregation)):
            self.aggr = _resolve(aggr) if not aggr_kwargs else _resolve_with(aggr, aggr_kwargs)
        elif isinstance(aggr, (tuple, list)):
            if aggr_kwargs:
                raise ValueError("'aggr_kwargs' is not supported for a list of aggregations")
            self.aggr = MultiAggregation(list(aggr))
        else:
            raise ValueError(f"Only strings, list, tuples and instances of"
                             f"`torch_geometric.nn.aggr.Aggregation` are "
                             f"valid aggregation schemes (got '{type(aggr)}')")
        self.scaler = [scaler] if isinstance(aggr, str) else scaler

        deg = deg.to(torch.float)
        N = int(deg.sum())
        bin_degree = torch.arange(deg.numel(), device=deg.device)
        self.init_avg_deg_lin = float((bin_degree * deg).sum()) / N
        self.init_avg_deg_log = float(((bin_degree + 1).log() * deg).sum()) / N
        if train_norm:
            self.avg_deg_lin = torch.nn.Parameter(torch.empty(1))
            self.avg_deg_log = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_buffer('avg_deg_lin', torch.empty(1))
            self.register_buffer('avg_deg_log', torch.empty(1))
        self.reset_parameters()

    def reset_parameters(self):
        self.avg_deg_lin.data.fill_(self.init_avg_deg_lin)
        self.avg_deg_log.data.fill_(self.init_avg_deg_log)

    def scale(self, out: Tensor, deg: Tensor) -> Tensor:
        """the scalers applied to an aggregate ``out [N, F]`` of nodes with in-degrees ``deg [N]``"""
        return degree_scale(out, deg.to(out.dtype).view(-1, 1), self.scaler, self.avg_deg_lin,
                            self.avg_deg_log)

    def forward(self, x: Tensor, index: Optional[Tensor] = None, ptr: Optional[Tensor] = None,
                dim_size: Optional[int] = None, dim: int = -2) -> Tensor:
        if index is None:
            raise NotImplementedError("Aggregation requires 'index' to be specified")
        if x.dim() != 2:
            raise ValueError(f"Aggregation requires two-dimensional inputs (got '{x.dim()}')")
        out = self.aggr(x, index, ptr, dim_size, dim)
        deg = torch.bincount(index.long(), minlength=out.size(0))
        return self.scale(out, deg)


def _resolve_with(aggr, aggr_kwargs) -> Aggregation:
    from .basic import aggregation_resolver
    if isinstance(aggr, str) and aggr.lower() in ('var', 'std'):
        from .fused import StdAggregation, VarAggregation
        return (VarAggregation if aggr.lower() == 'var' else StdAggregation)(**aggr_kwargs)
    return aggregation_resolver(aggr, **aggr_kwargs)
