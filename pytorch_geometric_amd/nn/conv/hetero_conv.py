import warnings
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from ..module_dict import ModuleDict

_ABSENT = object()


def group(xs: List[Tensor], aggr: Optional[str]) -> Optional[Tensor]:
    """The results of the edge types that share a destination type as one tensor
    (torch_geometric/nn/conv/hetero_conv.py:13-26): ``None`` stacks on ``dim=1``, a single result
    is returned as it is, ``'cat'`` concatenates the channels, anything else is that torch
    reduction over the stack."""
    if not xs:
        return None
    if aggr is None:
        return torch.stack(xs, dim=1)
    if len(xs) == 1:
        return xs[0]
    if aggr == 'cat':
        return torch.cat(xs, dim=-1)
    reduced = getattr(torch, aggr)(torch.stack(xs), dim=0)
    return reduced if isinstance(reduced, Tensor) else reduced[0]   # min / max: (values, indices)


def _route(values: dict, edge_type) -> Tuple[object, bool]:
    """What ``values`` (one positional or keyword dict of a layer call) holds for the conv of
    ``edge_type``, by the reference's rules (hetero_conv.py:125-154): the edge type's own entry
    (an edge-level argument), else for ``src == dst`` the node type's entry, else the
    ``(src, dst)`` pair when either is present.  Returns ``(value or _ABSENT, edge level?)``."""
    src, dst = edge_type[0], edge_type[-1]
    if edge_type in values:
        return values[edge_type], True
    if src == dst:
        return (values[src] if src in values else _ABSENT), False
    if src in values or dst in values:
        return (values.get(src), values.get(dst)), False
    return _ABSENT, False


class HeteroConv(torch.nn.Module):
    r"""One bipartite layer per edge type; the results that share a destination type are grouped
    by ``aggr`` (``sum``, ``mean``, ``min``, ``max``, ``cat`` or ``None``) — constructor,
    argument routing, output order and state-dict layout of ``torch_geometric.nn.HeteroConv``
    (torch_geometric/nn/conv/hetero_conv.py:29-172)::

        conv = HeteroConv({
            ('paper', 'cites', 'paper'): SAGEConv((64, 64), 64),
            ('author', 'writes', 'paper'): SAGEConv((64, 64), 64),
        }, aggr='sum')
        out_dict = conv(x_dict, edge_index_dict)

    When every edge type of a call holds a plain mean / sum :class:`SAGEConv` (no ``project``, no
    ``normalize``, no hooks) on float32 device features with plain ``[2, E]`` ``edge_index``
    tensors and ``aggr`` is ``sum`` or ``mean``, the layer does not loop: ALL neighbourhoods of
    all edge types are aggregated by one launch per source feature width over a cached stacked CSR
    (``_hetero.py``, csrc/hetero_conv.hip) and one GEMM per destination type applies every
    ``lin_l`` / ``lin_r`` at once.  The handle is shared by all layers that see the same
    ``edge_index`` tensors.  ``fuse = False`` on the layer opts out; any other call (other convs,
    other group modes, extra arguments, more than 64 edge types) runs the per-edge-type loop.  The
    two paths compute the same operator."""

    def __init__(self, convs: Dict[Tuple[str, str, str], torch.nn.Module],
                 aggr: Optional[str] = 'sum'):
        super().__init__()
        sources, destinations = set(), set()
        for edge_type, conv in convs.items():
            sources.add(edge_type[0])
            destinations.add(edge_type[-1])
            # (the reference's check_add_self_loops, utils/hetero.py:70-79, and its wording)
            if edge_type[0] != edge_type[-1] and getattr(conv, 'add_self_loops', False):
                raise ValueError(
                    f"'add_self_loops' attribute set to 'True' on module '{conv}' "
                    f"for use with edge type(s) '{[edge_type]}'. This will lead to "
                    f"incorrect message passing results.")
        never_updated = sources - destinations
        if never_updated:  # (the reference's wording, hetero_conv.py:75-81)
            warnings.warn(
                f"There exist node types ({never_updated}) "
                f"whose representations do not get updated during message "
                f"passing as they do not occur as destination type in any "
                f"edge type. This may lead to unexpected behavior.", stacklevel=2)
        self.convs = ModuleDict(convs)
        self.aggr = aggr
        self.fuse = True

    def reset_parameters(self):
        for conv in self.convs.values():
            conv.reset_parameters()

    def _fast_plan(self, args_dict, kwargs_dict):
        """The fast-path plan of this call (``_hetero.plan``) or ``None``: only the plain
        ``(x_dict, edge_index_dict)`` call is planned."""
        if not self.fuse or kwargs_dict or len(args_dict) != 2:
            return None
        x_dict, edge_index_dict = args_dict
        if not (isinstance(x_dict, dict) and isinstance(edge_index_dict, dict)):
            return None
        from ... import _hetero
        # the reference's routing rules give (x_src, x_dst) and the edge type's own edge_index
        # exactly when no edge type is a key of x_dict and no node type one of edge_index_dict
        convs = self.convs.items()
        if any(et in x_dict or et[0] in edge_index_dict or et[-1] in edge_index_dict
               for et, _ in convs):
            return None
        return _hetero.plan(convs, x_dict, edge_index_dict, self.aggr)

    def forward(self, *args_dict, **kwargs_dict) -> Dict[str, Tensor]:
        keywords = {}
        for name in kwargs_dict:
            if not name.endswith('_dict'):  # (the reference's wording, hetero_conv.py:139-142)
                raise ValueError(
                    f"Keyword arguments in '{self.__class__.__name__}' "
                    f"need to end with '_dict' (got '{name}')")
            keywords[name[:-len('_dict')]] = kwargs_dict[name]
        plan = self._fast_plan(args_dict, kwargs_dict)
        if plan is not None:
            from ... import _hetero
            return _hetero.run(self.convs.items(), plan, args_dict[0], args_dict[1], self.aggr)

        # the generic path: every conv in turn, on what the routing rules give it
        results: Dict[str, List[Tensor]] = {}
        for edge_type, conv in self.convs.items():
            positional = [_route(values, edge_type) for values in args_dict]
            named = {name: _route(values, edge_type) for name, values in keywords.items()}
            if not any(edge_level for _, edge_level in positional + list(named.values())):
                continue  # an edge type without an edge-level argument is skipped
            out = conv(*[v for v, _ in positional if v is not _ABSENT],
                       **{name: v for name, (v, _) in named.items() if v is not _ABSENT})
            results.setdefault(edge_type[-1], []).append(out)
        return {dst: group(outs, self.aggr) for dst, outs in results.items()}

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}(num_relations={len(self.convs)})'
