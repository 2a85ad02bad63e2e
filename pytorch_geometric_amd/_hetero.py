"""The fast path of :class:`~pytorch_geometric_amd.nn.HeteroConv` over ``SAGEConv``: the planner
(which edge types of a layer call may share one aggregation launch), the cached stacked graph
handle, and the autograd node round ``pygamd_hetero_spmm`` / ``pygamd_hetero_spmm_backward``
(csrc/hetero_conv.hip).

For destination type ``D`` with incoming edge types ``ET(D)`` the layer computes

    out[D] = (1/c) * ( [agg_et1 | agg_et2 | ... | x_D] @ [W_l[et1] | W_l[et2] | ... | sum_et W_r[et]]^T
                       + sum_et b_l[et] ),        c = 1 for 'sum', |ET(D)| for 'mean'

— the aggregation of EVERY edge type writes its column block of the concatenated operand in one
launch, and one GEMM per destination type does the rest; weight and bias gradients reach the convs'
own parameters through autograd's ``cat`` / ``sum``."""
import weakref
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native

MAX_TYPES = _native.MAX_HETERO_TYPES
FAST_GROUP_AGGRS = ('sum', 'mean')
_HOOKS = ('_propagate_forward_pre_hooks', '_propagate_forward_hooks',
          '_message_and_aggregate_forward_pre_hooks', '_message_and_aggregate_forward_hooks',
          '_message_forward_pre_hooks', '_message_forward_hooks',
          '_aggregate_forward_pre_hooks', '_aggregate_forward_hooks')


def conv_eligible(conv) -> bool:
    """A plain mean / sum ``SAGEConv`` of this package whose ``propagate`` nobody observes."""
    from .nn.conv._act_request import has_forward_hooks
    from .nn.conv.sage_conv import SAGEConv
    if type(conv) is not SAGEConv or not getattr(conv, 'fuse', True):
        return False
    if conv.aggr not in ('mean', 'sum', 'add') or conv.flow != 'source_to_target':
        return False
    if conv.project or conv.normalize:
        return False
    if getattr(conv, 'explain', False) or getattr(conv, 'decomposed_layers', 1) != 1:
        return False
    if any(getattr(conv, h, None) for h in _HOOKS) or has_forward_hooks(conv):
        return False
    return True


def _features_ok(x, require_device: bool) -> bool:
    """Float32 row blocks the kernels read in place: unit inner stride, rows that do not overlap
    (a transposed or expanded view takes the generic loop, which accepts it)."""
    if not (type(x) in (Tensor, torch.nn.Parameter) and x.dim() == 2
            and x.dtype == torch.float32 and (x.is_cuda or not require_device)):
        return False
    return (x.size(1) <= 1 or x.stride(1) == 1) and (x.size(0) <= 1 or x.stride(0) >= x.size(1))


def _edges_ok(ei, require_device: bool) -> bool:
    return (type(ei) is Tensor and ei.dim() == 2 and ei.size(0) == 2
            and ei.dtype in (torch.int32, torch.int64) and (ei.is_cuda or not require_device))


class Plan:
    """What one fast-path layer call does.  ``groups``: ``[(K, [edge types])]``, one aggregation
    launch each (edge types grouped by source feature width, in conv order); ``dst``:
    ``{D: (edge types in conv order, has a root term)}`` in order of first appearance."""

    def __init__(self, groups, dst):
        self.groups, self.dst = groups, dst

    @property
    def edge_types(self):
        return [et for _, ets in self.groups for et in ets]


def plan(convs, x_dict, edge_index_dict, group_aggr, fuse: bool = True,
         require_device: bool = True) -> Optional[Plan]:
    """The fast-path plan of ``HeteroConv(convs, group_aggr)(x_dict, edge_index_dict)``, or
    ``None`` when the call takes the generic per-edge-type loop: a group mode other than sum /
    mean, an edge type whose conv, features or ``edge_index`` do not qualify (a layer is planned as
    a whole: a mixed layer is generic), more than 64 edge types of one source width or more than
    64 node types.  ``convs``: ``[(edge_type, conv)]`` in the layer's order; edge types without an
    ``edge_index`` are skipped, as the layer skips them.  ``require_device=False`` plans CPU
    tensors too (host-side tests of the rules; there is no CPU kernel)."""
    if not fuse or group_aggr not in FAST_GROUP_AGGRS:
        return None
    if torch.is_autocast_enabled() or torch.jit.is_scripting() or torch.compiler.is_compiling():
        return None
    if require_device and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return None
    by_width: Dict[int, List[tuple]] = {}
    dst: Dict[str, Tuple[list, bool]] = {}
    device = idx_dtype = None
    for et, conv in convs:
        if et not in edge_index_dict:
            continue
        s, d = et[0], et[-1]
        x_src, x_dst, ei = x_dict.get(s), x_dict.get(d), edge_index_dict[et]
        if not (conv_eligible(conv) and _features_ok(x_src, require_device)
                and _features_ok(x_dst, require_device) and _edges_ok(ei, require_device)):
            return None
        if device is None:
            device, idx_dtype = ei.device, ei.dtype
        if not (x_src.device == x_dst.device == ei.device == device and ei.dtype == idx_dtype):
            return None
        lin_l, lin_r = conv.lin_l, getattr(conv, 'lin_r', None)
        if x_src.size(1) != lin_l.weight.size(1) or x_src.size(1) == 0:
            return None
        if lin_r is not None and x_dst.size(1) != lin_r.weight.size(1):
            return None
        params = [lin_l.weight, lin_l.bias] + ([] if lin_r is None else [lin_r.weight])
        if any(p is not None and (p.dtype != torch.float32 or p.device != device) for p in params):
            return None
        ets, root = dst.get(d, ([], False))
        if ets and ets[0][1].out_channels != conv.out_channels:
            return None
        ets.append((et, conv))
        dst[d] = (ets, root or lin_r is not None)
        by_width.setdefault(x_src.size(1), []).append(et)
    if not dst:
        return None
    if any(len(ets) > MAX_TYPES for ets in by_width.values()):
        return None
    node_types = {et[0] for ets in by_width.values() for et in ets}
    if len(node_types) > MAX_TYPES:
        return None
    return Plan(list(by_width.items()),
                {d: ([et for et, _ in ets], root) for d, (ets, root) in dst.items()})


# ---- the stacked graph handle ---------------------------------------------------------------------
class HeteroGraph:
    r"""Every edge type of one aggregation launch as ONE stacked CSR.

    * ``row_begin``  — host ``[n_et + 1]``: row ``row_begin[et] + i`` is the neighbourhood of
      destination ``i`` under edge type ``et`` (rows are dense: an empty neighbourhood is an empty
      row);
    * ``rowptr`` / ``col`` — the CSR: ``col`` holds the typed local source id; built with one
      stable ``index_sort`` of the key ``row_begin[et] + dst`` and one ``index2ptr``;
    * ``src_types`` / ``src_begin`` — the node types that are a source here, stacked;
    * ``rowptr_t`` / ``col_t`` — the transposed structure for the backward (rows = stacked source
      nodes, slots = stacked row ids), built by a second stable sort on first use.

    ``src`` and ``dst`` are range-checked once, here."""

    def __init__(self, edge_types, edge_indices, num_src, num_dst):
        self.edge_types = list(edge_types)
        dev, dt = edge_indices[0].device, edge_indices[0].dtype
        self.row_begin = [0]
        for n in num_dst:
            self.row_begin.append(self.row_begin[-1] + int(n))
        self.src_types, self.src_begin, type_off = [], [0], {}
        for et, n in zip(self.edge_types, num_src):
            if et[0] not in type_off:
                type_off[et[0]] = self.src_begin[-1]
                self.src_types.append(et[0])
                self.src_begin.append(self.src_begin[-1] + int(n))
        R, S = self.row_begin[-1], self.src_begin[-1]
        E = sum(int(ei.size(1)) for ei in edge_indices)
        if dt == torch.int32 and max(R, S, E) >= 2 ** 31 - 1:
            raise ValueError('int32 edge indices: the stacked graph does not fit')
        self.num_rows, self.num_src, self.num_edges = R, S, E
        live = [(k, ei) for k, ei in enumerate(edge_indices) if ei.size(1) > 0]
        if E == 0:
            self.rowptr = torch.zeros(R + 1, dtype=dt, device=dev)
            self.col = torch.zeros(0, dtype=dt, device=dev)
            self._skey = self._src_key = self.col
            self._t = (torch.zeros(S + 1, dtype=dt, device=dev), self.col)
            return
        # every edge with its edge type's bounds and offsets, without a loop over the edge types:
        # rows 0 / 1 of `per_edge` bound src / dst, rows 2 / 3 shift them into the stacked spaces
        ei_all = live[0][1] if len(live) == 1 else torch.cat([ei for _, ei in live], dim=1)
        table = torch.tensor([[int(num_src[k]) for k, _ in live],
                              [int(num_dst[k]) for k, _ in live],
                              [type_off[self.edge_types[k][0]] for k, _ in live],
                              [self.row_begin[k] for k, _ in live]], dtype=dt).to(dev)
        counts = torch.tensor([int(ei.size(1)) for _, ei in live]).to(dev)
        per_edge = table.repeat_interleave(counts, dim=1, output_size=E)
        if bool(((ei_all < 0) | (ei_all >= per_edge[:2])).any()):
            # (one host read per handle; handles are cached)
            for k, ei in live:
                for row, n, what in ((0, num_src[k], 'source'), (1, num_dst[k], 'destination')):
                    lo, hi = _native.index_minmax(ei[row])
                    if lo < 0 or hi >= n:
                        raise IndexError(
                            f"Found indices in 'edge_index' of edge type {self.edge_types[k]} "
                            f"outside the valid range [0, {int(n) - 1}] of its {what} node type "
                            f"(got interval [{lo}, {hi}])")
        keys = ei_all + per_edge[2:]   # [stacked source id; stacked row] of every edge
        self._skey, perm = _native.index_sort(keys[1], max_value=max(R, 1))
        self.rowptr = _native.index2ptr(self._skey, R)
        self.col = _native.permute_index(ei_all[0], perm)
        # the stacked source id of every slot, in slot order: the key of the transposed sort
        self._src_key = _native.permute_index(keys[0], perm)
        self._t = None

    def transposed(self):
        if self._t is None:
            skey2, perm2 = _native.index_sort(self._src_key, max_value=max(self.num_src, 1))
            self._t = (_native.index2ptr(skey2, self.num_src),
                       _native.permute_index(self._skey, perm2))
            self._src_key = None
        return self._t


_handles: list = []   # most recent first
_MAX_HANDLES = 8


def hetero_graph(edge_types, edge_indices, num_src, num_dst) -> HeteroGraph:
    """The handle of these edge types over these ``edge_index`` tensors, cached by tensor identity
    + in-place version (the pattern of ``rgcn_conv._relational_handle``) and shared by every layer
    and by forward and backward: a 3-layer model sorts twice per batch, not six times."""
    sig = (tuple(edge_types), tuple(int(n) for n in num_src), tuple(int(n) for n in num_dst))
    for i, (refs, versions, s, handle) in enumerate(_handles):
        if (s == sig and len(refs) == len(edge_indices)
                and all(r() is ei and v == ei._version
                        for r, v, ei in zip(refs, versions, edge_indices))):
            if i:
                _handles.insert(0, _handles.pop(i))
            return handle
    handle = HeteroGraph(edge_types, edge_indices, num_src, num_dst)
    # (entries whose tensors are gone can never match again: drop them with their device memory)
    _handles[:] = [h for h in _handles if all(r() is not None for r in h[0])]
    _handles.insert(0, (tuple(weakref.ref(ei) for ei in edge_indices),
                        tuple(ei._version for ei in edge_indices), sig, handle))
    del _handles[_MAX_HANDLES:]
    return handle


# ---- the autograd node -----------------------------------------------------------------------------
class _Spec:
    """Static description of one aggregation node: ``node_types`` (the order of the tensor
    inputs), ``groups`` ``[(graph, [(src type, dst type, column offset, mean)])]`` and ``dst``
    ``{D: (rows, width of the operand, root column offset or None)}`` (the order of the
    outputs)."""

    def __init__(self, node_types, groups, dst):
        self.node_types, self.groups, self.dst = node_types, groups, dst


class HeteroAggregateFunction(Function):
    """``xs`` (one matrix per node type) -> one operand ``[agg_et1 | agg_et2 | ... | x_D]`` per
    destination type: one ``pygamd_hetero_spmm`` launch per source width (usually one) writes every
    aggregation block in place; the backward is one ``pygamd_hetero_spmm_backward`` launch per
    source width plus the root blocks."""

    @staticmethod
    def forward(ctx, spec: _Spec, *xs: Tensor):
        x = dict(zip(spec.node_types, xs))
        dev = xs[0].device
        outs = {d: torch.empty(rows, width, dtype=torch.float32, device=dev)
                for d, (rows, width, _) in spec.dst.items()}
        for graph, blocks in spec.groups:
            K = x[blocks[0][0]].size(1)
            _native.hetero_spmm(graph.rowptr, graph.col, graph.row_begin,
                                [x[s] for s, _, _, _ in blocks],
                                [outs[d][:, off:off + K] for _, d, off, _ in blocks],
                                [mean for _, _, _, mean in blocks])
        for d, (_, _, root_off) in spec.dst.items():
            if root_off is not None:
                outs[d][:, root_off:].copy_(x[d])
        ctx.spec = spec
        ctx.widths = {t: v.size(1) for t, v in x.items()}
        return tuple(outs.values())

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads: Tensor):
        spec = ctx.spec
        need = dict(zip(spec.node_types, ctx.needs_input_grad[1:]))
        g = {d: (go if go.stride(1) == 1 or go.size(1) <= 1 else go.contiguous())
             for d, go in zip(spec.dst, grads)}
        gx = {}
        for graph, blocks in spec.groups:
            if not any(need[t] for t in graph.src_types):
                continue
            K = ctx.widths[blocks[0][0]]
            rowptr_t, col_t = graph.transposed()
            parts = [torch.empty(graph.src_begin[i + 1] - graph.src_begin[i], K,
                                 dtype=torch.float32, device=grads[0].device)
                     for i in range(len(graph.src_types))]
            _native.hetero_spmm_backward(rowptr_t, col_t, graph.rowptr, graph.row_begin,
                                         [g[d][:, off:off + K] for _, d, off, _ in blocks],
                                         [mean for _, _, _, mean in blocks], graph.src_begin,
                                         parts)
            gx.update(zip(graph.src_types, parts))
        for d, (_, _, root_off) in spec.dst.items():
            if root_off is not None and need[d]:
                root = g[d][:, root_off:]
                gx[d] = gx[d].add_(root) if d in gx else root.contiguous()
        return (None, ) + tuple(gx.get(t) if need[t] else None for t in spec.node_types)


def run(layer_convs, p: Plan, x_dict, edge_index_dict, group_aggr) -> Dict[str, Tensor]:
    """The planned layer call: one aggregation node, then one GEMM per destination type."""
    from ._functions import linear
    conv_of = dict(layer_convs)
    # the column layout of every destination's operand
    offsets, dst_spec = {}, {}
    for d, (ets, root) in p.dst.items():
        off = 0
        for et in ets:
            offsets[et] = off
            off += x_dict[et[0]].size(1)
        root_off = off if root else None
        dst_spec[d] = (x_dict[d].size(0), off + (x_dict[d].size(1) if root else 0), root_off)
    groups = []
    for _, ets in p.groups:
        eis = [edge_index_dict[et] for et in ets]
        graph = hetero_graph(ets, eis, [x_dict[et[0]].size(0) for et in ets],
                             [x_dict[et[-1]].size(0) for et in ets])
        groups.append((graph, [(et[0], et[-1], offsets[et],
                                conv_of[et].aggr == 'mean') for et in ets]))
    node_types = list(dict.fromkeys([et[0] for et in p.edge_types] + list(p.dst)))
    spec = _Spec(node_types, groups, dst_spec)
    operands = HeteroAggregateFunction.apply(spec, *[x_dict[t] for t in node_types])
    out = {}
    for (d, (ets, root)), operand in zip(p.dst.items(), operands):
        convs = [conv_of[et] for et in ets]
        blocks = [c.lin_l.weight for c in convs]
        if root:
            roots = [c.lin_r.weight for c in convs if hasattr(c, 'lin_r')]
            blocks.append(roots[0] if len(roots) == 1 else torch.stack(roots).sum(0))
        weight = blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1)
        biases = [c.lin_l.bias for c in convs if c.lin_l.bias is not None]
        bias = None if not biases else \
            (biases[0] if len(biases) == 1 else torch.stack(biases).sum(0))
        if group_aggr == 'mean' and len(ets) > 1:
            weight = weight * (1.0 / len(ets))
            bias = None if bias is None else bias * (1.0 / len(ets))
        out[d] = linear(operand, weight, bias)
    return out
