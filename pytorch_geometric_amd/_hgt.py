"""The fused route of :class:`~pytorch_geometric_amd.nn.HGTConv`: the stacking plan of a layer call,
the cached stacked bipartite handle and the eligibility rules.

Once the relation transforms are applied, the layer is ONE dot-product attention over one stacked
bipartite graph (hgt_conv.py:156-232): rows are the destinations, stacked by node type; columns are
the stacked source rows ``src_off[e] + j`` of the edge types of the call.  The softmax of a
destination runs over all its incoming edges, across edge types, which is what
``TransformerAttendFunction`` computes on the stacked handle."""
import weakref
from typing import Dict, List, Sequence, Tuple

import torch
from torch import Tensor

from . import _native
from ._hetero import _HOOKS, _edges_ok, _features_ok
from .edge_index import EdgeIndex

MAX_TYPES = _native.MAX_HETERO_TYPES


class Stacking:
    """Where every row of a layer call lives in the stacked graph.  ``node_types``: the node types
    of the call in stacking order with ``dst_off[t]`` their first destination row (``num_dst``
    rows in all); ``edge_types``: the edge types of the call with ``src_off[e]`` their first
    stacked source row (``num_src`` rows in all: a node type that is the source of two edge types
    is stacked twice, once under each relation's matrices)."""

    def __init__(self, sizes: Dict[str, int], edge_types: Sequence[Tuple[str, str, str]]):
        self.node_types = list(sizes)
        self.sizes = {t: int(n) for t, n in sizes.items()}
        self.dst_off, off = {}, 0
        for t, n in self.sizes.items():
            self.dst_off[t] = off
            off += n
        self.num_dst = off
        self.edge_types = list(edge_types)
        self.src_off, off = [], 0
        for et in self.edge_types:
            self.src_off.append(off)
            off += self.sizes[et[0]]
        self.num_src = off

    def signature(self):
        return (tuple(self.sizes.items()), tuple(self.edge_types))


def _check_ranges(st: Stacking, edge_indices: List[Tensor]):
    """The ``IndexError`` of ``_hetero.HeteroGraph`` for the first offender (host reads: called
    only after the one fused device check failed)."""
    for et, ei in zip(st.edge_types, edge_indices):
        if ei.size(1) == 0:
            continue
        for row, n, what in ((0, st.sizes[et[0]], 'source'), (1, st.sizes[et[-1]], 'destination')):
            lo, hi = _native.index_minmax(ei[row]) if ei.is_cuda else \
                (int(ei[row].min()), int(ei[row].max()))
            if lo < 0 or hi >= n:
                raise IndexError(
                    f"Found indices in 'edge_index' of edge type {et} "
                    f"outside the valid range [0, {int(n) - 1}] of its {what} node type "
                    f"(got interval [{lo}, {hi}])")


def build_stacked(st: Stacking, edge_indices: List[Tensor]) -> EdgeIndex:
    """The stacked ``[2, E]`` edge list as an :class:`EdgeIndex` handle of size ``(num_src,
    num_dst)``: its by-destination and by-source forms, hub plans and slot map come from the
    handle's own machinery.  Source and destination ids are range-checked once, here."""
    dev, dt = edge_indices[0].device, edge_indices[0].dtype
    E = sum(int(ei.size(1)) for ei in edge_indices)
    if dt == torch.int32 and max(st.num_src, st.num_dst, E) >= 2 ** 31 - 1:
        raise ValueError('int32 edge indices: the stacked graph does not fit')
    live = [(k, ei) for k, ei in enumerate(edge_indices) if ei.size(1) > 0]
    if E == 0:
        stacked = torch.zeros(2, 0, dtype=dt, device=dev)
    else:
        ei_all = live[0][1] if len(live) == 1 else torch.cat([ei for _, ei in live], dim=1)
        # rows 0 / 1 bound src / dst of every edge, rows 2 / 3 shift them into the stacked spaces
        table = torch.tensor([[st.sizes[st.edge_types[k][0]] for k, _ in live],
                              [st.sizes[st.edge_types[k][-1]] for k, _ in live],
                              [st.src_off[k] for k, _ in live],
                              [st.dst_off[st.edge_types[k][-1]] for k, _ in live]], dtype=dt).to(dev)
        counts = torch.tensor([int(ei.size(1)) for _, ei in live]).to(dev)
        per_edge = table.repeat_interleave(counts, dim=1, output_size=E)
        if bool(((ei_all < 0) | (ei_all >= per_edge[:2])).any()):
            _check_ranges(st, edge_indices)
        stacked = ei_all + per_edge[2:]
    return EdgeIndex(stacked, (st.num_src, st.num_dst), validate=False)


_handles: list = []   # most recent first
_MAX_HANDLES = 8


def stacked_graph(st: Stacking, edge_indices: List[Tensor]) -> EdgeIndex:
    """The stacked handle of this call, cached by tensor identity + in-place version (as
    ``_hetero.hetero_graph``) and shared by every layer of a model and by forward and backward: a
    3-layer model sorts twice per batch (by destination, by source), not six times."""
    sig = st.signature()
    for i, (refs, versions, s, handle) in enumerate(_handles):
        if (s == sig and len(refs) == len(edge_indices)
                and all(r() is ei and v == ei._version
                        for r, v, ei in zip(refs, versions, edge_indices))):
            if i:
                _handles.insert(0, _handles.pop(i))
            return handle
    handle = build_stacked(st, edge_indices)
    _handles[:] = [h for h in _handles if all(r() is not None for r in h[0])]
    _handles.insert(0, (tuple(weakref.ref(ei) for ei in edge_indices),
                        tuple(ei._version for ei in edge_indices), sig, handle))
    del _handles[_MAX_HANDLES:]
    return handle


def eligible(conv, x_dict, edge_types, edge_index_dict, require_device: bool = True) -> bool:
    """The call takes the fused route: float32 (device) feature blocks and parameters, plain
    ``[2, E]`` int32 / int64 ``edge_index`` tensors of one dtype on one device, ``fuse``,
    ``source_to_target``, nobody observing ``propagate`` / ``message`` (the rule of
    ``_hetero.conv_eligible``), a head layout both kernels serve and at most 64 edge and node
    types.  ``require_device=False`` judges CPU stand-ins (host-side tests; there is no CPU
    kernel)."""
    from .nn.conv._act_request import has_forward_hooks
    if not getattr(conv, 'fuse', True) or conv.flow != 'source_to_target':
        return False
    if getattr(conv, 'explain', False) or getattr(conv, 'decomposed_layers', 1) != 1:
        return False
    if any(getattr(conv, h, None) for h in _HOOKS) or has_forward_hooks(conv):
        return False
    if torch.is_autocast_enabled() or torch.jit.is_scripting() or torch.compiler.is_compiling():
        return False
    H, D = conv.heads, conv.out_channels // conv.heads
    if H * D > 512 or H > 64 or D > 128:   # pygamd_hgt_supported / pygamd_transformer_supported
        return False
    if len(edge_types) > MAX_TYPES or len(x_dict) > MAX_TYPES or not x_dict:
        return False
    device = next(iter(x_dict.values())).device
    if not all(_features_ok(x, require_device) and x.device == device for x in x_dict.values()):
        return False
    if any(p.dtype != torch.float32 or p.device != device for p in conv.parameters()):
        return False
    dt = None
    for et in edge_types:
        ei = edge_index_dict[et]
        if not _edges_ok(ei, require_device) or ei.device != device:
            return False
        dt = ei.dtype if dt is None else dt
        if ei.dtype != dt:
            return False
    return not require_device or (_native.hgt_supported(H, D)
                                  and _native.transformer_supported(H, D))
