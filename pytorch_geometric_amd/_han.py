"""The fused route of :class:`~pytorch_geometric_amd.nn.HANConv`: the stacking plan of a layer call,
the cached stacked by-destination handle and the eligibility rules.

HAN's node-level attention runs once per edge type, each with its own softmax (han_conv.py:141-156).
Stacked, the edge types of a call are ONE bipartite graph whose rows are the (edge type,
destination) pairs ``row_begin[e] + i`` — dense: an empty neighbourhood is an empty row — and whose
columns are the sources stacked by edge type, ``src_begin[e] + j``.  The projected features are
stacked once per NODE type; ``val_shift[e]`` maps a column of edge type ``e`` to its row there, so a
node type that feeds several edge types is never copied."""
import os
import weakref
from typing import Dict, List, Sequence, Tuple

import torch
from torch import Tensor

from . import _native
from ._hetero import _HOOKS, _edges_ok, _features_ok
from ._hgt import _check_ranges
from .edge_index import EdgeIndex

MAX_TYPES = _native.MAX_HETERO_TYPES
# the default of HANConv.fuse, read at import
FUSE_DEFAULT = os.environ.get('PYGAMD_FUSE_HAN', '1') not in ('', '0')


class Stacking:
    """Where every row of a layer call lives.  ``node_types``: the node types of the call in the
    order of ``x_dict`` with ``node_off[t]`` their first row of the stacked features (``num_nodes``
    rows in all); ``edge_types``: the edge types in the order of the call with ``row_begin[e]``
    their first stacked destination row (``num_rows`` in all), ``src_begin[e]`` their first stacked
    source column (``num_cols`` in all) and ``val_shift[e] = node_off[src] - src_begin[e]``."""

    def __init__(self, sizes: Dict[str, int], edge_types: Sequence[Tuple[str, str, str]]):
        self.node_types = list(sizes)
        self.sizes = {t: int(n) for t, n in sizes.items()}
        self.node_off, off = {}, 0
        for t, n in self.sizes.items():
            self.node_off[t] = off
            off += n
        self.num_nodes = off
        self.edge_types = [tuple(et) for et in edge_types]
        self.row_begin, self.src_begin, self.val_shift = [0], [0], []
        for et in self.edge_types:
            self.val_shift.append(self.node_off[et[0]] - self.src_begin[-1])
            self.src_begin.append(self.src_begin[-1] + self.sizes[et[0]])
            self.row_begin.append(self.row_begin[-1] + self.sizes[et[-1]])
        self.num_rows, self.num_cols = self.row_begin[-1], self.src_begin[-1]

    @property
    def types(self):
        """what the kernels and the operator take: ``(row_begin, src_begin, val_shift)``"""
        return tuple(self.row_begin), tuple(self.src_begin), tuple(self.val_shift)

    def signature(self):
        return (tuple(self.sizes.items()), tuple(self.edge_types))


def build_stacked(st: Stacking, edge_indices: List[Tensor]) -> EdgeIndex:
    """The stacked ``[2, E]`` edge list as an :class:`EdgeIndex` handle of size ``(num_cols,
    num_rows)``: its by-destination and by-source forms, hub plans and slot map come from the
    handle's own machinery.  Source and destination ids are range-checked once, here."""
    dev, dt = edge_indices[0].device, edge_indices[0].dtype
    E = sum(int(ei.size(1)) for ei in edge_indices)
    if dt == torch.int32 and max(st.num_cols, st.num_rows, E) >= 2 ** 31 - 1:
        raise ValueError('int32 edge indices: the stacked graph does not fit')
    live = [(k, ei) for k, ei in enumerate(edge_indices) if ei.size(1) > 0]
    if E == 0:
        stacked = torch.zeros(2, 0, dtype=dt, device=dev)
    else:
        ei_all = live[0][1] if len(live) == 1 else torch.cat([ei for _, ei in live], dim=1)
        # rows 0 / 1 bound src / dst of every edge, rows 2 / 3 shift them into the stacked spaces
        table = torch.tensor([[st.sizes[st.edge_types[k][0]] for k, _ in live],
                              [st.sizes[st.edge_types[k][-1]] for k, _ in live],
                              [st.src_begin[k] for k, _ in live],
                              [st.row_begin[k] for k, _ in live]], dtype=dt).to(dev)
        counts = torch.tensor([int(ei.size(1)) for _, ei in live]).to(dev)
        per_edge = table.repeat_interleave(counts, dim=1, output_size=E)
        if bool(((ei_all < 0) | (ei_all >= per_edge[:2])).any()):
            _check_ranges(st, edge_indices)
        stacked = ei_all + per_edge[2:]
    return EdgeIndex(stacked, (st.num_cols, st.num_rows), validate=False)


_handles: list = []   # most recent first
_MAX_HANDLES = 8


def stacked_graph(st: Stacking, edge_indices: List[Tensor]) -> EdgeIndex:
    """The stacked handle of this call, cached by tensor identity + in-place version (as
    ``_hgt.stacked_graph``) and shared by every layer of a model and by forward and backward: a
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
    ``source_to_target``, nobody observing ``propagate`` / ``message`` / ``aggregate`` (the rule
    of ``_hgt.eligible``), no dropout on the coefficients (``dropout == 0`` or not training), a
    head layout the kernels serve (``H * D <= 512``, ``H <= 64``) and at most 64 edge types and 64
    node types.  ``require_device=False`` judges CPU stand-ins (host-side tests; there is no CPU
    kernel)."""
    from .nn.conv._act_request import has_forward_hooks
    from .nn.conv.han_conv import HANConv
    if not getattr(conv, 'fuse', True) or conv.flow != 'source_to_target':
        return False
    if getattr(conv, 'explain', False) or getattr(conv, 'decomposed_layers', 1) != 1:
        return False
    if any(getattr(conv, h, None) for h in _HOOKS) or has_forward_hooks(conv):
        return False
    if type(conv).message is not HANConv.message or type(conv).aggregate is not HANConv.aggregate:
        return False
    if torch.is_autocast_enabled() or torch.jit.is_scripting() or torch.compiler.is_compiling():
        return False
    if conv.training and conv.dropout > 0:
        return False
    H, D = conv.heads, conv.out_channels // conv.heads
    if H * D > 512 or H > 64:   # pygamd_han_supported
        return False
    if not 1 <= len(edge_types) <= MAX_TYPES or not 1 <= len(x_dict) <= MAX_TYPES:
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
    return not require_device or _native.han_supported(H, D)
