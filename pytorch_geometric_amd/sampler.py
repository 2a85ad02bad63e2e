"""Device-side neighbour sampling (the row that bounds BASELINE config 4).

Mirrors the contract of ``torch_geometric.sampler.NeighborSampler._sample`` ->
``torch.ops.pyg.neighbor_sample`` (torch_geometric/sampler/neighbor_sampler.py:550-620): a CSC
graph, seed nodes and a fan-out per hop in; ``SamplerOutput(node, row, col, edge,
num_sampled_nodes, num_sampled_edges)`` out (torch_geometric/sampler/base.py:168-214) — nodes
ordered seeds first, then hop by hop in order of first appearance (the reference's hash-map
insertion order); edges ordered hop by hop and, inside a hop, by destination;
``row`` / ``col`` are local source / destination indices into ``node``; ``edge`` are positions in
the original ``edge_index``.  Options of the reference's contract (loader/neighbor_loader.py:
209-233 -> sampler/neighbor_sampler.py:463-599): ``replace`` (draws with replacement: exactly k
edges per node with at least one in-neighbour), ``disjoint`` (one tree per seed: the same graph
node reached from two seeds is two batch nodes, ``batch`` holds the seed index of every node) and
``subgraph_type`` ``'directional'`` (default) or ``'bidirectional'`` (every sampled edge also in
the reverse direction, coalesced by destination; ``SamplerOutput.to_bidirectional``,
sampler/base.py:248-276) or ``'induced'`` (all edges of the graph between the sampled nodes).
``edge_weight`` is the reference's ``weight_attr`` (loader/neighbor_loader.py:168-174 ->
``NeighborSampler.edge_weight``, sampler/neighbor_sampler.py:110-114, 559-571): bounded hops draw
in proportion to edge weight (``pygamd_sample_neighbors_weighted``) — without replacement by
successive sampling (Efraimidis-Spirakis keys, a node's edges in key order), with replacement k
independent draws; a node with at most k in-neighbours (without replacement) and ``-1`` hops still
take every neighbour, so the counts, the hop structure and the relabelling are the uniform
sampler's.

Temporal sampling is the reference's ``time_attr`` / ``input_time`` / ``temporal_strategy``
(loader/neighbor_loader.py:150-165 -> sampler/neighbor_sampler.py:79-108, 386-395, 550-571):
``node_time`` ``[N]`` or ``edge_time`` ``[E]`` (integer, never both).  Every seed ``i`` has a seed
time (``NodeSamplerInput.time`` / the loader's ``input_time``, else ``node_time[seed]``; edge-level
time needs them given).  Temporal sampling is always disjoint, and every node of tree ``t`` is
bounded by ``seed_time[t]``, its root's time: the in-edge ``e = (u -> v)`` is eligible iff
``node_time[u] <= seed_time[t]`` (node-level) or ``edge_time[e] <= seed_time[t]`` (edge-level);
seeds are in the batch whatever their own time.  The sampler keeps its own CSC sorted like the
reference's ``sort_csc`` (sampler/utils.py:24-42): inside a destination the slots ascend in time,
ties in ``edge_index`` order, so a node's eligible in-edges are a prefix ``[s, hi)`` of its slots
(``pygamd_sample_temporal_window`` finds ``hi``).  ``temporal_strategy='uniform'`` runs the uniform
draws on that window (Floyd without replacement, all of it if it holds at most ``k`` slots; ``k``
independent draws with replacement if it is not empty; all of it for ``-1``);
``temporal_strategy='last'`` first narrows it to its last ``k`` slots, ``lo = max(s, hi - k)``
(``k >= 0``), then does the same: without replacement a node takes its ``min(k, window)`` most
recent eligible edges, with replacement ``k`` draws among them.  The output follows the disjoint
sampler's conventions; ``metadata = (input_id, time)``.

``sample_from_nodes`` takes either a tensor of seed nodes or the reference's
``NodeSamplerInput`` (``.node``, ``.input_id``, ``.time``; sampler/base.py:52-92) and fills
``metadata = (input_id, time)`` like ``NeighborSampler.sample_from_nodes`` does
(sampler/neighbor_sampler.py:333-356), so that ``torch_geometric.loader.NodeLoader`` can drive it
(``backend.neighbor_sampler`` wraps it in a ``BaseSampler`` subclass).

``sample_from_edges`` is link-level sampling, the homogeneous branch of the reference's
``edge_sample`` / ``neg_sample`` (sampler/neighbor_sampler.py:821-1096): ``ceil(B * amount)``
negatives per endpoint drawn on the device (``pygamd_sample_negatives``: uniform, in proportion to
the :class:`NegativeSampling` weights, or bounded by the links' times under node-level time), the
seeds ``cat([src, dst])`` deduplicated into their sorted unique (``pygamd_unique_inverse``) unless
``disjoint``, then the hops of ``sample_from_nodes`` on that seed vector, so the subgraph is the
one ``sample_from_nodes`` gives for the same seeds and ``seed``.  The reference's retry rounds for
temporal negatives test ``node_time >= seed_time`` (neighbor_sampler.py:1089) where its first round
and its comment test ``<=``; every round here uses ``<=``.

Host synchronisation.  With bounded fan-outs every hop is sized by the STATIC bound
``frontier capacity x fan-out`` and all counts stay on the device (``pygamd_sample_counts`` /
``pygamd_relabel`` read them from device memory): a batch costs ONE host read at the very end
(the hop sizes the reference's ``SamplerOutput`` reports as Python ints), instead of two per hop;
``sample_padded`` returns the padded tensors with device-side counts and no host read at all (a
batch is then hipGraph-capturable).  ``-1`` ("all neighbours") has no static bound and keeps the
per-hop reads.

Parity status: UNPINNED against the reference sampler's RNG stream — ``pyg-lib`` / ``torch-sparse``
are not installable in the build container, so ``torch.ops.pyg.neighbor_sample`` cannot be run, and
its draws are implementation-defined anyway.  What CAN be pinned is: with ``num_neighbors =
[-1] * k`` the sampled node and edge sets equal the reference's
``k_hop_subgraph(directed=True)`` exactly (golden in tests/golden/golden_khop_v1.pt, generated by
the reference's pure-Python utils/_subgraph.py:249-370), plus the contract: every sampled edge
exists, per-destination counts equal ``min(deg, k)`` without duplicates, hop structure, marginal
uniformity (tests/test_gpu_sampler.py).  The weighted draws are pinned the same way: the known
answer of the reference's ``test_weighted_homo_neighbor_loader`` (test/loader/
test_neighbor_loader.py:822-846), the exact successive-sampling inclusion probabilities and the
proportional draws with replacement (tests/test_gpu_sampler_weighted.py).  The temporal draws with
``'last'`` (and ``'uniform'`` with ``-1``) are deterministic and equal a per-tree BFS restatement of
the rules above exactly; bounded ``'uniform'`` draws keep the contract on the window and equal the
disjoint sampler bit for bit when every edge is eligible (tests/test_gpu_sampler_temporal.py).
"""
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import _native
from .edge_index import as_edge_index


@dataclass
class SamplerOutput:
    node: Tensor
    row: Tensor
    col: Tensor
    edge: Optional[Tensor]
    batch: Optional[Tensor] = None
    num_sampled_nodes: Optional[List[int]] = None
    num_sampled_edges: Optional[List[int]] = None
    orig_row: Optional[Tensor] = None
    orig_col: Optional[Tensor] = None
    metadata: Optional[Any] = None


@dataclass
class PaddedSamplerOutput:
    """Fixed-shape result of :meth:`NeighborSampler.sample_padded`: per-hop tensors at their static
    capacity with the valid counts on the device (``n_nodes[h]``, ``n_edges[h]`` int64 [1])."""
    seeds: Tensor
    new_nodes: List[Tensor]
    rows: List[Tensor]
    cols: List[Tensor]
    edges: List[Tensor]
    n_nodes: List[Tensor]
    n_edges: List[Tensor]
    # ptrs[h] [capacity of frontier h + 1]: the sampled edges of frontier position f are the slots
    # [ptrs[h][f], ptrs[h][f + 1]) of hop h — the hop's CSR pointer over its destinations
    ptrs: Optional[List[Tensor]] = None
    # padded_ids: local ids are STATIC block positions instead of dense counts — block 0 = the
    # seeds, block h + 1 = the new nodes of hop h at its capacity; bases[b] = first id of block b
    # (len = hops + 2).  A batch then has the same tensor shapes AND the same row ranges every time
    # (what a captured training step needs); rows past a block's valid count are padding.
    bases: Optional[List[int]] = None


@dataclass(init=False)
class NegativeSampling:
    r"""The negative sampling configuration of :meth:`NeighborSampler.sample_from_edges`: the
    reference's ``NegativeSampling`` (sampler/base.py:848-904) with its validation and wording.

    Args:
        mode: ``'binary'`` (random negative pairs of nodes) or ``'triplet'`` (random negative
            destinations for every positive source).
        amount: the ratio of negative to positive edges (an integer for ``'triplet'``).
        src_weight, dst_weight: optional node-level ``[num_nodes]`` weights of the source /
            destination draws (need not sum to one); uniform when not given.
    """
    mode: str
    amount: float = 1
    src_weight: Optional[Tensor] = None
    dst_weight: Optional[Tensor] = None

    def __init__(self, mode, amount=1, src_weight: Optional[Tensor] = None,
                 dst_weight: Optional[Tensor] = None):
        mode = getattr(mode, 'value', mode)  # the reference's NegativeSamplingMode
        if mode not in ('binary', 'triplet'):
            raise ValueError(f"'{mode}' is not a valid NegativeSamplingMode (expected 'binary' or "
                             f"'triplet')")
        self.mode, self.amount = mode, amount
        self.src_weight, self.dst_weight = src_weight, dst_weight
        if self.amount <= 0:
            raise ValueError(f"The attribute 'amount' needs to be positive for "
                             f"'{self.__class__.__name__}' (got {self.amount})")
        if self.is_triplet():
            if self.amount != math.ceil(self.amount):
                raise ValueError(f"The attribute 'amount' needs to be an integer for "
                                 f"'{self.__class__.__name__}' with 'triplet' negative sampling "
                                 f"(got {self.amount}).")
            self.amount = math.ceil(self.amount)

    def is_binary(self) -> bool:
        return self.mode == 'binary'

    def is_triplet(self) -> bool:
        return self.mode == 'triplet'

    def check(self, num_nodes: int) -> None:
        """The reference's weight check of ``NegativeSampling.sample`` (sampler/base.py:924-928)."""
        for w in (self.src_weight, self.dst_weight):
            if w is not None and w.numel() != num_nodes:
                raise ValueError(f"The 'weight' attribute in '{self.__class__.__name__}' needs "
                                 f"to match the number of nodes {num_nodes} (got {w.numel()})")

    @classmethod
    def cast(cls, value) -> Optional['NegativeSampling']:
        """``None``, this class, the reference's object (duck-typed: ``mode`` or ``mode.value``,
        ``amount``, ``src_weight``, ``dst_weight``), a ``dict`` of its arguments or a mode
        string."""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, dict):
            return cls(**value)
        if isinstance(value, str):
            return cls(value)
        if hasattr(value, 'mode'):
            return cls(value.mode, getattr(value, 'amount', 1), getattr(value, 'src_weight', None),
                       getattr(value, 'dst_weight', None))
        raise ValueError(f"cannot interpret {type(value).__name__} as 'NegativeSampling'")


def _check_time(t, name: str, n: int) -> None:
    if not isinstance(t, Tensor) or t.dim() != 1 or t.numel() != n:
        raise ValueError(f"'{name}' must be a 1-D tensor with {n} entries")
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"'{name}' must be an integer tensor (got {t.dtype}): temporal sampling "
                         f"takes int64 times")


def _cached_cdf(cache: dict, weight: Tensor, num_nodes: int, device) -> Tensor:
    """The fp64 inclusive CDF of a node weight vector, built once per tensor (and version) and
    kept in ``cache``: setup work, the per-batch draw is the kernel.  One host read validates it
    like ``torch.multinomial`` does (non-negative, finite, positive sum)."""
    key = id(weight)
    hit = cache.get(key)
    if hit is not None and hit[0] is weight and hit[1] == weight._version:
        return hit[2]
    if not isinstance(weight, Tensor) or weight.dim() != 1 or weight.numel() != num_nodes:
        raise ValueError(f"The 'weight' attribute in 'NegativeSampling' needs to match the "
                         f"number of nodes {num_nodes}")
    if not weight.is_floating_point():
        raise ValueError(f"negative-sampling weights must be floating (got {weight.dtype})")
    w = weight.to(device=device, dtype=torch.float64)
    cdf = torch.cumsum(w, 0)
    lo, total = (float(v) for v in torch.stack([w.min(), cdf[-1]]).tolist())
    if not (lo >= 0 and math.isfinite(total) and total > 0):
        raise ValueError("negative-sampling weights must be finite and non-negative with a "
                         "positive sum")
    if len(cache) >= 8:  # (a caller that makes a new weight tensor per batch)
        cache.clear()
    cache[key] = (weight, weight._version, cdf)
    return cdf


# ---- what NeighborSampler and HeteroNeighborSampler share ---------------------------------------------
def _subgraph_type(subgraph_type) -> str:
    subgraph_type = getattr(subgraph_type, 'value', subgraph_type)  # the reference's enum
    if subgraph_type not in ('directional', 'bidirectional', 'induced'):
        raise ValueError(f"unknown subgraph_type '{subgraph_type}'")
    return subgraph_type


def _check_temporal_strategy(temporal_strategy) -> None:
    if temporal_strategy not in ('uniform', 'last'):
        raise ValueError(f"unknown temporal_strategy '{temporal_strategy}' (expected "
                         f"'uniform' or 'last')")


def _check_seed_time(time, n: int) -> None:
    """Caller-supplied seed times: an integer tensor with one entry per seed."""
    if not isinstance(time, Tensor) or time.dim() != 1 or time.numel() != n:
        raise ValueError(f"the seed times must be a 1-D tensor with one entry per seed "
                         f"({n})")
    if time.is_floating_point() or time.is_complex() or time.dtype == torch.bool:
        raise ValueError(f"the seed times must be an integer tensor (got {time.dtype})")


def _link_input(index, neg_sampling, is_temporal: bool):
    """The input of ``sample_from_edges``, a ``[2, B]`` tensor of positive edges or an
    ``EdgeSamplerInput``-like object, as ``(src, dst, input_id, label, time, neg, B)``, with the
    checks on shapes and on times against the kind of sampler."""
    input_id = label = time = None
    if isinstance(index, Tensor):
        if index.dim() != 2 or index.size(0) != 2:
            raise ValueError(f"the positive edges must be a [2, B] tensor (got "
                             f"{list(index.shape)})")
        src, dst = index[0], index[1]
    else:
        src, dst = index.row, index.col
        input_id = getattr(index, 'input_id', None)
        label, time = getattr(index, 'label', None), getattr(index, 'time', None)
    neg = NegativeSampling.cast(neg_sampling)
    B = src.numel()
    if dst.numel() != B or src.dim() != 1 or dst.dim() != 1:
        raise ValueError('the source and destination of the positive edges must be 1-D '
                         'tensors of one length')
    if B == 0:
        raise ValueError("'sample_from_edges' needs at least one positive edge")
    if time is not None and not is_temporal:
        raise ValueError("'edge_label_time' is given but the sampler is not temporal (no "
                         "'node_time' / 'edge_time')")
    if time is None and is_temporal:
        raise ValueError("a temporal sampler needs the seed-link times ('edge_label_time')")
    return src, dst, input_id, label, time, neg, B


def _check_link_label(neg, label, B: int) -> None:
    if neg is not None and neg.is_triplet() and label is not None:
        raise ValueError("'edge_label' needs to be undefined for 'triplet'-based negative "
                         "sampling")
    if label is not None and label.size(0) != B:
        raise ValueError(f"'edge_label' needs one entry per positive edge ({B})")


def _binary_label(label, B: int, num_neg: int, device) -> Tensor:
    """The labels of binary negative sampling: the positives' (1 by default), then 0."""
    if label is None:
        label = torch.ones(B, device=device)
    return torch.cat([label, label.new_zeros((num_neg, ) + label.shape[1:])])


def _link_metadata(input_id, index, label, src_time, neg, B: int, disjoint: bool):
    """``metadata`` of a link batch from ``index``, the local id of every seed slot (int64, the
    source slots, then the destination slots: positives, then negatives)."""
    if neg is None or neg.is_binary():  # as many source as destination slots
        return (input_id, index.view(2, -1), label, src_time)
    dst_neg_index = index[2 * B:]
    if disjoint:
        dst_neg_index = dst_neg_index.view(-1, B).t()
    dst_neg_index = dst_neg_index.reshape(B, -1).squeeze(-1)
    return (input_id, index[:B], index[B:2 * B], dst_neg_index, src_time)


def _time_sorted_perm(times, edge_key, col_keys: Tensor, max_col: int):
    """The reference's ``sort_csc`` (sampler/utils.py:24-42): ``lexsort([time, column])`` as two
    stable radix sorts, first on the time key (biased to be non-negative), then on the column.
    ``times``: the int64 time vectors; one host read gives their span, which picks the key dtype.
    ``edge_key(narrow, key_dtype)`` builds the per-edge time key, where ``narrow(t)`` is ``t``
    minus the smallest time in the key dtype (applied to a vector at its own length: node times
    are narrowed at ``[N]`` and only then gathered by source, so there is no ``[E]`` int64 copy).
    Returns the permutation and the sorted column keys."""
    full = [t for t in times if t.numel() > 0]
    lo_t, hi_t = 0, 0
    if full:
        lo_t, hi_t = (int(x) for x in torch.stack(
            [torch.stack([t.min() for t in full]).min(),
             torch.stack([t.max() for t in full]).max()]).tolist())
    span = hi_t - lo_t
    if span >= 2 ** 63:
        raise ValueError('the times span more than the int64 range')
    kdt = torch.int32 if span < 2 ** 31 else torch.int64
    key = edge_key(lambda t: (t - lo_t).to(kdt), kdt)
    perm1 = _native.index_sort(key, max_value=span)[1]
    del key
    sorted_cols, perm2 = _native.index_sort(col_keys[perm1], max_value=max_col)
    return perm1[perm2], sorted_cols


def _relabel_pairs(keys_all: Tensor, keys: Tensor, total, cap: int, max_key: int):
    """The relabelling of disjoint trees.  A batch node is a pair, one int64 key; ``keys_all``
    ``[P]`` are the pairs of the batch so far, ``keys`` ``[cap]`` the pairs a hop sampled, the
    first ``total`` (a host int, or int64 [1] on the device) real and the rest ``max_key``, which
    sorts last.  One stable sort: the first appearance of a pair is the smallest position of its
    run.  Returns, over the positions of ``cat([keys_all, keys])``, ``first_of`` (the first
    position of the entry's pair) and ``rank`` (at the first position of a pair new in this hop:
    its rank among those, in order of first appearance), then ``new_keys`` ``[cap]`` (the new
    pairs in that order; unwritten past their count) and ``n_new`` (int64 [1]).  No host read."""
    dev = keys.device
    P = keys_all.numel()
    n_all = P + cap
    allk = torch.cat([keys_all, keys])
    sorted_k, perm = _native.index_sort(allk, max_value=max_key)
    head = torch.ones_like(sorted_k, dtype=torch.bool)
    head[1:] = sorted_k[1:] != sorted_k[:-1]
    gid = _native.cumsum(head.to(torch.int64)) - 1
    headpos = torch.empty(n_all + 1, dtype=torch.int64, device=dev)
    headpos.scatter_(0, torch.where(head, gid, n_all), perm)   # first position of every pair
    first_of = torch.empty(n_all, dtype=torch.int64, device=dev)
    first_of.scatter_(0, perm, headpos[gid])
    idx = torch.arange(n_all, device=dev)
    mark = (first_of == idx) & (idx >= P) & (idx < P + total)  # pairs new in this hop
    rank = _native.cumsum(mark.to(torch.int64)) - 1
    n_new = rank[-1:] + 1
    new_keys = torch.empty(cap + 1, dtype=torch.int64, device=dev)
    new_keys.scatter_(0, torch.where(mark[P:], rank[P:], cap), allk[P:])
    return first_of, rank, new_keys[:cap], n_new


class NeighborSampler:
    r"""k-hop neighbour sampler on the GPU (uniform, biased by ``edge_weight``, or temporal).

    Args:
        edge_index: ``[2, E]`` device tensor or :class:`EdgeIndex` handle (its destination-sorted
            form is the CSC ``colptr`` / ``row`` the reference's sampler consumes,
            sampler/utils.py:46-111).
        num_nodes: number of nodes of the (homogeneous) graph.
        num_neighbors: fan-out per hop; ``-1`` takes every in-neighbour.
        seed: base of the counter-based RNG; batch ``b`` uses ``seed + b``.
        output_cls: class of the returned object (default :class:`SamplerOutput`; the
            ``BaseSampler`` adapter passes ``torch_geometric.sampler.SamplerOutput``).
        replace: sample with replacement (bounded fan-outs; ``-1`` hops still take every
            neighbour once).
        disjoint: one sampled tree per seed node; fills ``batch``.
        subgraph_type: ``'directional'`` or ``'bidirectional'``.
        edge_weight: optional ``[E]`` non-negative, finite floating weights in ``edge_index``
            order (the reference's ``weight_attr``): neighbours with higher weights are more likely
            to be sampled.  Without replacement a node's draw is successive sampling in proportion
            to weight (zero-weight edges only fill up when fewer than ``k`` positive ones exist,
            uniformly among themselves); with replacement every draw picks an edge with
            probability ``w / W`` (a node whose weights are all zero — outside the reference's
            domain — draws uniformly).  Converted once to fp32 in CSC order; the draws depend on
            the seed alone, so every path (eager, synced, padded, captured) gives the same batch.
        node_time, edge_time: optional integer timestamps of the nodes ``[N]`` or of the edges
            ``[E]`` (in ``edge_index`` order), never both: temporal sampling (the reference's
            ``time_attr``).  Converted once to int64 on the device; a floating tensor is refused.
            Forces ``disjoint``; a neighbour is eligible iff its time (source node or edge) is
            at most the seed time of the tree (see the module docstring).  Not combined with
            ``edge_weight``, ``subgraph_type='induced'`` or :meth:`sample_padded`.
        temporal_strategy: ``'uniform'`` (uniform draws among the eligible neighbours) or
            ``'last'`` (the draws among the last ``k`` eligible neighbours in time order: without
            replacement, the ``k`` most recent).
    """

    def __init__(self, edge_index, num_nodes: int, num_neighbors: List[int], seed: int = 0,
                 output_cls=SamplerOutput, replace: bool = False, disjoint: bool = False,
                 subgraph_type: str = 'directional', edge_weight: Optional[Tensor] = None,
                 node_time: Optional[Tensor] = None, edge_time: Optional[Tensor] = None,
                 temporal_strategy: str = 'uniform'):
        subgraph_type = _subgraph_type(subgraph_type)
        _check_temporal_strategy(temporal_strategy)
        self.temporal_strategy = temporal_strategy
        self.is_temporal = node_time is not None or edge_time is not None
        if self.is_temporal:
            if node_time is not None and edge_time is not None:
                raise ValueError("temporal sampling takes either 'node_time' or 'edge_time', not "
                                 "both")
            if edge_weight is not None:
                raise ValueError("weighted temporal sampling ('edge_weight' with 'node_time' or "
                                 "'edge_time') is not supported")
            if node_time is not None:
                _check_time(node_time, 'node_time', num_nodes)
            else:
                _check_time(edge_time, 'edge_time', edge_index.size(-1))
            disjoint = True  # the reference: disjoint = _disjoint or is_temporal
        if subgraph_type == 'induced' and disjoint:
            # (the reference's wording, sampler/neighbor_sampler.py:486-489)
            raise ValueError("'disjoint' sampling not supported for neighbor sampling with "
                             "`subgraph_type='induced'`")
        self.replace, self.disjoint, self.subgraph_type = bool(replace), bool(disjoint), \
            subgraph_type
        graph = as_edge_index(edge_index, num_nodes, num_nodes)
        csc = graph.by_dst()
        self.graph = graph
        self.colptr, self.row, self.perm = csc.ptr, csc.idx, csc.perm
        self.edge_weight = None if edge_weight is None else self._csc_weights(edge_weight)
        self.num_nodes = num_nodes
        # temporal: `time` is node_time [N] (edge_level False) or edge_time [E] in slot order
        self.time, self.edge_level = None, edge_time is not None
        if self.is_temporal:
            self._sort_by_time(graph, node_time, edge_time)
        self.num_neighbors = list(num_neighbors)
        if any(k > _native._lib.load().pygamd_sample_max_fanout() for k in self.num_neighbors):
            raise ValueError('bounded fan-outs above 64 are not supported (use -1 for all)')
        self.seed = seed
        self.output_cls = output_cls
        self._calls = 0
        # link-level sampling: the fp64 CDFs of negative-sampling weights (per tensor) and the
        # temporal fallback node, both built on first use
        self._neg_cdf = {}
        self._neg_fallback = None
        # global -> local id map; the dtype's minimum = not in the current batch (it must sort
        # below every claim value of pygamd_relabel); reset after every batch
        self._unset = torch.iinfo(self.colptr.dtype).min
        self._local = torch.full((num_nodes, ), self._unset, dtype=self.colptr.dtype,
                                 device=self.colptr.device)
        # the same value as a DEVICE tensor: `local[idx] = python_int` stages the scalar through a
        # host-to-device copy, which a stream capture refuses
        self._unset_t = torch.full((1, ), self._unset, dtype=self.colptr.dtype,
                                   device=self.colptr.device)

    def _csc_weights(self, w) -> Tensor:
        """Validate the caller's ``[E]`` edge weights (one host read) and return them as fp32 in
        CSC slot order on the graph's device."""
        E = self.row.numel()
        if not isinstance(w, Tensor) or w.dim() != 1 or w.numel() != E:
            raise ValueError(f"'edge_weight' must be a 1-D tensor with one entry per edge ({E})")
        if not w.is_floating_point():
            raise ValueError(f"'edge_weight' must be a floating tensor (got {w.dtype})")
        w32 = w.to(device=self.row.device, dtype=torch.float32)
        if E > 0 and not bool((torch.isfinite(w32) & (w >= 0).to(w32.device)).all()):
            raise ValueError("'edge_weight' must be finite and non-negative")
        return w32[self.perm].contiguous()

    def _sort_by_time(self, graph, node_time, edge_time) -> None:
        """:func:`_time_sorted_perm` by (time, destination).  ``colptr`` is unchanged; ``row`` /
        ``perm`` are replaced by the time-sorted ones, and ``time`` keeps ``node_time`` ``[N]`` or
        ``edge_time`` in slot order."""
        dev, dt = self.row.device, self.row.dtype
        self.time = (node_time if node_time is not None else edge_time).to(
            device=dev, dtype=torch.int64).contiguous()
        if self.row.numel() == 0:
            return
        src, dst = graph[0], graph[1]
        perm, _ = _time_sorted_perm(
            [self.time],
            lambda narrow, _: (narrow(self.time).index_select(0, src) if node_time is not None
                               else narrow(self.time)),
            dst, max(self.num_nodes - 1, 0))
        self.row = src[perm].contiguous()
        self.perm = perm.to(dt)
        if edge_time is not None:
            self.time = self.time[perm].contiguous()

    def seed_time(self, seeds: Tensor, time: Optional[Tensor] = None) -> Tensor:
        """The int64 seed time of every seed of a temporal batch: ``time`` if given (integer, one
        per seed), else ``node_time[seeds]``; edge-level time needs ``time``."""
        if not self.is_temporal:
            raise ValueError('seed times belong to a temporal sampler (node_time / edge_time)')
        if time is None:
            if self.edge_level:
                raise ValueError("temporal sampling with edge-level time ('edge_time') needs the "
                                 "seed times (NodeSamplerInput.time / the loader's 'input_time')")
            return self.time[seeds.to(device=self.time.device).long()]
        _check_seed_time(time, seeds.numel())
        return time.to(device=self.row.device, dtype=torch.int64).contiguous()

    def _weight(self, k: int) -> Optional[Tensor]:
        """The weights for a hop of fan-out ``k`` (``-1`` takes every neighbour: uniform kernel)."""
        return self.edge_weight if k >= 0 else None

    # -- entry points --------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_from_nodes(self, index, seed: Optional[int] = None,
                          time: Optional[Tensor] = None, **kwargs):
        """``index``: a tensor of seed nodes or a ``NodeSamplerInput``-like object.  ``time``: the
        seed times of a temporal sampler (``index.time`` takes their place when given)."""
        input_id = None
        seeds = index
        if not isinstance(index, Tensor):
            seeds, input_id = index.node, getattr(index, 'input_id', None)
            if getattr(index, 'time', None) is not None:
                time = index.time
            if getattr(index, 'input_type', None) is not None:
                raise NotImplementedError('heterogeneous sampling is out of scope (SURVEY.md §8)')
        if time is not None and not self.is_temporal:
            raise NotImplementedError('temporal sampling is out of scope (SURVEY.md §8)')
        dev, dt = self.colptr.device, self.colptr.dtype
        seeds = seeds.to(device=dev, dtype=dt).contiguous()
        seed_time = self.seed_time(seeds, time) if self.is_temporal else None
        rng = self.seed + self._calls if seed is None else seed
        self._calls += 1
        out = self._sample_seeds(seeds, rng, seed_time)
        out.metadata = (input_id if input_id is not None else None, time)
        return out

    def _sample_seeds(self, seeds: Tensor, rng: int, seed_time: Optional[Tensor]):
        """The hops from a seed vector (device, graph dtype) and the ``subgraph_type`` step."""
        if self.disjoint:
            out = self._hops_disjoint(seeds, rng, seed_time)
        elif all(k >= 0 for k in self.num_neighbors):
            out = self._compact(self._hops_padded(seeds, rng))
        else:
            out = self._hops_synced(seeds, rng)
        if self.subgraph_type == 'bidirectional':
            out = self._to_bidirectional(out)
        elif self.subgraph_type == 'induced':
            out = self._to_induced(out)
        return out

    @torch.no_grad()
    def sample_from_edges(self, index, neg_sampling=None, seed: Optional[int] = None):
        """Link-level sampling, the reference's ``edge_sample`` (sampler/neighbor_sampler.py:
        821-1048, homogeneous branch): ``index`` is a ``[2, B]`` tensor of positive edges or an
        ``EdgeSamplerInput``-like object (``row``, ``col``, ``label``, ``time``, ``input_id``).
        ``neg_sampling``: :class:`NegativeSampling` or anything its ``cast`` takes.

        ``num_neg = ceil(B * amount)`` negatives are drawn on the device
        (``pygamd_sample_negatives``): binary draws source and destination negatives, triplet
        destination negatives only.  The seeds are ``cat([src, dst])``, deduplicated into their
        sorted unique (``pygamd_unique_inverse``, the reference's ``unique(return_inverse=True)``)
        unless ``disjoint``; the hops are :meth:`sample_from_nodes`' on that seed vector.
        ``metadata`` is ``(input_id, edge_label_index, edge_label, src_time)`` without negatives or
        with binary ones, ``(input_id, src_index, dst_pos_index, dst_neg_index, src_time)`` with
        triplet ones.  ``seed`` fixes the RNG like in :meth:`sample_from_nodes`; the negatives
        draw from a stream of their own."""
        if not isinstance(index, Tensor) and getattr(index, 'input_type', None) is not None:
            raise NotImplementedError('heterogeneous sampling is out of scope (SURVEY.md §8)')
        src, dst, input_id, label, time, neg, B = _link_input(index, neg_sampling,
                                                              self.is_temporal)
        if neg is not None:
            neg.check(self.num_nodes)
        _check_link_label(neg, label, B)
        dev, dt = self.colptr.device, self.colptr.dtype
        src = src.to(device=dev, dtype=dt)
        dst = dst.to(device=dev, dtype=dt)
        if time is not None:
            time = self.seed_time(src, time)       # int64 [B] on the device
        if label is not None:
            label = label.to(dev)
        rng = self.seed + self._calls if seed is None else seed
        self._calls += 1
        src_time = dst_time = time
        num_neg = 0
        if neg is not None:
            num_neg = math.ceil(B * neg.amount)
            if neg.is_binary():
                src = torch.cat([src, self._negatives(num_neg, neg, 0, rng, src_time)])
                dst = torch.cat([dst, self._negatives(num_neg, neg, 1, rng, dst_time)])
                label = _binary_label(label, B, num_neg, dev)
                if time is not None:
                    src_time = dst_time = time.repeat(1 + math.ceil(neg.amount))[:B + num_neg]
            else:
                dst = torch.cat([dst, self._negatives(num_neg, neg, 1, rng, dst_time)])
                if time is not None:
                    dst_time = time.repeat(1 + neg.amount)
        seeds = torch.cat([src, dst])
        if not self.disjoint:
            seeds, inverse = _native.unique_inverse(seeds, max_value=max(self.num_nodes - 1, 0))
        seed_time = torch.cat([src_time, dst_time]) if time is not None else None
        out = self._sample_seeds(seeds, rng, seed_time)
        if self.disjoint:   # local ids are seed positions
            out.batch = out.batch % B
            inverse = torch.arange(seeds.numel(), device=dev)
        out.metadata = _link_metadata(input_id, inverse, label, src_time, neg, B, self.disjoint)
        return out

    def _negatives(self, n: int, neg: NegativeSampling, endpoint: int, rng: int,
                   bound: Optional[Tensor]) -> Tensor:
        """``n`` negatives of one endpoint (0: source, 1: destination) in the graph's dtype: the
        reference's ``neg_sample`` (sampler/neighbor_sampler.py:1051-1096).  With node-level time
        draw ``j`` is bounded by ``bound[j % B]``; edge-level time draws without a bound, as the
        reference does (its ``node_time`` is ``None`` then)."""
        dev, dt = self.colptr.device, self.colptr.dtype
        weight = neg.src_weight if endpoint == 0 else neg.dst_weight
        cdf = None if weight is None else self._negative_cdf(weight)
        node_time = fallback = None
        if self.is_temporal and not self.edge_level:
            node_time = self.time
            if self._neg_fallback is None:  # the reference's node_time.argmin(), once
                self._neg_fallback = int(torch.argmin(node_time))
            fallback = self._neg_fallback
        else:
            bound = None
        return _native.sample_negatives(n, self.num_nodes, (rng * 2 + endpoint), dev, dt, cdf=cdf,
                                        node_time=node_time, bound=bound,
                                        fallback=fallback or 0)

    def _negative_cdf(self, weight: Tensor) -> Tensor:
        """The fp64 inclusive CDF of a node weight vector (:func:`_cached_cdf`)."""
        return _cached_cdf(self._neg_cdf, weight, self.num_nodes, self.colptr.device)

    @torch.no_grad()
    def sample_padded(self, seeds: Tensor, seed: Optional[int] = None, padded_ids: bool = False,
                      seed_dev: Optional[Tensor] = None,
                      want_edge_ids: bool = True) -> PaddedSamplerOutput:
        """No host synchronisation at all (bounded fan-outs only): per-hop tensors at their static
        capacities ``len(seeds) * k_0 * ... * k_h`` with the valid counts as device scalars.
        ``padded_ids``: local node ids are static block positions (see
        :class:`PaddedSamplerOutput`).  ``seed_dev`` (int64 [1], device) is added to the RNG seed
        on the device: bump it between the replays of a captured graph.  ``want_edge_ids=False``
        skips the lookup of the original edge positions (``edges`` stays empty): a training step
        without edge features never reads them, and at the papers100M shape the three random
        gathers from the 1.6 G-entry permutation cost 0.45 ms per batch."""
        if any(k < 0 for k in self.num_neighbors):
            raise ValueError("'sample_padded' needs bounded fan-outs")
        if self.is_temporal:
            raise ValueError("'sample_padded' does not cover temporal sampling (its disjoint "
                             "trees are sized on the host)")
        if self.disjoint or self.subgraph_type != 'directional':
            raise ValueError("'sample_padded' covers the directional, non-disjoint sampler only "
                             "(the other modes size their outputs on the host)")
        dev, dt = self.colptr.device, self.colptr.dtype
        seeds = seeds.to(device=dev, dtype=dt).contiguous()
        rng = self.seed + self._calls if seed is None else seed
        self._calls += 1
        out = self._hops_padded(seeds, rng, padded_ids, seed_dev, want_edge_ids)
        # (padded tails hold node 0: resetting it twice is harmless)
        self._local[seeds] = self._unset_t
        for new in out.new_nodes:
            self._local[new] = self._unset_t
        return out

    # -- bounded fan-outs: static capacities, counts on the device ------------------------------------
    def _hops_padded(self, seeds: Tensor, rng: int, padded_ids: bool = False,
                     seed_dev: Optional[Tensor] = None,
                     want_edge_ids: bool = True) -> PaddedSamplerOutput:
        dev, dt = self.colptr.device, self.colptr.dtype
        local = self._local
        n_seeds = seeds.numel()
        local[seeds] = torch.arange(n_seeds, dtype=dt, device=dev)
        frontier = seeds
        n_frontier = torch.full((1, ), n_seeds, dtype=torch.int64, device=dev)
        frontier_base = torch.zeros(1, dtype=torch.int64, device=dev)
        n_total = n_frontier.clone()
        out = PaddedSamplerOutput(seeds, [], [], [], [], [], [], ptrs=[])
        if padded_ids:
            out.bases = [0, n_seeds]
        for hop, k in enumerate(self.num_neighbors):
            cap_f = frontier.numel()
            cap_e = cap_f * k
            cnt = _native.sample_counts(self.colptr, frontier, k, n_valid=n_frontier,
                                        replace=self.replace)
            offsets = torch.zeros(cap_f + 1, dtype=dt, device=dev)
            _native.cumsum(cnt, out=offsets[1:])
            total = offsets[-1:].to(torch.int64)
            src_g, dstpos, slot = _native.sample_neighbors(
                self.colptr, self.row, frontier, offsets, cap_e, k,
                (rng * 1_000_003 + hop) & 0x7FFFFFFFFFFFFFFF, zero_fill=True,
                replace=self.replace, seed_dev=seed_dev, weight=self._weight(k))
            if padded_ids:  # the new nodes of this hop are numbered from their block's base
                n_total = torch.full((1, ), out.bases[-1], dtype=torch.int64, device=dev)
                frontier_base = torch.full((1, ), out.bases[-2], dtype=torch.int64, device=dev)
                out.bases.append(out.bases[-1] + cap_e)
            new, row_local, n_new = _native.relabel_new_nodes_padded(src_g, total, local, n_total)
            out.new_nodes.append(new)
            out.rows.append(row_local)
            out.cols.append(dstpos + frontier_base.to(dt))
            if want_edge_ids:
                out.edges.append(self.perm[slot] if cap_e > 0 else slot)
            out.n_nodes.append(n_new)
            out.n_edges.append(total)
            out.ptrs.append(offsets)
            frontier, frontier_base = new, n_total
            n_frontier, n_total = n_new, n_total + n_new
        return out

    def _compact(self, p: PaddedSamplerOutput):
        """ONE host read (all hop sizes in one transfer), then slicing by those sizes."""
        dev, dt = self.colptr.device, self.colptr.dtype
        L = len(self.num_neighbors)
        sizes = torch.cat(p.n_nodes + p.n_edges).tolist() if L > 0 else []
        n_new, n_edge = sizes[:L], sizes[L:]
        node = torch.cat([p.seeds] + [t[:n] for t, n in zip(p.new_nodes, n_new)])
        self._local[node] = self._unset_t  # leave the map clean for the next batch
        cat = (lambda ts: torch.cat([t[:n] for t, n in zip(ts, n_edge)]) if ts
               else torch.empty(0, dtype=dt, device=dev))
        return self.output_cls(node=node, row=cat(p.rows), col=cat(p.cols), edge=cat(p.edges),
                               num_sampled_nodes=[p.seeds.numel()] + n_new,
                               num_sampled_edges=n_edge)

    # -- unbounded fan-out (-1): the hop sizes are read on the host, two reads per hop ------------------
    def _hops_synced(self, seeds: Tensor, rng: int):
        dev, dt = self.colptr.device, self.colptr.dtype
        local = self._local
        n_nodes = seeds.numel()
        local[seeds] = torch.arange(n_nodes, dtype=dt, device=dev)
        nodes, rows, cols, edges = [seeds], [], [], []
        num_nodes_hop, num_edges_hop = [n_nodes], []
        frontier, frontier_base = seeds, 0
        for hop, k in enumerate(self.num_neighbors):
            if frontier.numel() == 0:
                num_nodes_hop.append(0)
                num_edges_hop.append(0)
                continue
            cnt = _native.sample_counts(self.colptr, frontier, k, replace=self.replace)
            offsets = torch.zeros(frontier.numel() + 1, dtype=dt, device=dev)
            _native.cumsum(cnt, out=offsets[1:])
            total = int(offsets[-1])  # host sync: sizes the hop's outputs (the reference's
            #                           CPU sampler is synchronous at the same point)
            src_g, dstpos, slot = _native.sample_neighbors(
                self.colptr, self.row, frontier, offsets, total, max(k, 0),
                (rng * 1_000_003 + hop) & 0x7FFFFFFFFFFFFFFF, replace=self.replace and k >= 0,
                weight=self._weight(k))
            # relabel: new nodes = sampled sources not seen yet, in order of first appearance
            new, row_local = _native.relabel_new_nodes(src_g, local, n_nodes)
            rows.append(row_local)
            cols.append(dstpos + frontier_base)
            edges.append(self.perm[slot])
            nodes.append(new)
            num_nodes_hop.append(new.numel())
            num_edges_hop.append(total)
            frontier, frontier_base = new, n_nodes
            n_nodes += new.numel()
        node = torch.cat(nodes)
        local[node] = self._unset_t  # leave the map clean for the next batch
        cat = (lambda xs: torch.cat(xs) if xs else torch.empty(0, dtype=dt, device=dev))
        return self.output_cls(node=node, row=cat(rows), col=cat(cols), edge=cat(edges),
                               num_sampled_nodes=num_nodes_hop, num_sampled_edges=num_edges_hop)

    # -- disjoint: one tree per seed --------------------------------------------------------------------
    def _hops_disjoint(self, seeds: Tensor, rng: int, seed_time: Optional[Tensor] = None):
        """The reference's ``disjoint=True`` (sampler/neighbor_sampler.py:590-591: ``batch, node =
        node.t()``): a batch node is a PAIR (seed index, graph node).  The pair is one int64 key
        ``tree * num_nodes + node``; a hop's sampled sources are relabelled against the keys of the
        batch so far with one stable sort (first appearance = smallest position in the sorted
        run), new pairs keep their order of first appearance.  Sizes are read on the host like in
        the ``-1`` path.  The draws of a node depend on its position in the frontier as well, so
        the same graph node in two trees samples independently.  ``seed_time`` (int64 [B], a
        temporal sampler): every frontier node draws from its eligible window, bounded by the seed
        time of its tree (``pygamd_sample_temporal_window`` -> ``pygamd_sample_neighbors_temporal``).
        The relabelling is :func:`_relabel_pairs` at the hop's exact size."""
        dev, dt = self.colptr.device, self.colptr.dtype
        N = self.num_nodes
        B = seeds.numel()
        if B * N >= 2 ** 62:
            raise ValueError('disjoint sampling: batch size x num_nodes overflows the pair key')
        keys_all = torch.arange(B, dtype=torch.int64, device=dev) * N + seeds.to(torch.int64)
        rows, cols, edges = [], [], []
        num_nodes_hop, num_edges_hop = [B], []
        frontier, frontier_tree, frontier_base = seeds, torch.arange(B, device=dev), 0
        for hop, k in enumerate(self.num_neighbors):
            if frontier.numel() == 0:
                num_nodes_hop.append(0)
                num_edges_hop.append(0)
                continue
            rep = self.replace and k >= 0
            hop_seed = (rng * 1_000_003 + hop) & 0x7FFFFFFFFFFFFFFF
            window = None
            if seed_time is not None:
                *window, cnt = _native.sample_temporal_window(
                    self.colptr, self.row, self.time, frontier, seed_time[frontier_tree], k,
                    edge_level=self.edge_level, replace=rep,
                    last=self.temporal_strategy == 'last')
            else:
                cnt = _native.sample_counts(self.colptr, frontier, k, replace=rep)
            offsets = torch.zeros(frontier.numel() + 1, dtype=dt, device=dev)
            _native.cumsum(cnt, out=offsets[1:])
            total = int(offsets[-1])
            src_g, dstpos, slot = _native.sample_neighbors(
                self.colptr, self.row, frontier, offsets, total, max(k, 0), hop_seed,
                replace=rep, salt_position=True, weight=self._weight(k), window=window)
            P = keys_all.numel()
            if total == 0:
                num_nodes_hop.append(0)
                num_edges_hop.append(0)
                frontier = frontier[:0]
                continue
            tree_e = frontier_tree[dstpos.long()]
            keys = tree_e * N + src_g.to(torch.int64)
            first_of, rank, new_keys, n_new = _relabel_pairs(keys_all, keys, total, total, B * N)
            new_keys = new_keys[:int(n_new)]  # host sync: sizes the next hop (the frontier)
            first_of = first_of[P:]           # per sampled edge: first position of its pair
            rows.append(torch.where(first_of < P, first_of, P + rank[first_of]).to(dt))
            cols.append((dstpos + frontier_base).to(dt))
            edges.append(self.perm[slot])
            keys_all = torch.cat([keys_all, new_keys])
            num_nodes_hop.append(new_keys.numel())
            num_edges_hop.append(total)
            frontier = (new_keys % N).to(dt)
            frontier_tree = new_keys // N
            frontier_base = P
        cat = (lambda xs: torch.cat(xs) if xs else torch.empty(0, dtype=dt, device=dev))
        return self.output_cls(node=(keys_all % N).to(dt), row=cat(rows), col=cat(cols),
                               edge=cat(edges), batch=(keys_all // N).to(dt),
                               num_sampled_nodes=num_nodes_hop, num_sampled_edges=num_edges_hop)

    # -- subgraph_type = 'induced' ---------------------------------------------------------------------
    def _to_induced(self, out):
        """The reference's ``subgraph_type='induced'`` (loader/neighbor_loader.py:146-147: "the
        returned subgraph contains the induced subgraph of all sampled nodes"; its native route is
        torch-sparse's ``neighbor_sample(..., directed=False)``, neighbor_sampler.py:600): the NODES
        are the ones the directional sampler drew, the EDGES are all edges of the graph between
        them — every in-edge of every batch node whose source is in the batch too.  Edges are
        ordered by destination (batch order), inside a destination in storage order; ``edge``
        holds positions in the original ``edge_index``; the per-hop counts describe the nodes only
        (``num_sampled_edges`` is ``None``, as for 'bidirectional').  One host read sizes the
        expansion (the in-degrees of the batch nodes) and one the result."""
        dev, dt = self.colptr.device, self.colptr.dtype
        node = out.node
        n = node.numel()
        if n == 0:
            return out
        local = self._local
        local[node] = torch.arange(n, dtype=dt, device=dev)
        cnt = _native.sample_counts(self.colptr, node, -1)      # in-degree of every batch node
        offsets = torch.zeros(n + 1, dtype=dt, device=dev)
        _native.cumsum(cnt, out=offsets[1:])
        total = int(offsets[-1])
        if total == 0:
            local[node] = self._unset_t
            e = torch.empty(0, dtype=dt, device=dev)
            out.row, out.col, out.edge, out.num_sampled_edges = e, e.clone(), e.clone(), None
            return out
        src_g, dstpos, slot = _native.sample_neighbors(self.colptr, self.row, node, offsets, total,
                                                      0, 0)     # k = 0: every in-neighbour
        loc = local[src_g]
        keep = loc != self._unset
        out.row, out.col = loc[keep].contiguous(), dstpos[keep].contiguous()
        out.edge = self.perm[slot[keep]]
        out.num_sampled_edges = None
        local[node] = self._unset_t
        return out

    # -- subgraph_type = 'bidirectional' ---------------------------------------------------------------
    def _to_bidirectional(self, out):
        """``SamplerOutput.to_bidirectional()`` (sampler/base.py:248-276 -> sampler/utils.py:143-171):
        the sampled edges plus their reverses, coalesced in destination-major order, duplicate edge
        ids merged with ``reduce='any'``; the per-hop counts no longer describe the edge list."""
        n = out.node.numel()
        dt = out.row.dtype
        row = torch.cat([out.row, out.col]).to(torch.int64)
        col = torch.cat([out.col, out.row]).to(torch.int64)
        eid = torch.cat([out.edge, out.edge])
        if row.numel() == 0:
            return out
        key, perm = _native.index_sort(col * n + row, max_value=n * n)  # destination-major
        head = torch.ones_like(key, dtype=torch.bool)
        head[1:] = key[1:] != key[:-1]
        key = key[head]
        # ('any': one of the merged ids — the first in the stable order, i.e. the sampled edge
        # itself where both directions were drawn)
        out.row, out.col, out.edge = (key % n).to(dt), (key // n).to(dt), eid[perm][head]
        out.num_sampled_nodes = out.num_sampled_edges = None
        return out


# ==== heterogeneous sampling ===========================================================================
@dataclass
class HeteroSamplerOutput:
    """The reference's ``HeteroSamplerOutput`` (sampler/base.py:504-557): per node type ``node`` /
    ``batch`` / ``num_sampled_nodes``, per edge type ``row`` / ``col`` / ``edge`` /
    ``num_sampled_edges``."""
    node: Dict[str, Tensor]
    row: Dict[Tuple[str, str, str], Tensor]
    col: Dict[Tuple[str, str, str], Tensor]
    edge: Optional[Dict[Tuple[str, str, str], Tensor]]
    batch: Optional[Dict[str, Tensor]] = None
    num_sampled_nodes: Optional[Dict[str, List[int]]] = None
    num_sampled_edges: Optional[Dict[Tuple[str, str, str], List[int]]] = None
    orig_row: Optional[Dict[Tuple[str, str, str], Tensor]] = None
    orig_col: Optional[Dict[Tuple[str, str, str], Tensor]] = None
    metadata: Optional[Any] = None


def _edge_type(key) -> Tuple[str, str, str]:
    """An edge type as a ``(src, rel, dst)`` tuple: the reference's ``EdgeTypeStr`` rules
    (typing.py:359-390): ``'src__rel__dst'`` strings are split, ``(src, dst)`` gets ``'to'``."""
    if isinstance(key, str):
        key = tuple(key.split('__'))
    key = tuple(key)
    if len(key) == 2:
        key = (key[0], 'to', key[1])
    if len(key) != 3 or not all(isinstance(k, str) for k in key):
        raise ValueError(f"'{key}' is not an edge type (expected '(src, rel, dst)')")
    return key


def hetero_num_neighbors(num_neighbors, edge_types: List[Tuple[str, str, str]]
                         ) -> Dict[Tuple[str, str, str], List[int]]:
    """The fan-outs per edge type by the reference's ``NumNeighbors`` rules (sampler/base.py:
    699-790) and wording: one list for every edge type, or a dict keyed by edge type (plus an
    optional ``default`` list for the types it leaves out, given as ``(values, default)`` or as the
    reference's ``NumNeighbors`` object); every list has the same number of hops."""
    default = None
    if hasattr(num_neighbors, 'values') and not isinstance(num_neighbors, dict):
        num_neighbors, default = num_neighbors.values, getattr(num_neighbors, 'default', None)
    elif isinstance(num_neighbors, tuple) and len(num_neighbors) == 2 \
            and isinstance(num_neighbors[0], dict):
        num_neighbors, default = num_neighbors
    if isinstance(num_neighbors, (tuple, list)):
        if default is not None:
            raise ValueError(f"'default' must be set to 'None' in case a single list is given as "
                             f"the number of neighbors (got '{type(default)})'")
        out = {et: list(num_neighbors) for et in edge_types}
    elif isinstance(num_neighbors, dict):
        values = {_edge_type(k): list(v) for k, v in num_neighbors.items()}
        if set(values) - set(edge_types):
            raise ValueError("Not all edge types specified in 'num_neighbors' exist in the graph")
        out = {}
        for et in edge_types:
            if et in values:
                out[et] = values[et]
            elif default is None:
                raise ValueError(f"Missing number of neighbors for edge type '{et}'")
            else:
                out[et] = list(default)
    else:
        raise ValueError(f"'num_neighbors' must be a list or a dict keyed by edge type (got "
                         f"{type(num_neighbors).__name__})")
    num_hops = {len(v) for v in out.values()}
    if len(num_hops) > 1:
        raise ValueError(f"Number of hops must be the same across all edge types (got "
                         f"{len(num_hops)} different number of hops)")
    for et, ks in out.items():
        for k in ks:
            if int(k) != k or k < -1:
                raise ValueError(f"fan-outs are integers >= -1 (got {k} for edge type '{et}')")
    return out


class HeteroNeighborSampler:
    r"""Heterogeneous k-hop neighbour sampler on the GPU: the reference's ``NeighborSampler`` on a
    ``HeteroData`` (sampler/neighbor_sampler.py:438-548 -> ``pyg-lib``'s
    ``hetero_neighbor_sample(..., csc=True)``), uniform draws, optionally temporal.

    Node types and edge types keep the order of ``num_nodes_dict`` / ``edge_index_dict``.  An edge
    type ``(src, rel, dst)`` samples in-edges of ``dst`` nodes and discovers ``src`` nodes.  Hop
    ``h`` goes through the edge types in order and draws ``k = num_neighbors[et][h]`` in-neighbours
    (``min(deg, k)`` without replacement, ``k`` with replacement where ``deg > 0``, all for ``-1``)
    for every ``dst`` node ADDED in hop ``h - 1`` (the seeds, of the input type, count as hop -1).
    A newly seen ``src`` node is appended to its type's list in order of first appearance in that
    iteration; a node found in hop ``h`` is never a destination in hop ``h``.  The edges of a type
    are ordered hop by hop, then by destination, then by draw; ``row`` / ``col`` are local indices
    into ``node[src]`` / ``node[dst]`` and ``edge`` the positions in that type's own
    ``edge_index``.  ``num_sampled_nodes[t]`` has ``hops + 1`` entries for every node type,
    ``num_sampled_edges[et]`` ``hops`` for every edge type.  ``disjoint``: nodes are (tree, node)
    pairs and ``batch[t]`` the seed index of every node.

    Device layout: ONE stacked CSC over every edge type, built at construction with one stable
    radix sort keyed by ``col_base[et] + dst`` (node ``i`` of type ``t`` is the global id
    ``node_base[t] + i``; ``row`` holds global ids, ``perm`` positions in each type's
    ``edge_index``).  A hop is one set of launches whatever the number of edge types
    (``pygamd_hetero_sample_counts``, ``pygamd_cumsum``, ``pygamd_hetero_sample_neighbors``, the
    relabelling over the global id map (disjoint: the pair-key sort) and ``pygamd_hetero_split``)
    and ONE host read: the hop's edge boundaries per edge type and new nodes per node type.  The
    draws are sized by a static bound (``k`` per item); a hop with a ``-1`` fan-out is sized by
    its exact total instead, read after the counts (a second host read), so its buffers follow
    the edges it really draws and not destinations x the largest in-degree.  Seeds are checked
    against their type's node count (host seeds on the host, device seeds with one read).  With one
    node type and one edge type the batch is :class:`NeighborSampler`'s for the same ``seed`` bit
    for bit.

    Temporal sampling (the reference's ``time_attr`` on a ``HeteroData``, sampler/utils.py:114-137,
    neighbor_sampler.py:438-471):

    1. ``node_time`` is a dict from node type to an integer tensor ``[N_t]``, ``edge_time`` a dict
       from edge type (keys normalised like those of ``num_neighbors``) to an integer tensor
       ``[E_et]`` in that type's ``edge_index`` order.  Only one of the two may be given; types may
       be missing.  Unknown keys, wrong lengths and floating, bool or complex tensors are refused
       before any device work.
    2. An edge type ``(src, rel, dst)`` is *timed* iff ``src`` has an entry in ``node_time`` or the
       edge type one in ``edge_time``.  A timed edge type keeps the slots of every column ascending
       in time, ties in ``edge_index`` order (the reference's ``sort_csc``); an untimed one keeps
       ``edge_index`` order and all of its in-edges are eligible, whatever the strategy.
    3. A temporal sampler is always ``disjoint``.
    4. An in-edge of a timed type is eligible iff its time (the source node's, or the edge's) is
       ``<=`` the seed time of the TREE its destination belongs to: the bound is the root's time,
       not the destination's.
    5. Per work item (edge type, destination), with that edge type's ``k`` of the hop:
       ``'uniform'`` draws from the eligible prefix of the column, ``'last'`` from its last ``k``
       slots (``k >= 0``).  The count is ``min(window, k)`` (``k`` wherever the window is not empty
       with ``replace``, for bounded ``k`` only), and ``-1`` takes the whole window.
    6. Seed times are one int64 per seed: ``sample_from_nodes((type, seeds), time=...)``,
       ``NodeSamplerInput.time`` or the loader's ``input_time``; the default is
       ``node_time[input_type][seeds]``.  Without a default (edge-level time, or an input type
       without an entry in ``node_time``) they must be given.  A non-temporal sampler refuses
       seed times.
    7. Everything else is as above: node and edge ordering, ``num_sampled_*``, ``batch``, both
       index dtypes, the limits, one host read per hop (two for a ``-1`` hop).

    A temporal CSC is built as ``lexsort([time key, stacked column])`` with two stable radix sorts
    (the time key biased by the smallest time, 0 for untimed edge types), and keeps ONE int64
    ``time`` vector: over the global node ids (node level) or over the slots (edge level).  A
    temporal hop replaces the counts launch by ``pygamd_hetero_sample_temporal_window`` (one wave
    per item: the 64-probe search of the homogeneous sampler, bounded by ``seed_time[tree]``
    gathered once per hop) and draws with ``pygamd_hetero_sample_neighbors_temporal``.  A sampler
    without times takes none of this.  With one node type and one edge type the temporal batch is
    :class:`NeighborSampler`'s ``node_time`` / ``edge_time`` batch bit for bit.

    Link-level sampling (:meth:`sample_from_edges`; the reference's ``LinkNeighborLoader(
    hetero_data, edge_label_index=((S, rel, D), eli))`` -> ``edge_sample``, heterogeneous branch,
    sampler/neighbor_sampler.py:852-998).  For ``P`` seed links of the edge type ``(S, rel, D)``:

    1. Negatives: ``num_neg = ceil(P * amount)``.  Binary draws ``num_neg`` sources in
       ``[0, N_S)`` and ``num_neg`` destinations in ``[0, N_D)``, triplet destinations only; the
       :class:`NegativeSampling` weights are per endpoint type (``src_weight`` ``[N_S]``,
       ``dst_weight`` ``[N_D]``).  Under node-level time the draws of an endpoint are bounded by
       the link's time (draw ``j`` by ``time[j % P]``) iff that endpoint's node type has an entry
       in ``node_time`` (fallback: that type's earliest node); edge-level time never bounds them.
    2. ``pygamd_hetero_link_seeds`` writes the whole seed block ``[src | src negatives | dst | dst
       negatives]`` as global ids, and the seed time of every slot, in ONE launch; its negatives
       are ``pygamd_sample_negatives``' for the seed ``rng * 2 + endpoint``.
    3. ``S != D``: the seed dict is ``{S: src, D: dst}``.  Not disjoint: each made unique on its
       own (``node[S]`` / ``node[D]`` start with the sorted unique seeds of their type) by ONE
       ``pygamd_unique_inverse`` over the global ids, which are type-major; ONE host read gives
       the number of distinct seeds and the split point between the two types.  Disjoint (no host
       read for the seeds): the TREES ARE NUMBERED CONSECUTIVELY THROUGH THE SEED DICT IN ITS
       ORDER: source seed ``j`` is tree ``j``, destination seed ``j`` tree ``n_src + j`` (``n_src
       = P``, or ``P + num_neg`` for binary), and the seed time of a tree is the entry of
       ``cat([src_time, dst_time])`` at that number.  ``S == D``: one merged seed vector
       ``cat([src, dst])`` of that type, unique unless disjoint, as in :class:`NeighborSampler`.
    4. The hops start from both blocks; ``batch[t] %= P`` for every node type (disjoint).  As in
       the reference, the folded id names the tree's positive link only when ``n_src`` is a
       multiple of ``P`` (triplet, or binary with an integer ``amount``); the time bound uses
       the unfolded tree id and holds for every ``amount``.
    5. ``metadata``: ``(input_id, edge_label_index, edge_label, src_time)`` without negatives or
       with binary ones, ``(input_id, src_index, dst_pos_index, dst_neg_index, src_time)`` with
       triplet ones (``dst_neg_index`` ``[P]`` for ``amount == 1``, else ``[P, amount]``).  Row 0
       / ``src_index`` are local ids into ``node[S]``, row 1 / ``dst_*_index`` into ``node[D]``
       (int64, device).  Disjoint with ``S != D``: both rows are ``arange(P + num_neg)``,
       ``dst_pos_index = arange(P)`` and ``dst_neg_index`` starts at ``P``.
    6. With one node type and one edge type the output is
       :meth:`NeighborSampler.sample_from_edges`' for the same ``seed`` bit for bit.

    Out of scope, refused: edge weights (``edge_weight``, alone or with time), floating-point
    times, ``subgraph_type`` ``'bidirectional'`` / ``'induced'``, seed links without their edge
    type, the static-shape and hipGraph paths, ``sample_direction='backward'`` and
    ``(FeatureStore, GraphStore)`` inputs."""


    def __init__(self, edge_index_dict, num_nodes_dict, num_neighbors, seed: int = 0,
                 replace: bool = False, disjoint: bool = False,
                 subgraph_type: str = 'directional', output_cls=HeteroSamplerOutput,
                 edge_weight=None, node_time=None, edge_time=None,
                 temporal_strategy: str = 'uniform'):
        subgraph_type = _subgraph_type(subgraph_type)
        if subgraph_type != 'directional':
            raise ValueError(f"heterogeneous sampling supports subgraph_type='directional' only "
                             f"(got '{subgraph_type}')")
        if edge_weight is not None:
            raise ValueError("weighted heterogeneous sampling ('edge_weight') is not supported")
        _check_temporal_strategy(temporal_strategy)
        for name, t in (('node_time', node_time), ('edge_time', edge_time)):
            if t is not None and not isinstance(t, dict):
                raise ValueError(f"temporal heterogeneous sampling takes '{name}' as a dict keyed "
                                 f"by {name[:4]} type (got {type(t).__name__})")
        if node_time is not None and edge_time is not None:
            raise ValueError("temporal sampling takes either 'node_time' or 'edge_time', not "
                             "both")
        self.temporal_strategy = temporal_strategy
        self.is_temporal = node_time is not None or edge_time is not None
        self.edge_level = edge_time is not None
        self.node_types = list(num_nodes_dict.keys())
        self.num_nodes = {t: int(n) for t, n in num_nodes_dict.items()}
        if len(self.node_types) == 0:
            raise ValueError("heterogeneous sampling needs at least one node type")
        if len(self.node_types) > 64 or len(edge_index_dict) > 64:
            raise ValueError("heterogeneous sampling supports up to 64 node types and 64 edge "
                             "types")
        if any(n < 0 for n in self.num_nodes.values()):
            raise ValueError("the number of nodes of a type must be non-negative")
        self.edge_types = [_edge_type(k) for k in edge_index_dict.keys()]
        if len(set(self.edge_types)) != len(self.edge_types):
            raise ValueError("an edge type is given twice")
        eis = list(edge_index_dict.values())
        for et, ei in zip(self.edge_types, eis):
            if et[0] not in self.num_nodes or et[2] not in self.num_nodes:
                raise ValueError(f"edge type '{et}' names a node type missing from "
                                 f"'num_nodes_dict'")
            if not isinstance(ei, Tensor) or ei.dim() != 2 or ei.size(0) != 2:
                raise ValueError(f"the edge_index of '{et}' must be a [2, E] tensor")
        dtypes = {ei.dtype for ei in eis}
        if len(dtypes) > 1:
            raise ValueError(f"every edge_index must have one index dtype (got "
                             f"{sorted(str(d) for d in dtypes)})")
        dt = dtypes.pop() if dtypes else torch.int64
        if dt not in (torch.int32, torch.int64):
            raise ValueError(f"edge_index must be int32 or int64 (got {dt})")
        self.num_neighbors = hetero_num_neighbors(num_neighbors, self.edge_types)
        self.num_hops = len(next(iter(self.num_neighbors.values()))) if self.edge_types else 0
        if any(k > _native._lib.load().pygamd_sample_max_fanout()
               for ks in self.num_neighbors.values() for k in ks):
            raise ValueError('bounded fan-outs above 64 are not supported (use -1 for all)')
        # the global id spaces: node_base[t] (nodes), col_base[et] (stacked columns)
        nb = [0]
        for t in self.node_types:
            nb.append(nb[-1] + self.num_nodes[t])
        self.node_base = nb
        self._type_index = {t: i for i, t in enumerate(self.node_types)}
        cb = [0]
        for et in self.edge_types:
            cb.append(cb[-1] + self.num_nodes[et[2]])
        self.col_base = cb
        self.num_edges = [int(ei.size(1)) for ei in eis]
        node_time, edge_time = self._check_times(node_time, edge_time)
        if dt == torch.int32 and max(nb[-1], cb[-1], sum(self.num_edges)) >= 2 ** 31:
            raise ValueError("int32 edge_index: the total number of nodes, of stacked columns or "
                             "of edges does not fit in int32 (use int64)")
        devs = {ei.device for ei in eis}
        if len(devs) > 1:
            raise ValueError("every edge_index must be on one device")
        dev = devs.pop() if devs else torch.device('cuda', torch.cuda.current_device())
        if dev.type != 'cuda':
            raise ValueError("the sampler needs every 'edge_index' on the HIP device (there is no "
                             "CPU fallback)")
        # (the reference: disjoint = _disjoint or is_temporal)
        self.seed, self.replace = seed, bool(replace)
        self.disjoint = bool(disjoint) or self.is_temporal
        self.subgraph_type = subgraph_type
        self.output_cls = output_cls
        self._calls = 0
        self.time = None
        # link-level sampling: the fp64 CDFs of negative-sampling weights (per tensor) and the
        # temporal fallback node of every node type, both built on first use
        self._neg_cdf, self._neg_fallback = {}, {}
        self._build_csc(eis, dt, dev, node_time, edge_time)
        self._unset = torch.iinfo(dt).min
        self._local = torch.full((max(nb[-1], 1), ), self._unset, dtype=dt, device=dev)
        self._unset_t = torch.full((1, ), self._unset, dtype=dt, device=dev)

    def _check_times(self, node_time, edge_time):
        """Rules 1 and 2 on host-side facts only: the dicts with normalised keys, and
        ``timed_mask`` (bit ``e``: edge type ``e`` is timed) / ``timed_node_types``."""
        self.timed_mask, self.timed_node_types = 0, set()
        if node_time is not None:
            node_time = dict(node_time)
            for t, v in node_time.items():
                if t not in self.num_nodes:
                    raise ValueError(f"'node_time' names the node type '{t}', which is not a "
                                     f"node type of the graph ({self.node_types})")
                _check_time(v, f"node_time['{t}']", self.num_nodes[t])
            self.timed_node_types = set(node_time)
            for e, et in enumerate(self.edge_types):
                if et[0] in node_time:
                    self.timed_mask |= 1 << e
        if edge_time is not None:
            edge_time = {_edge_type(k): v for k, v in edge_time.items()}
            for et, v in edge_time.items():
                if et not in self.edge_types:
                    raise ValueError(f"'edge_time' names the edge type '{et}', which is not an "
                                     f"edge type of the graph")
                _check_time(v, f"edge_time[{et}]", self.num_edges[self.edge_types.index(et)])
            for e, et in enumerate(self.edge_types):
                if et in edge_time:
                    self.timed_mask |= 1 << e
        return node_time, edge_time

    def _time_keys(self, eis, live, dev, node_time, edge_time):
        """Fills ``self.time`` (node level: int64 over the global node ids; edge level: the
        per-edge times in the order of the stacked edge list, permuted into slot order by the
        caller) and returns the ``times`` and ``edge_key`` of :func:`_time_sorted_perm`: the
        key of an edge is its time (its source node's, or its own), 0 for an untimed edge type."""
        times = node_time if node_time is not None else edge_time
        vals = {k: v.to(device=dev, dtype=torch.int64).contiguous() for k, v in times.items()}
        zeros = (lambda e, dtype: torch.zeros(eis[e].size(1), dtype=dtype, device=dev))
        if node_time is not None:
            self.time = torch.zeros(max(self.node_base[-1], 1), dtype=torch.int64, device=dev)
            for t, v in vals.items():
                b = self.node_base[self._type_index[t]]
                self.time[b:b + v.numel()] = v
            of = (lambda e: vals.get(self.edge_types[e][0]))
            key = (lambda e, narrow: narrow(of(e)).index_select(0, eis[e][0].long()))
        else:
            of = (lambda e: vals.get(self.edge_types[e]))
            key = (lambda e, narrow: narrow(of(e)))
            self.time = torch.cat([of(e) if of(e) is not None else zeros(e, torch.int64)
                                   for e in live]) if live else \
                torch.zeros(1, dtype=torch.int64, device=dev)

        def edge_key(narrow, kdt):
            return torch.cat([key(e, narrow) if of(e) is not None else zeros(e, kdt)
                              for e in live])
        return list(vals.values()), edge_key

    def _build_csc(self, eis, dt, dev, node_time=None, edge_time=None) -> None:
        """The stacked CSC: one stable radix sort of every edge keyed by ``col_base[et] + dst``
        (slots of a column stay in ``edge_index`` order).  Two host reads at construction: one
        validates the indices (before any of them is used as an address), one gives every edge
        type's largest in-degree (the static bound of ``-1`` hops).  A temporal sampler sorts
        ``lexsort([time key, stacked column])`` instead, as two stable sorts (the reference's
        ``sort_csc`` per timed edge type), with one more host read for the span of the times."""
        ET = len(self.edge_types)
        C = self.col_base[-1]
        eis = [ei.to(dev) for ei in eis]
        live = [e for e in range(ET) if eis[e].size(1) > 0]
        if live:
            host = torch.stack([torch.stack([eis[e].min().long(), eis[e][0].max().long(),
                                             eis[e][1].max().long()]) for e in live]).tolist()
            for e, (lo, hi_src, hi_dst) in zip(live, host):
                et = self.edge_types[e]
                if lo < 0 or hi_src >= self.num_nodes[et[0]] or hi_dst >= self.num_nodes[et[2]]:
                    raise ValueError(f"the edge_index of '{et}' holds node indices outside "
                                     f"[0, num_nodes) of its source / destination type")
        if live:
            keys = torch.cat([eis[e][1].long() + self.col_base[e] for e in live]).to(dt)
            srcs = torch.cat([eis[e][0].long() + self.node_base[self._type_index[
                self.edge_types[e][0]]] for e in live])
            pos = torch.cat([torch.arange(eis[e].size(1), device=dev) for e in live])
            if self.is_temporal:
                p, skeys = _time_sorted_perm(
                    *self._time_keys(eis, live, dev, node_time, edge_time), keys, max(C - 1, 0))
                if self.edge_level:
                    self.time = self.time[p].contiguous()
            else:
                skeys, p = _native.index_sort(keys, max_value=max(C - 1, 0))
            self.colptr = _native.index2ptr(skeys, C)
            self.row = srcs[p].to(dt).contiguous()
            self.perm = pos[p].to(dt).contiguous()
        else:
            self.colptr = torch.zeros(C + 1, dtype=dt, device=dev)
            self.row = torch.empty(0, dtype=dt, device=dev)
            self.perm = torch.empty(0, dtype=dt, device=dev)
            if self.is_temporal:
                self._time_keys(eis, live, dev, node_time, edge_time)
        deg = self.colptr[1:] - self.colptr[:-1]
        maxdeg = [deg[self.col_base[e]:self.col_base[e + 1]].max().long()
                  if self.num_edges[e] > 0 else torch.zeros((), dtype=torch.int64, device=dev)
                  for e in range(ET)]
        self.max_in_degree = [int(v) for v in torch.stack(maxdeg).tolist()] if ET else []

    # -- entry points --------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_from_nodes(self, index, seed: Optional[int] = None,
                          time: Optional[Tensor] = None, **kwargs):
        """``index``: ``(input_type, seeds)`` or a ``NodeSamplerInput``-like object (``.node``,
        ``.input_id``, ``.input_type``, ``.time``).  ``time``: the seed times of a temporal sampler
        (``index.time`` takes their place when given; a non-temporal sampler refuses them).
        ``metadata = (input_id, time)``."""
        input_id = None
        if isinstance(index, (tuple, list)):
            if len(index) != 2:
                raise ValueError("'index' must be (input_type, seeds)")
            input_type, seeds = index
        else:
            seeds, input_id = index.node, getattr(index, 'input_id', None)
            input_type = getattr(index, 'input_type', None)
            if getattr(index, 'time', None) is not None:
                time = index.time
        if time is not None and not self.is_temporal:
            raise ValueError("seed times belong to a temporal sampler ('node_time' / "
                             "'edge_time'): this heterogeneous sampler has none")
        if input_type not in self._type_index:
            raise ValueError(f"the input type '{input_type}' is not a node type of the graph "
                             f"({self.node_types})")
        self.check_seeds(input_type, seeds)
        seed_time = self.seed_time(input_type, seeds, time) if self.is_temporal else None
        out = self._sample(input_type, seeds, seed, seed_time)
        out.metadata = (input_id, time)
        return out

    def seed_time(self, input_type: str, seeds: Tensor, time: Optional[Tensor] = None) -> Tensor:
        """The int64 seed time of every seed of a temporal batch: ``time`` if given (integer, one
        per seed), else ``node_time[input_type][seeds]``; edge-level time, or an input type without
        node times, needs ``time``."""
        if not self.is_temporal:
            raise ValueError('seed times belong to a temporal sampler (node_time / edge_time)')
        if time is None:
            if self.edge_level:
                raise ValueError("temporal sampling with edge-level time ('edge_time') needs the "
                                 "seed times (NodeSamplerInput.time / the loader's 'input_time')")
            if input_type not in self.timed_node_types:
                raise ValueError(f"temporal sampling from the input type '{input_type}', which "
                                 f"has no entry in 'node_time', needs the seed times "
                                 f"(NodeSamplerInput.time / the loader's 'input_time')")
            idx = seeds.to(device=self.time.device).long() + \
                self.node_base[self._type_index[input_type]]
            return self.time[idx]
        _check_seed_time(time, seeds.numel())
        return time.to(device=self.row.device, dtype=torch.int64).contiguous()

    def check_seeds(self, input_type: str, seeds) -> None:
        """Seeds must be a 1-D integer tensor of ids in ``[0, num_nodes[input_type])``: an id past
        its type would name a node of the next type in the stacked id space.  Host seeds are
        checked on the host; device seeds cost one host read (``pygamd_index_minmax``)."""
        if not isinstance(seeds, Tensor) or seeds.dim() != 1:
            raise ValueError("the seed nodes must be a 1-D tensor")
        if seeds.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"the seed nodes must be int32 or int64 (got {seeds.dtype})")
        if seeds.numel() == 0:
            return
        if seeds.is_cuda:
            lo, hi = _native.index_minmax(seeds)
        else:
            lo, hi = int(seeds.min()), int(seeds.max())
        n = self.num_nodes[input_type]
        if lo < 0 or hi >= n:
            raise ValueError(f"seed node ids must lie in [0, {n}) for node type '{input_type}' "
                             f"(got {lo} .. {hi})")

    def _sample(self, input_type: str, seeds: Tensor, seed: Optional[int] = None,
                seed_time: Optional[Tensor] = None):
        """The batch of already checked seeds (``seed_time``: :meth:`seed_time`'s, temporal)."""
        seeds = seeds.to(device=self.colptr.device, dtype=self.colptr.dtype).contiguous()
        rng = self.seed + self._calls if seed is None else seed
        self._calls += 1
        return self._hops([(input_type, seeds)], rng, seed_time)

    @torch.no_grad()
    def sample_from_edges(self, index, neg_sampling=None, seed: Optional[int] = None):
        """Link-level sampling from seed links of ONE edge type, the heterogeneous branch of the
        reference's ``edge_sample`` (sampler/neighbor_sampler.py:852-998).  ``index``:
        ``(edge_type, [2, B] tensor)`` or an ``EdgeSamplerInput``-like object (``row``, ``col``,
        ``label``, ``time``, ``input_id``, ``input_type`` = the edge type).  ``neg_sampling``:
        :class:`NegativeSampling` or anything its ``cast`` takes; its weights are per endpoint
        type.  See the class docstring for the seed blocks, the tree numbering and ``metadata``.
        ``seed`` fixes the RNG like in :meth:`sample_from_nodes`; the negatives draw from a stream
        of their own."""
        if isinstance(index, Tensor):
            raise NotImplementedError(
                "heterogeneous link-level sampling needs the edge type of the seed links: pass "
                "(edge_type, [2, B] tensor) or an EdgeSamplerInput with 'input_type'")
        if isinstance(index, (tuple, list)):
            if len(index) != 2:
                raise ValueError("'index' must be (edge_type, [2, B] tensor)")
            input_type, index = index
            if not isinstance(index, Tensor):
                raise ValueError(f"the positive edges must be a [2, B] tensor (got "
                                 f"{type(index)})")
        else:
            input_type = getattr(index, 'input_type', None)
            if input_type is None:
                raise NotImplementedError(
                    "heterogeneous link-level sampling needs the edge type of the seed links "
                    "('input_type' of the EdgeSamplerInput)")
        et = _edge_type(input_type)
        if et not in self.edge_types:
            raise ValueError(f"the input type '{et}' is not an edge type of the graph "
                             f"({self.edge_types})")
        s_t, d_t = et[0], et[2]
        src, dst, input_id, label, time, neg, B = _link_input(index, neg_sampling,
                                                              self.is_temporal)
        if neg is not None:
            for w, t in ((neg.src_weight, s_t), (neg.dst_weight, d_t)):
                if w is not None and w.numel() != self.num_nodes[t]:
                    raise ValueError(f"The 'weight' attribute in 'NegativeSampling' needs to "
                                     f"match the number of nodes {self.num_nodes[t]} of node "
                                     f"type '{t}' (got {w.numel()})")
        _check_link_label(neg, label, B)
        self.check_seeds(s_t, src)
        self.check_seeds(d_t, dst)
        dev, dt = self.colptr.device, self.colptr.dtype
        src = src.to(device=dev, dtype=dt)
        dst = dst.to(device=dev, dtype=dt)
        if time is not None:
            time = self.seed_time(s_t, src, time)  # int64 [B] on the device
        if label is not None:
            label = label.to(dev)
        rng = self.seed + self._calls if seed is None else seed
        self._calls += 1
        # the seed block, ONE launch: [src | src negatives | dst | dst negatives] as global ids,
        # and the seed time of every slot
        mode, num_neg = None, 0
        if neg is not None:
            mode, num_neg = neg.mode, math.ceil(B * neg.amount)
        binary = mode == 'binary'
        ends = [self._link_endpoint(s_t, neg.src_weight if binary else None, binary),
                self._link_endpoint(d_t, neg.dst_weight if neg is not None else None,
                                    neg is not None)]
        g_seeds, seed_time = _native.hetero_link_seeds(src, dst, num_neg, mode, rng, ends,
                                                       link_time=time)
        n_src = B + (num_neg if binary else 0)
        src_time = None if time is None else seed_time[:n_src]
        if binary:
            label = _binary_label(label, B, num_neg, dev)
        si, di = self._type_index[s_t], self._type_index[d_t]
        inverse = None  # the local id of every seed slot: sources, then destinations
        if si == di:    # one node type: the merged seed vector cat([src, dst])
            seeds = g_seeds - self.node_base[si] if self.node_base[si] else g_seeds
            if not self.disjoint:
                seeds, inverse = _native.unique_inverse(
                    seeds, max_value=max(self.num_nodes[s_t] - 1, 0))
            blocks = [(s_t, seeds)]
        elif self.disjoint:
            blocks = [(s_t, g_seeds[:n_src] - self.node_base[si]),
                      (d_t, g_seeds[n_src:] - self.node_base[di])]
        else:
            # ONE unique over the global ids: they are type-major, so the sorted unique holds the
            # sorted unique seeds of the type with the lower index, then the other type's; ONE
            # host read gives the number of distinct seeds and the split point between the two
            lo_i, hi_i = min(si, di), max(si, di)
            uniq, inverse, n_u = _native.unique_inverse(
                g_seeds, max_value=max(self.node_base[-1] - 1, 0), count_on_device=True)
            pos = torch.arange(uniq.numel(), device=dev)
            n_lo = ((uniq < self.node_base[hi_i]) & (pos < n_u)).sum().view(1)
            n_uniq, n_first = torch.cat([n_u, n_lo]).tolist()
            first = uniq[:n_first] - self.node_base[lo_i]
            second = uniq[n_first:n_uniq] - self.node_base[hi_i]
            if si < di:     # the ids of the second type count from its own first seed
                inverse[n_src:] -= n_first
                blocks = [(s_t, first), (d_t, second)]
            else:
                inverse[:n_src] -= n_first
                blocks = [(s_t, second), (d_t, first)]
        out = self._hops(blocks, rng, seed_time)
        if self.disjoint:
            out.batch = {t: b % B for t, b in out.batch.items()}
            # local ids are seed positions: of node[S] / node[D] for two node types, of the
            # merged vector (destinations after the n_src sources) for one
            inverse = torch.arange(g_seeds.numel(), device=dev)
            if si != di:
                inverse[n_src:] -= n_src
        out.metadata = _link_metadata(input_id, inverse, label, src_time, neg, B, self.disjoint)
        return out

    def _link_endpoint(self, node_type: str, weight: Optional[Tensor], draws: bool) -> dict:
        """The per-endpoint table of ``pygamd_hetero_link_seeds``.  For an endpoint that draws
        negatives: the cached fp64 CDF of its weights, and, under node-level time, the type's
        slice of the time vector with its fallback ``node_time[t].argmin()`` (one host read per
        node type, once) iff the type has an entry in ``node_time``."""
        ti = self._type_index[node_type]
        n, base = self.num_nodes[node_type], self.node_base[ti]
        ep = {'num_nodes': n, 'node_base': base}
        if not draws:
            return ep
        if weight is not None:
            ep['cdf'] = _cached_cdf(self._neg_cdf, weight, n, self.colptr.device)
        if self.is_temporal and not self.edge_level and node_type in self.timed_node_types \
                and n > 0:
            ep['node_time'] = self.time[base:base + n]
            if node_type not in self._neg_fallback:
                self._neg_fallback[node_type] = int(torch.argmin(ep['node_time']))
            ep['fallback'] = self._neg_fallback[node_type]
        return ep

    def sample_padded(self, *args, **kwargs):
        raise NotImplementedError("the static-shape paths (sample_padded, collate_padded, "
                                  "collate_slots, hipGraph capture) do not cover heterogeneous "
                                  "sampling")

    # -- the hop loop --------------------------------------------------------------------------------
    def _capacity(self, e: int, k: int, n_items: int, distinct: bool) -> int:
        """Static bound on the edges edge type ``e`` can draw for ``n_items`` destinations
        (``distinct``: no destination repeats, so ``-1`` takes at most every edge once).  For
        ``-1`` it only decides whether the hop draws anything: such a hop is sized by its exact
        total (see :meth:`_hops`)."""
        d = self.max_in_degree[e]
        if k < 0:
            cap = n_items * d
            return min(cap, self.num_edges[e]) if distinct else cap
        if self.replace:
            return n_items * k if d > 0 else 0
        return n_items * min(k, d)

    def _hops(self, blocks, rng: int, seed_time: Optional[Tensor] = None):
        """The hop loop from typed seed blocks.  ``blocks``: ``[(node type, seeds)]`` (typed local
        ids, device, graph dtype) of distinct node types in seed-dict order: one block for
        :meth:`sample_from_nodes`, the source and the destination block for seed links between
        two node types.  ``node[t]`` starts with type ``t``'s block.  The frontier buffer is
        type-major by node-type index whatever the order of the blocks; ``disjoint``: the trees
        are numbered consecutively through the blocks in THEIR order (seed ``j`` of the second
        block is tree ``len(first block) + j``).  ``seed_time`` (int64, one per tree, a temporal
        sampler): the counts launch becomes the typed window, bounded by the seed time of every
        frontier node's tree, and the draw runs on the windows."""
        dev, dt = self.colptr.device, self.colptr.dtype
        T, ET = len(self.node_types), len(self.edge_types)
        tis = [self._type_index[t] for t, _ in blocks]
        assert len(set(tis)) == len(tis), 'one seed block per node type'
        B = sum(sd.numel() for _, sd in blocks)     # seeds = trees of a disjoint batch
        S = self.node_base[-1]
        count = [0] * T               # nodes of every type in the batch so far
        block_off, block_n = [0] * T, [0] * T  # the frontier's type-major blocks
        prev = [0] * T                # typed local id of every frontier block's first node
        nodes = [[] for _ in range(T)]
        trees = [[] for _ in range(T)]
        rows, cols, edges = ([[] for _ in range(ET)] for _ in range(3))
        n_nodes = [[0] for _ in range(T)]
        n_edges = [[] for _ in range(ET)]
        if self.disjoint and B * max(S, 1) >= 2 ** 62:
            raise ValueError('disjoint sampling: batch size x num_nodes overflows the pair key')
        tree0, acc = [], 0            # first tree id of every block
        for _, sd in blocks:
            tree0.append(acc)
            acc += sd.numel()
        front, ftrees, typed0, off = [], [], [], 0
        for b in sorted(range(len(blocks)), key=lambda b: tis[b]):
            tin, sd = tis[b], blocks[b][1]
            n = sd.numel()
            count[tin] = block_n[tin] = n_nodes[tin][0] = n
            block_off[tin] = off
            off += n
            nodes[tin].append(sd)
            front.append(sd + self.node_base[tin])
            if self.disjoint:
                tree = torch.arange(tree0[b], tree0[b] + n, device=dev)
                trees[tin].append(tree)
                ftrees.append(tree)
                typed0.append(torch.arange(n, dtype=dt, device=dev))
            else:
                self._local[front[-1]] = torch.arange(n, dtype=dt, device=dev)

        def cat(xs):
            return torch.cat(xs) if len(xs) > 1 else (xs[0] if xs else
                                                     torch.empty(0, dtype=dt, device=dev))
        frontier = cat(front)
        if self.disjoint:
            ftree, n_front = cat(ftrees), B
            keys_all = ftree * S + frontier.long()
            pos2typed = cat(typed0)
        else:
            local = self._local
            touched = [frontier]
        for hop in range(self.num_hops):
            item_begin, table, cap, unbounded = [0], [], 0, False
            window = None
            for e, et in enumerate(self.edge_types):
                d = self._type_index[et[2]]
                k = int(self.num_neighbors[et][hop])
                table.append((block_off[d], self.col_base[e] - self.node_base[d], prev[d], k))
                item_begin.append(item_begin[-1] + block_n[d])
                c = self._capacity(e, k, block_n[d], hop > 0 and not self.disjoint)
                cap += c
                unbounded |= k < 0 and c > 0
            if cap > 0:
                if seed_time is not None:
                    # the hop's ONE gather of seed times (the work items name the first n_front
                    # entries of the frontier buffers only; the rest is unwritten capacity)
                    ftime = seed_time[ftree[:n_front]]
                    *window, cnt = _native.hetero_sample_temporal_window(
                        self.colptr, self.row, self.time, frontier, ftime, item_begin, table,
                        self.timed_mask, edge_level=self.edge_level, replace=self.replace,
                        last=self.temporal_strategy == 'last')
                else:
                    cnt = _native.hetero_sample_counts(self.colptr, frontier, item_begin, table,
                                                       replace=self.replace)
                offsets = torch.zeros(item_begin[-1] + 1, dtype=dt, device=dev)
                if unbounded and dt == torch.int32 and cap >= 2 ** 31:
                    # the int32 scan could wrap: take the exact total from an int64 scan first
                    if int(_native.cumsum(cnt.to(torch.int64))[-1]) >= 2 ** 31:
                        raise ValueError('int32 graph: a hop draws more than 2^31 - 1 edges (use '
                                         'int64)')
                _native.cumsum(cnt, out=offsets[1:])
                if unbounded:
                    # a -1 fan-out has no useful static bound (destinations x largest in-degree
                    # is orders of magnitude above a hop with one hub): size the hop by its
                    # exact total, a second host read, as NeighborSampler's -1 hops do
                    cap = int(offsets[-1])
                elif dt == torch.int32 and cap >= 2 ** 31:
                    raise ValueError('int32 graph: a hop can draw more than 2^31 - 1 edges (use '
                                     'int64)')
            if cap == 0:  # nothing to draw (no destinations, k = 0 or no in-edges)
                for t in range(T):
                    n_nodes[t].append(0)
                for e in range(ET):
                    n_edges[e].append(0)
                prev, block_n = list(count), [0] * T
                continue
            hop_seed = (rng * 1_000_003 + hop) & 0x7FFFFFFFFFFFFFFF
            total = offsets[-1:].to(torch.int64)
            # (a temporal sampler is disjoint: salted, with the frontier positions)
            src, col, edge, fpos = _native.hetero_sample_neighbors(
                self.colptr, self.row, self.perm, frontier, offsets, cap, item_begin, table,
                hop_seed, replace=self.replace, salt_position=self.disjoint,
                want_fpos=self.disjoint, window=window)
            if self.disjoint:
                row, sg, sl, tree_sorted, new_keys, typed, stats = self._relabel_disjoint(
                    keys_all, ftree, fpos, src, total, pos2typed, cap, count, offsets,
                    item_begin, B, S)
            else:
                new, n_new = _native.relabel_claim_assign(src, total, local)
                sg, sl, _, _, stats = _native.hetero_split(new, n_new, self.node_base, count,
                                                           offsets, item_begin, local_map=local)
                row = _native.relabel_lookup(src, total, local)
            host = stats.tolist()  # the hop's ONE host read: new nodes per type, edge bounds
            new_t, bounds = host[:T], host[T:]
            for e in range(ET):
                a, b = bounds[e], bounds[e + 1]
                rows[e].append(row[a:b])
                cols[e].append(col[a:b])
                edges[e].append(edge[a:b])
                n_edges[e].append(b - a)
            off = 0
            for t in range(T):
                block_off[t], block_n[t] = off, new_t[t]
                nodes[t].append(sl[off:off + new_t[t]])
                if self.disjoint:
                    trees[t].append(tree_sorted[off:off + new_t[t]])
                n_nodes[t].append(new_t[t])
                off += new_t[t]
            if self.disjoint:
                keys_all = torch.cat([keys_all, new_keys[:off]])
                pos2typed = torch.cat([pos2typed, typed[:off]])
                ftree, n_front = tree_sorted, off
            else:
                touched.append(sg[:off])
            prev = list(count)
            count = [c + n for c, n in zip(count, new_t)]
            frontier = sg
        if not self.disjoint:
            local[torch.cat(touched)] = self._unset_t  # leave the map clean for the next batch

        nt, ets = self.node_types, self.edge_types
        out = self.output_cls(
            node={t: cat(nodes[i]) for i, t in enumerate(nt)},
            row={et: cat(rows[e]) for e, et in enumerate(ets)},
            col={et: cat(cols[e]) for e, et in enumerate(ets)},
            edge={et: cat(edges[e]) for e, et in enumerate(ets)},
            batch=({t: cat(trees[i]).to(dt) for i, t in enumerate(nt)} if self.disjoint
                   else None),
            num_sampled_nodes={t: n_nodes[i] for i, t in enumerate(nt)},
            num_sampled_edges={et: n_edges[e] for e, et in enumerate(ets)})
        return out

    def _relabel_disjoint(self, keys_all, ftree, fpos, src, total, pos2typed, cap, count,
                          offsets, item_begin, B, S):
        """:func:`_relabel_pairs` (pair ``tree * S + global id``) at the hop's static capacity,
        without a host read, then the typed split of the new pairs."""
        dev, dt = src.device, src.dtype
        P = keys_all.numel()
        ar = torch.arange(cap, device=dev)
        keys = ftree[fpos.long()] * S + src.long()
        keys = torch.where(ar < total, keys, B * S)       # the unused capacity sorts last
        first_of, rank, new_keys, n_new = _relabel_pairs(keys_all, keys, total, cap, B * S)
        new_g = (new_keys % S).to(dt) if S > 0 else new_keys.to(dt)
        sg, sl, typed, tree_sorted, stats = _native.hetero_split(
            new_g, n_new, self.node_base, count, offsets, item_begin, want_typed=True,
            aux=new_keys // max(S, 1))
        f = first_of[P:]
        row = torch.where(f < P, pos2typed[f.clamp(max=max(P - 1, 0))],
                          typed[rank[f].clamp(min=0)])
        return row, sg, sl, tree_sorted, new_keys, typed, stats
