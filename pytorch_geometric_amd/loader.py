"""Mini-batch loader over a device-resident graph: the ``NeighborLoader`` role
(torch_geometric/loader/neighbor_loader.py, node_loader.py:90-207, loader/utils.py:32-83,159) for
BASELINE config 4 — seeds are drawn per batch, the k-hop neighbourhood is sampled ON THE GPU
(:mod:`.sampler`), features are gathered with the HIP gather kernel (``filter_data``'s
``x[n_id]``) and the batch never touches the host.  :class:`LinkNeighborLoader` is the
``LinkNeighborLoader`` role (loader/link_neighbor_loader.py, link_loader.py): batches of seed
links with negatives drawn on the device.  :class:`HeteroNeighborLoader` is ``NeighborLoader`` on
a ``HeteroData`` (seeds of one node type, features per node type) and
:class:`HeteroLinkNeighborLoader` ``LinkNeighborLoader`` on a ``HeteroData`` (seed links of one edge
type)."""
import queue
import threading
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Iterator, List, Optional

import torch
from torch import Tensor

import os

from . import _native
from .edge_index import EdgeIndex
from .sampler import HeteroNeighborSampler, NegativeSampling, NeighborSampler, _edge_type

# collate_slots: layer 0 of the slot stack gathers its neighbours' rows straight from the feature
# matrix (only the destination rows of a batch are copied) — slots.SlotSampler.gather(direct=True).
# PYGAMD_SLOTS_DIRECT=0 copies every row of the batch first, as rounds 4-5 did.
SLOTS_DIRECT = os.environ.get('PYGAMD_SLOTS_DIRECT', '1') != '0'


@dataclass
class Batch:
    """What a model step needs, with the reference's field names (``n_id``, ``e_id``,
    ``batch_size``, ``num_sampled_nodes`` / ``num_sampled_edges`` for ``trim_to_layer``)."""
    x: Tensor
    y: Optional[Tensor]
    edge_index: Tensor
    graph: EdgeIndex       # destination-sorted handle of `edge_index` (no sort, no host sync)
    n_id: Tensor
    e_id: Tensor
    input_id: Tensor
    batch_size: int
    num_sampled_nodes: Optional[List[int]]
    num_sampled_edges: Optional[List[int]]
    batch: Optional[Tensor] = None  # disjoint sampling: the seed (tree) index of every node
    seed_time: Optional[Tensor] = None  # temporal sampling: the int64 time of every seed

    def record_stream(self, stream) -> None:
        for t in (self.x, self.y, self.edge_index, self.n_id, self.e_id, self.input_id,
                  self.batch, self.seed_time):
            if isinstance(t, Tensor) and t.is_cuda:
                t.record_stream(stream)
        self.graph.record_stream(stream)


@dataclass
class LinkBatch(Batch):
    """A link-level mini-batch (:class:`LinkNeighborLoader`): :class:`Batch`'s fields plus the
    reference's link fields (loader/link_loader.py:264-279).  Without negatives or with binary
    ones: ``edge_label_index`` ``[2, B + num_neg]`` (local ids into ``n_id``), ``edge_label`` and
    ``edge_label_time``; with triplet ones: ``src_index``, ``dst_pos_index``, ``dst_neg_index``
    (``[B]`` or ``[B, amount]``) and ``seed_time``.  ``batch_size`` is the number of positive
    edges ``B``."""
    edge_label_index: Optional[Tensor] = None
    edge_label: Optional[Tensor] = None
    edge_label_time: Optional[Tensor] = None
    src_index: Optional[Tensor] = None
    dst_pos_index: Optional[Tensor] = None
    dst_neg_index: Optional[Tensor] = None

    def record_stream(self, stream) -> None:
        super().record_stream(stream)
        for t in (self.edge_label_index, self.edge_label, self.edge_label_time, self.src_index,
                  self.dst_pos_index, self.dst_neg_index):
            if isinstance(t, Tensor) and t.is_cuda:
                t.record_stream(stream)


@dataclass
class PaddedBatch:
    """A mini-batch at STATIC shapes (``NeighborLoader.collate_padded``): ``hops`` is the
    sampler's padded-id output (block positions as node ids, per-hop CSR pointers, device-side
    counts), ``x`` the features of all ``hops.bases[-1]`` padded rows (padding rows repeat node 0),
    ``y`` the labels of the seeds.  Nothing in it depends on a host read: sampling, gather, the
    padded hop stack (nn/models/_fused_sage_hops.py) and the optimizer step replay as one
    hipGraph."""
    x: Tensor
    y: Optional[Tensor]
    hops: object
    n_id: Tensor
    batch_size: int


class _Prefetching:
    """``__iter__`` of the loaders: batches from ``self._plan()`` through ``self.collate``, sampled
    inline (``prefetch <= 0``) or ahead of the consumer by a producer thread on its own stream."""

    def __iter__(self) -> Iterator:
        if self.prefetch <= 0:
            for seeds, sel in self._plan():
                yield self.collate(seeds, sel)
            return
        yield from self._prefetching_iter()

    def _stream_device(self):
        return self.x.device

    def _prefetching_iter(self) -> Iterator:
        dev = self._stream_device()
        if self._side is None:
            self._side = torch.cuda.Stream(dev)
        side = self._side
        plan = self._plan()
        first = next(plan, None)   # the seed tensors are made on the consumer's stream ...
        side.wait_stream(torch.cuda.current_stream(dev))  # ... before the producer reads them
        ready: 'queue.Queue' = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        def put(item) -> bool:
            while not stop.is_set():
                try:
                    ready.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    continue
            return False

        def produce():
            try:
                torch.cuda.set_device(dev)
                item = first
                with torch.cuda.stream(side):
                    while item is not None and not stop.is_set():
                        batch = self.collate(*item)
                        done = torch.cuda.Event()
                        done.record(side)
                        if not put((batch, done)):
                            return
                        item = next(plan, None)
                put(None)
            except BaseException as exc:  # surfaced in the consumer
                put(exc)

        worker = threading.Thread(target=produce, name='pyg-amd-sampler', daemon=True)
        worker.start()
        try:
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                batch, done = item
                cur = torch.cuda.current_stream(dev)
                cur.wait_event(done)
                batch.record_stream(cur)
                yield batch
        finally:
            stop.set()
            worker.join(timeout=10.0)


class NeighborLoader(_Prefetching):
    r"""Iterates over mini-batches of ``batch_size`` seed nodes with their sampled ``k``-hop
    neighbourhoods.

    Args:
        x, y: node features ``[N, F]`` (fp32, device) and optional labels ``[N]``.
        edge_index: ``[2, E]`` device tensor.
        num_neighbors: fan-out per hop (``-1`` = all).
        input_nodes: seed pool (default: all nodes); shard it across ranks with
            :func:`pytorch_geometric_amd.data_parallel.shard_seeds`.
        prefetch: number of batches sampled AHEAD of the consumer (0 = sample inside
            ``__next__``).  With ``prefetch > 0`` a producer thread samples and gathers on its own
            HIP stream while the caller trains on the previous batch — the role the reference
            gives to ``num_workers`` DataLoader processes (loader/node_loader.py:90-152), without
            leaving the device.  Batches are handed over with an event the consumer's stream
            waits on.
        replace, disjoint, subgraph_type: the sampler options of the reference's loader
            (loader/neighbor_loader.py:209-233; see :class:`~.sampler.NeighborSampler`).
        edge_weight: ``[E]`` edge weights for biased sampling, the tensor the reference's
            ``weight_attr`` names (loader/neighbor_loader.py:168-174; see
            :class:`~.sampler.NeighborSampler`).  The slot layout (:meth:`collate_slots`) stays
            uniform and refuses it.
        node_time, edge_time, temporal_strategy: temporal sampling, the tensor the reference's
            ``time_attr`` names (node-level ``[N]`` or edge-level ``[E]`` integer times) and its
            ``temporal_strategy`` (loader/neighbor_loader.py:150-165; see
            :class:`~.sampler.NeighborSampler`).  Forces ``disjoint``; :meth:`collate_padded` and
            :meth:`collate_slots` refuse it.
        input_time: the reference's ``input_time``: one integer seed time per entry of
            ``input_nodes``, shuffled and batched with them (default: ``node_time`` of the seeds;
            edge-level time needs it).  Every batch carries its seeds' times as ``seed_time``.
    """

    def __init__(self, x: Tensor, edge_index: Tensor, num_neighbors: List[int],
                 batch_size: int = 1024, y: Optional[Tensor] = None,
                 input_nodes: Optional[Tensor] = None, shuffle: bool = False,
                 drop_last: bool = False, seed: int = 0, prefetch: int = 0,
                 replace: bool = False, disjoint: bool = False,
                 subgraph_type: str = 'directional', edge_weight: Optional[Tensor] = None,
                 node_time: Optional[Tensor] = None, edge_time: Optional[Tensor] = None,
                 input_time: Optional[Tensor] = None, temporal_strategy: str = 'uniform'):
        if input_time is not None and node_time is None and edge_time is None:
            # (the reference's wording, loader/neighbor_loader.py:223-226)
            raise ValueError("Received conflicting 'input_time' and 'time_attr' arguments: "
                             "'input_time' is set while 'time_attr' is not set.")
        self.prefetch = int(prefetch)
        self._side = None
        self._slots = None  # the static-shape sampler of `collate_slots`, built on first use
        self.x, self.y = x, y
        self.num_nodes = x.size(0)
        self.sampler = NeighborSampler(edge_index, self.num_nodes, num_neighbors, seed=seed,
                                       replace=replace, disjoint=disjoint,
                                       subgraph_type=subgraph_type, edge_weight=edge_weight,
                                       node_time=node_time, edge_time=edge_time,
                                       temporal_strategy=temporal_strategy)
        if input_nodes is None:
            input_nodes = torch.arange(self.num_nodes, device=x.device)
        self.input_nodes = input_nodes.to(x.device)
        self.input_time = None
        if input_time is not None:
            if not isinstance(input_time, Tensor) or input_time.dim() != 1 \
                    or input_time.numel() != self.input_nodes.numel():
                raise ValueError("'input_time' must be a 1-D tensor with one entry per input node")
            self.input_time = self.sampler.seed_time(self.input_nodes, input_time)
        elif edge_time is not None:
            raise ValueError("temporal sampling with edge-level time ('edge_time') needs the seed "
                             "times ('input_time')")
        self.batch_size, self.shuffle, self.drop_last = batch_size, shuffle, drop_last
        self._gen = torch.Generator().manual_seed(seed)

    def __len__(self) -> int:
        n = self.input_nodes.numel()
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def collate(self, seeds: Tensor, input_id: Optional[Tensor] = None) -> Batch:
        smp = self.sampler
        seed_time = None
        if smp.is_temporal:  # input_id: positions in `input_nodes` (None: seeds given directly)
            time = None if self.input_time is None or input_id is None \
                else self.input_time[input_id]
            seed_time = smp.seed_time(seeds, time)
        out = smp.sample_from_nodes(seeds, time=seed_time)
        x = _native.gather_rows(self.x, out.node)  # filter_data: x[n_id]
        y = None if self.y is None else self.y[out.node]
        ei = torch.stack([out.row, out.col])
        fan = self.sampler.num_neighbors
        bounded = min(fan) >= 0 and self.sampler.subgraph_type == 'directional'
        graph = EdgeIndex.from_sorted_batch(
            ei, out.node.numel(), max_in_degree=max(fan) if bounded else None)
        return Batch(x=x, y=y, edge_index=ei, graph=graph, n_id=out.node,
                     e_id=out.edge, input_id=seeds if input_id is None else input_id,
                     batch_size=seeds.numel(), num_sampled_nodes=out.num_sampled_nodes,
                     num_sampled_edges=out.num_sampled_edges, batch=out.batch,
                     seed_time=seed_time)

    def collate_padded(self, seeds: Tensor, seed: int = 0,
                       seed_dev: Optional[Tensor] = None) -> PaddedBatch:
        """One batch at its static capacity, without any host synchronisation (bounded fan-outs,
        directional, non-disjoint).  ``seed_dev`` (int64 [1], device) is added to the RNG seed on
        the device: a captured step bumps it before every replay."""
        p = self.sampler.sample_padded(seeds, seed=seed, padded_ids=True, seed_dev=seed_dev,
                                       want_edge_ids=False)
        n_id = torch.cat([p.seeds] + p.new_nodes)
        x = _native.gather_rows(self.x, n_id)  # filter_data: x[n_id]
        y = None if self.y is None else self.y[seeds]
        return PaddedBatch(x=x, y=y, hops=p, n_id=n_id, batch_size=seeds.numel())

    def collate_slots(self, seeds: Tensor, epoch_dev: Tensor, with_labels: bool = True):
        """One batch in the static-shape SLOT layout (:mod:`pytorch_geometric_amd.slots`; bounded
        fan-outs, directional, non-disjoint, without replacement): 1 + 2 launches per hop for the
        sampling, 3 for the transposed CSRs of the backward, 1 for the feature gather, no host
        synchronisation.  ``epoch_dev``: int64 [1] on the device, >= 1, growing from batch to batch
        (a captured step bumps it before every replay).  Returns a ``SlotBatch`` with ``x`` = the
        gathered ``[R, 2 F]`` buffer and ``y`` = the seeds' labels (``with_labels=False``: none
        — ``slots.SlotTrainer`` reads them from ``self.y`` inside its loss launch)."""
        from .slots import SlotPlan, SlotSampler
        smp = self.sampler
        if smp.edge_weight is not None:
            raise NotImplementedError("'collate_slots' samples uniformly: weighted sampling "
                                      "(edge_weight) is served by 'collate' / 'collate_padded'")
        if smp.replace or smp.disjoint or smp.subgraph_type != 'directional' \
                or any(k < 1 for k in smp.num_neighbors):
            raise ValueError("'collate_slots' covers bounded fan-outs, directional, non-disjoint, "
                             "without replacement")
        if self._slots is None or self._slots.plan.B != seeds.numel():
            plan = SlotPlan(seeds.numel(), smp.num_neighbors, self.x.device)
            self._slots = SlotSampler(smp.colptr, smp.row, self.num_nodes, plan, seed=smp.seed)
        b = self._slots.sample(seeds, epoch_dev)
        b.x = self._slots.gather(self.x, b, direct=SLOTS_DIRECT and len(smp.num_neighbors) > 0)
        b.y = None if (self.y is None or not with_labels) else self.y[seeds]
        return b

    def _plan(self):
        n = self.input_nodes.numel()
        order = (torch.randperm(n, generator=self._gen).to(self.input_nodes.device)
                 if self.shuffle else torch.arange(n, device=self.input_nodes.device))
        nodes = self.input_nodes[order]   # ONE index launch per epoch; a batch's seeds are a view
        for b in range(len(self)):
            lo, hi = b * self.batch_size, (b + 1) * self.batch_size
            yield nodes[lo:hi], order[lo:hi]


class LinkNeighborLoader(_Prefetching):
    r"""Iterates over mini-batches of ``batch_size`` seed LINKS with their sampled ``k``-hop
    neighbourhoods: the reference's ``LinkNeighborLoader`` (loader/link_neighbor_loader.py ->
    loader/link_loader.py) for one node type, sampled on the GPU
    (:meth:`~.sampler.NeighborSampler.sample_from_edges`).

    Args:
        x, y, edge_index, num_neighbors, batch_size, shuffle, drop_last, seed, prefetch, replace,
            disjoint, subgraph_type, edge_weight, node_time, edge_time, temporal_strategy: as
            for :class:`NeighborLoader`.
        edge_label_index: ``[2, L]`` the positive links to iterate over (default:
            ``edge_index``).
        edge_label: optional ``[L, ...]`` labels of the links.  With binary negatives, labels
            whose minimum is 0 are shifted by +1 so that 0 denotes "negative"; triplet negatives
            refuse labels.
        edge_label_time: optional ``[L]`` integer times of the links, the seed times of a temporal
            sampler (which needs them; a non-temporal one refuses them).
        neg_sampling: :class:`~.sampler.NegativeSampling`, the reference's object, a ``dict`` of
            its arguments or a mode string.
        neg_sampling_ratio: shorthand for ``NegativeSampling('binary', ratio)`` (it takes
            precedence when set and non-zero).

    Yields :class:`LinkBatch`.
    """

    def __init__(self, x: Tensor, edge_index: Tensor, num_neighbors: List[int],
                 edge_label_index: Optional[Tensor] = None, edge_label: Optional[Tensor] = None,
                 edge_label_time: Optional[Tensor] = None, neg_sampling=None,
                 neg_sampling_ratio: Optional[float] = None, batch_size: int = 1024,
                 y: Optional[Tensor] = None, shuffle: bool = False, drop_last: bool = False,
                 seed: int = 0, prefetch: int = 0, replace: bool = False,
                 disjoint: bool = False, subgraph_type: str = 'directional',
                 edge_weight: Optional[Tensor] = None, node_time: Optional[Tensor] = None,
                 edge_time: Optional[Tensor] = None, temporal_strategy: str = 'uniform'):
        temporal = node_time is not None or edge_time is not None
        if (edge_label_time is not None) != temporal:
            # (the reference's wording, loader/link_neighbor_loader.py:242-249; 'time_attr' is
            # node_time / edge_time here)
            raise ValueError(
                f"Received conflicting 'edge_label_time' and 'time_attr' arguments: "
                f"'edge_label_time' is {'set' if edge_label_time is not None else 'not set'} "
                f"while 'time_attr' is {'set' if temporal else 'not set'}. Both arguments must "
                f"be provided for temporal sampling.")
        if neg_sampling_ratio is not None and neg_sampling_ratio != 0.0:
            neg_sampling = NegativeSampling('binary', neg_sampling_ratio)
        self.neg_sampling = NegativeSampling.cast(neg_sampling)
        self.num_nodes = x.size(0)
        if self.neg_sampling is not None:
            self.neg_sampling.check(self.num_nodes)
        if self.neg_sampling is not None and self.neg_sampling.is_triplet() \
                and edge_label is not None:
            # (the reference's wording, loader/link_loader.py:177-183)
            raise ValueError("'edge_label' needs to be undefined for 'triplet'-based negative "
                             "sampling. Please use `src_index`, `dst_pos_index` and "
                             "`neg_pos_index` of the returned mini-batch instead to "
                             "differentiate between positive and negative samples.")
        if edge_label_index is None:
            edge_label_index = edge_index
        if edge_label_index.dim() != 2 or edge_label_index.size(0) != 2:
            raise ValueError(f"'edge_label_index' must be a [2, L] tensor (got "
                             f"{list(edge_label_index.shape)})")
        L = edge_label_index.size(1)
        for name, t in (('edge_label', edge_label), ('edge_label_time', edge_label_time)):
            if t is not None and (t.dim() < 1 or t.size(0) != L):
                raise ValueError(f"'{name}' needs one entry per link of 'edge_label_index' ({L})")
        self.prefetch = int(prefetch)
        self._side = None
        self.x, self.y = x, y
        self.sampler = NeighborSampler(edge_index, self.num_nodes, num_neighbors, seed=seed,
                                       replace=replace, disjoint=disjoint,
                                       subgraph_type=subgraph_type, edge_weight=edge_weight,
                                       node_time=node_time, edge_time=edge_time,
                                       temporal_strategy=temporal_strategy)
        dev = x.device
        self.edge_label_index = edge_label_index.to(dev)
        if edge_label is not None:
            edge_label = edge_label.to(dev)
            if self.neg_sampling is not None and self.neg_sampling.is_binary() \
                    and L > 0 and edge_label.min() == 0:
                edge_label = edge_label + 1  # zero now denotes "negative"
        self.edge_label = edge_label
        self.edge_label_time = None if edge_label_time is None else \
            self.sampler.seed_time(self.edge_label_index[0], edge_label_time)
        self.batch_size, self.shuffle, self.drop_last = batch_size, shuffle, drop_last
        self._gen = torch.Generator().manual_seed(seed)

    def __len__(self) -> int:
        n = self.edge_label_index.size(1)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _plan(self):
        n = self.edge_label_index.size(1)
        dev = self.edge_label_index.device
        order = (torch.randperm(n, generator=self._gen).to(dev) if self.shuffle
                 else torch.arange(n, device=dev))
        for b in range(len(self)):
            sel = order[b * self.batch_size:(b + 1) * self.batch_size]
            yield self.edge_label_index[:, sel], sel

    def collate(self, edges: Tensor, input_id: Tensor) -> LinkBatch:
        """One batch from the positive links ``edges`` ``[2, B]`` (``input_id``: their positions
        in ``edge_label_index``)."""
        inp = SimpleNamespace(
            row=edges[0], col=edges[1], input_id=input_id, input_type=None,
            label=None if self.edge_label is None else self.edge_label[input_id],
            time=None if self.edge_label_time is None else self.edge_label_time[input_id])
        out = self.sampler.sample_from_edges(inp, self.neg_sampling)
        x = _native.gather_rows(self.x, out.node)  # filter_data: x[n_id]
        y = None if self.y is None else self.y[out.node]
        ei = torch.stack([out.row, out.col])
        fan = self.sampler.num_neighbors
        bounded = min(fan, default=0) >= 0 and self.sampler.subgraph_type == 'directional'
        graph = EdgeIndex.from_sorted_batch(
            ei, out.node.numel(), max_in_degree=max(fan) if bounded and fan else None)
        b = LinkBatch(x=x, y=y, edge_index=ei, graph=graph, n_id=out.node, e_id=out.edge,
                      input_id=input_id, batch_size=edges.size(1),
                      num_sampled_nodes=out.num_sampled_nodes,
                      num_sampled_edges=out.num_sampled_edges, batch=out.batch)
        md = out.metadata
        if self.neg_sampling is None or self.neg_sampling.is_binary():
            b.edge_label_index, b.edge_label, b.edge_label_time = md[1], md[2], md[3]
        else:
            b.src_index, b.dst_pos_index, b.dst_neg_index, b.seed_time = md[1:5]
        return b


@dataclass
class HeteroBatch:
    """A heterogeneous mini-batch (:class:`HeteroNeighborLoader`): per node type ``x_dict``,
    ``n_id`` and (disjoint) ``batch``; per edge type ``edge_index_dict`` (local ``[row, col]``
    into ``n_id[src]`` / ``n_id[dst]``) and ``e_id`` (positions in that type's ``edge_index``);
    ``y`` the labels of the sampled ``input_type`` nodes (seeds first); ``seed_time`` the int64
    time of every seed of a temporal batch."""
    x_dict: Dict[str, Tensor]
    edge_index_dict: Dict[tuple, Tensor]
    n_id: Dict[str, Tensor]
    e_id: Dict[tuple, Tensor]
    input_type: str
    input_id: Tensor
    batch_size: int
    num_sampled_nodes: Dict[str, List[int]]
    num_sampled_edges: Dict[tuple, List[int]]
    y: Optional[Tensor] = None
    batch: Optional[Dict[str, Tensor]] = None
    seed_time: Optional[Tensor] = None

    def record_stream(self, stream) -> None:
        for d in (self.x_dict, self.edge_index_dict, self.n_id, self.e_id, self.batch or {}):
            for t in d.values():
                if isinstance(t, Tensor) and t.is_cuda:
                    t.record_stream(stream)
        for t in (self.input_id, self.y, self.seed_time):
            if isinstance(t, Tensor) and t.is_cuda:
                t.record_stream(stream)


class HeteroNeighborLoader(_Prefetching):
    r"""Iterates over mini-batches of ``batch_size`` seed nodes of one node type with their sampled
    heterogeneous ``k``-hop neighbourhoods: the reference's ``NeighborLoader(hetero_data,
    input_nodes=...)`` (loader/neighbor_loader.py, node_loader.py:209-257), sampled on the GPU
    (:class:`~.sampler.HeteroNeighborSampler`).

    Args:
        x_dict: node features per node type ``[N_t, F_t]`` (fp32, device); their row counts are the
            numbers of nodes, their order the node types'.
        edge_index_dict: ``[2, E]`` device tensors per edge type ``(src, rel, dst)``.
        num_neighbors: one fan-out list for every edge type, or a dict keyed by edge type.
        input_nodes: the seed type, or ``(type, nodes)`` with a tensor of node ids or a boolean
            mask of that type.
        y: optional labels of the input type ``[N_input]``; a batch carries those of its sampled
            input-type nodes.
        batch_size, shuffle, drop_last, seed, prefetch, replace, disjoint: as for
            :class:`NeighborLoader`.
        node_time, edge_time, temporal_strategy: temporal sampling, the tensors the reference's
            ``time_attr`` names: a dict from node type to integer times ``[N_t]`` or from edge type
            to integer times ``[E_et]``, types may be missing (see
            :class:`~.sampler.HeteroNeighborSampler`).  Forces ``disjoint``.
        input_time: the reference's ``input_time``: one integer seed time per entry of the input
            nodes, shuffled and batched with them (default: ``node_time[input_type]`` of the seeds;
            edge-level time, or an input type without node times, needs it).  Every batch carries
            its seeds' times as ``seed_time``.

    Yields :class:`HeteroBatch`.
    """

    def __init__(self, x_dict: Dict[str, Tensor], edge_index_dict, num_neighbors, input_nodes,
                 batch_size: int = 1024, y: Optional[Tensor] = None, shuffle: bool = False,
                 drop_last: bool = False, seed: int = 0, prefetch: int = 0,
                 replace: bool = False, disjoint: bool = False, node_time=None, edge_time=None,
                 input_time: Optional[Tensor] = None, temporal_strategy: str = 'uniform'):
        if input_time is not None and node_time is None and edge_time is None:
            # (the reference's wording, loader/neighbor_loader.py:223-226)
            raise ValueError("Received conflicting 'input_time' and 'time_attr' arguments: "
                             "'input_time' is set while 'time_attr' is not set.")
        if isinstance(input_nodes, str):
            input_type, nodes = input_nodes, None
        elif isinstance(input_nodes, (tuple, list)) and len(input_nodes) == 2:
            input_type, nodes = input_nodes
        else:
            raise ValueError("'input_nodes' must be a node type or (node type, nodes)")
        if input_type not in x_dict:
            raise ValueError(f"the input type '{input_type}' has no entry in 'x_dict'")
        self.prefetch = int(prefetch)
        self._side = None
        self.x_dict, self.y = dict(x_dict), y
        self.sampler = HeteroNeighborSampler(
            edge_index_dict, {t: x.size(0) for t, x in self.x_dict.items()}, num_neighbors,
            seed=seed, replace=replace, disjoint=disjoint, node_time=node_time,
            edge_time=edge_time, temporal_strategy=temporal_strategy)
        dev = self.sampler.colptr.device
        self.input_type = input_type
        if nodes is None:
            nodes = torch.arange(self.x_dict[input_type].size(0), device=dev)
        elif nodes.dtype == torch.bool:
            nodes = nodes.nonzero().view(-1)
        self.input_nodes = nodes.to(dev)
        self.sampler.check_seeds(input_type, self.input_nodes)  # once: batches are slices of it
        self.input_time = None
        if input_time is not None:
            if not isinstance(input_time, Tensor) or input_time.dim() != 1 \
                    or input_time.numel() != self.input_nodes.numel():
                raise ValueError("'input_time' must be a 1-D tensor with one entry per input node")
            self.input_time = self.sampler.seed_time(input_type, self.input_nodes, input_time)
        elif self.sampler.is_temporal:
            self.sampler.seed_time(input_type, self.input_nodes[:0])  # refuses a missing default
        self.batch_size, self.shuffle, self.drop_last = batch_size, shuffle, drop_last
        self._gen = torch.Generator().manual_seed(seed)

    def _stream_device(self):
        return self.sampler.colptr.device

    def __len__(self) -> int:
        n = self.input_nodes.numel()
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _plan(self):
        n = self.input_nodes.numel()
        dev = self.input_nodes.device
        order = (torch.randperm(n, generator=self._gen).to(dev) if self.shuffle
                 else torch.arange(n, device=dev))
        nodes = self.input_nodes[order]
        for b in range(len(self)):
            lo, hi = b * self.batch_size, (b + 1) * self.batch_size
            yield nodes[lo:hi], order[lo:hi]

    def collate(self, seeds: Tensor, input_id: Optional[Tensor] = None) -> HeteroBatch:
        smp = self.sampler
        seed_time = None
        if smp.is_temporal:  # input_id: positions in `input_nodes` (None: seeds given directly)
            time = None if self.input_time is None or input_id is None \
                else self.input_time[input_id]
            seed_time = smp.seed_time(self.input_type, seeds, time)
        out = smp._sample(self.input_type, seeds, seed_time=seed_time)
        # filter_hetero_data: x[t][n_id[t]] per node type, with the HIP gather kernel
        x_dict = {t: _native.gather_rows(x, out.node[t]) for t, x in self.x_dict.items()}
        ei = {et: torch.stack([out.row[et], out.col[et]]) for et in out.row}
        y = None if self.y is None else self.y[out.node[self.input_type].long()]
        return HeteroBatch(x_dict=x_dict, edge_index_dict=ei, n_id=out.node, e_id=out.edge,
                           input_type=self.input_type,
                           input_id=seeds if input_id is None else input_id,
                           batch_size=seeds.numel(), num_sampled_nodes=out.num_sampled_nodes,
                           num_sampled_edges=out.num_sampled_edges, y=y, batch=out.batch,
                           seed_time=seed_time)


@dataclass
class HeteroLinkBatch(HeteroBatch):
    """A heterogeneous link-level mini-batch (:class:`HeteroLinkNeighborLoader`):
    :class:`HeteroBatch`'s fields (``input_type`` is the edge type ``(S, rel, D)`` of the seed
    links, ``batch_size`` the number of positive links ``B``) plus the reference's link fields
    (loader/link_loader.py:281-303).  Without negatives or with binary ones: ``edge_label_index``
    ``[2, B + num_neg]`` (row 0 local ids into ``n_id[S]``, row 1 into ``n_id[D]``),
    ``edge_label`` and ``edge_label_time``; with triplet ones: ``src_index`` (into ``n_id[S]``),
    ``dst_pos_index`` / ``dst_neg_index`` (into ``n_id[D]``; ``[B]`` or ``[B, amount]``) and
    ``seed_time``."""
    edge_label_index: Optional[Tensor] = None
    edge_label: Optional[Tensor] = None
    edge_label_time: Optional[Tensor] = None
    src_index: Optional[Tensor] = None
    dst_pos_index: Optional[Tensor] = None
    dst_neg_index: Optional[Tensor] = None

    def record_stream(self, stream) -> None:
        super().record_stream(stream)
        for t in (self.edge_label_index, self.edge_label, self.edge_label_time, self.src_index,
                  self.dst_pos_index, self.dst_neg_index):
            if isinstance(t, Tensor) and t.is_cuda:
                t.record_stream(stream)


class HeteroLinkNeighborLoader(_Prefetching):
    r"""Iterates over mini-batches of ``batch_size`` seed LINKS of one edge type with their sampled
    heterogeneous ``k``-hop neighbourhoods: the reference's ``LinkNeighborLoader(hetero_data,
    edge_label_index=(edge_type, edge_label_index))`` (loader/link_neighbor_loader.py ->
    loader/link_loader.py), sampled on the GPU
    (:meth:`~.sampler.HeteroNeighborSampler.sample_from_edges`).

    Args:
        x_dict, edge_index_dict, num_neighbors, batch_size, shuffle, drop_last, seed, prefetch,
            replace, disjoint, node_time, edge_time, temporal_strategy: as for
            :class:`HeteroNeighborLoader`.
        edge_label_index: ``(edge_type, tensor)``: the edge type ``(S, rel, D)`` of the seed links
            and the ``[2, L]`` positive links to iterate over (typed local ids; ``None``: that
            edge type's own ``edge_index``).
        edge_label, edge_label_time, neg_sampling, neg_sampling_ratio: as for
            :class:`LinkNeighborLoader`; the weights of ``neg_sampling`` are per endpoint type
            (``src_weight`` ``[N_S]``, ``dst_weight`` ``[N_D]``).

    Yields :class:`HeteroLinkBatch`.
    """

    def __init__(self, x_dict: Dict[str, Tensor], edge_index_dict, num_neighbors,
                 edge_label_index, edge_label: Optional[Tensor] = None,
                 edge_label_time: Optional[Tensor] = None, neg_sampling=None,
                 neg_sampling_ratio: Optional[float] = None, batch_size: int = 1024,
                 shuffle: bool = False, drop_last: bool = False, seed: int = 0,
                 prefetch: int = 0, replace: bool = False, disjoint: bool = False,
                 node_time=None, edge_time=None, temporal_strategy: str = 'uniform'):
        temporal = node_time is not None or edge_time is not None
        if (edge_label_time is not None) != temporal:
            # (the reference's wording, loader/link_neighbor_loader.py:242-249; 'time_attr' is
            # node_time / edge_time here)
            raise ValueError(
                f"Received conflicting 'edge_label_time' and 'time_attr' arguments: "
                f"'edge_label_time' is {'set' if edge_label_time is not None else 'not set'} "
                f"while 'time_attr' is {'set' if temporal else 'not set'}. Both arguments must "
                f"be provided for temporal sampling.")
        if neg_sampling_ratio is not None and neg_sampling_ratio != 0.0:
            neg_sampling = NegativeSampling('binary', neg_sampling_ratio)
        self.neg_sampling = NegativeSampling.cast(neg_sampling)
        if self.neg_sampling is not None and self.neg_sampling.is_triplet() \
                and edge_label is not None:
            # (the reference's wording, loader/link_loader.py:177-183)
            raise ValueError("'edge_label' needs to be undefined for 'triplet'-based negative "
                             "sampling. Please use `src_index`, `dst_pos_index` and "
                             "`neg_pos_index` of the returned mini-batch instead to "
                             "differentiate between positive and negative samples.")
        if not isinstance(edge_label_index, (tuple, list)) or len(edge_label_index) != 2 \
                or isinstance(edge_label_index[0], Tensor):
            raise ValueError("'edge_label_index' must be (edge_type, [2, L] tensor or None): "
                             "heterogeneous link-level sampling needs the edge type of the seed "
                             "links")
        input_type, links = edge_label_index
        input_type = _edge_type(input_type)
        edge_types = [_edge_type(k) for k in edge_index_dict.keys()]
        if input_type not in edge_types:
            raise ValueError(f"the input type '{input_type}' is not an edge type of the graph "
                             f"({edge_types})")
        for t in (input_type[0], input_type[2]):
            if t not in x_dict:
                raise ValueError(f"the node type '{t}' of the seed links has no entry in "
                                 f"'x_dict'")
        if links is None:
            links = list(edge_index_dict.values())[edge_types.index(input_type)]
        if not isinstance(links, Tensor) or links.dim() != 2 or links.size(0) != 2:
            raise ValueError(f"'edge_label_index' must be a [2, L] tensor (got "
                             f"{list(links.shape) if isinstance(links, Tensor) else type(links)})")
        L = links.size(1)
        for name, t in (('edge_label', edge_label), ('edge_label_time', edge_label_time)):
            if t is not None and (t.dim() < 1 or t.size(0) != L):
                raise ValueError(f"'{name}' needs one entry per link of 'edge_label_index' ({L})")
        if self.neg_sampling is not None:
            for w, t in ((self.neg_sampling.src_weight, input_type[0]),
                         (self.neg_sampling.dst_weight, input_type[2])):
                if w is not None and w.numel() != x_dict[t].size(0):
                    raise ValueError(f"The 'weight' attribute in 'NegativeSampling' needs to "
                                     f"match the number of nodes {x_dict[t].size(0)} of node "
                                     f"type '{t}' (got {w.numel()})")
        self.prefetch = int(prefetch)
        self._side = None
        self.x_dict = dict(x_dict)
        self.sampler = HeteroNeighborSampler(
            edge_index_dict, {t: x.size(0) for t, x in self.x_dict.items()}, num_neighbors,
            seed=seed, replace=replace, disjoint=disjoint, node_time=node_time,
            edge_time=edge_time, temporal_strategy=temporal_strategy)
        dev = self.sampler.colptr.device
        self.input_type = input_type
        self.edge_label_index = links.to(dev)
        # once: batches are column selections of it
        self.sampler.check_seeds(input_type[0], self.edge_label_index[0])
        self.sampler.check_seeds(input_type[2], self.edge_label_index[1])
        if edge_label is not None:
            edge_label = edge_label.to(dev)
            if self.neg_sampling is not None and self.neg_sampling.is_binary() \
                    and L > 0 and edge_label.min() == 0:
                edge_label = edge_label + 1  # zero now denotes "negative"
        self.edge_label = edge_label
        self.edge_label_time = None if edge_label_time is None else \
            self.sampler.seed_time(input_type[0], self.edge_label_index[0], edge_label_time)
        self.batch_size, self.shuffle, self.drop_last = batch_size, shuffle, drop_last
        self._gen = torch.Generator().manual_seed(seed)

    def _stream_device(self):
        return self.sampler.colptr.device

    def __len__(self) -> int:
        n = self.edge_label_index.size(1)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _plan(self):
        n = self.edge_label_index.size(1)
        dev = self.edge_label_index.device
        order = (torch.randperm(n, generator=self._gen).to(dev) if self.shuffle
                 else torch.arange(n, device=dev))
        for b in range(len(self)):
            sel = order[b * self.batch_size:(b + 1) * self.batch_size]
            yield self.edge_label_index[:, sel], sel

    def collate(self, edges: Tensor, input_id: Tensor) -> HeteroLinkBatch:
        """One batch from the positive links ``edges`` ``[2, B]`` (``input_id``: their positions
        in ``edge_label_index``)."""
        inp = SimpleNamespace(
            row=edges[0], col=edges[1], input_id=input_id, input_type=self.input_type,
            label=None if self.edge_label is None else self.edge_label[input_id],
            time=None if self.edge_label_time is None else self.edge_label_time[input_id])
        out = self.sampler.sample_from_edges(inp, self.neg_sampling)
        # filter_hetero_data: x[t][n_id[t]] per node type, with the HIP gather kernel
        x_dict = {t: _native.gather_rows(x, out.node[t]) for t, x in self.x_dict.items()}
        ei = {et: torch.stack([out.row[et], out.col[et]]) for et in out.row}
        b = HeteroLinkBatch(x_dict=x_dict, edge_index_dict=ei, n_id=out.node, e_id=out.edge,
                            input_type=self.input_type, input_id=input_id,
                            batch_size=edges.size(1), num_sampled_nodes=out.num_sampled_nodes,
                            num_sampled_edges=out.num_sampled_edges, batch=out.batch)
        md = out.metadata
        if self.neg_sampling is None or self.neg_sampling.is_binary():
            b.edge_label_index, b.edge_label, b.edge_label_time = md[1], md[2], md[3]
        else:
            b.src_index, b.dst_pos_index, b.dst_neg_index, b.seed_time = md[1:5]
        return b
