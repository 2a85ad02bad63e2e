"""Uniform vs weighted neighbour sampling at the BASELINE config-4 shape (bench.py's mini-batch
mode: ``powerlaw_undirected`` at the ogbn-papers100M shape, generated on the device; batch 1024,
fan-outs [15, 10, 5]), with uniform random edge weights in [0, 1).

Prints JSON lines:
  batch   — ``sample_from_nodes`` per batch, uniform and weighted alternately (device events,
            after warm-up; median / min over the timed batches);
  kernel  — the hop kernels alone on the frontiers of one batch (device events over repeated
            launches), with the weighted kernel's byte model: 4 B per in-edge weight of every
            frontier node that draws (deg > k), plus the index reads (colptr x 2, offsets x 2,
            frontier) of every frontier node and the index read (row) and 3 writes of every
            chosen slot; the uniform kernel's model drops the weights;
  copy    — the box's device copy rate (read + write bytes of a 4 GiB clone over its time).
Usage: python scripts/time_weighted_sampling.py [--scale 1.0] [--batches 20] [--reps 50]
       [--out FILE]"""
import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_geometric_amd import _native  # noqa: E402
from pytorch_geometric_amd.datasets import powerlaw_undirected  # noqa: E402
from pytorch_geometric_amd.sampler import NeighborSampler  # noqa: E402


def timed(fn, reps, dev):
    """Per-call milliseconds of ``reps`` back-to-back calls (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scale', type=float, default=1.0, help='fraction of the papers100M shape')
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    fan = [15, 10, 5]
    N = int(111_059_956 * args.scale)
    E = int(1_615_685_872 * args.scale) // 2 * 2
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    ei = powerlaw_undirected(N, E, seed=3, device=dev)
    w = torch.rand(E, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    sw = NeighborSampler(ei, N, fan, seed=17, edge_weight=w)
    del w
    su = copy.copy(sw)            # the same CSC graph and id map, without weights
    su.edge_weight = None
    torch.cuda.synchronize(dev)
    idx_b = sw.colptr.element_size()
    emit({'what': 'graph', 'N': N, 'E': E, 'scale': args.scale, 'idx_bytes': idx_b,
          'batch': args.batch, 'fanouts': fan})
    n_b = args.warmup + args.batches
    pool = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(11))
    pool = pool[:n_b * args.batch].clone()

    # -- whole batches, alternating ------------------------------------------------------------
    ms = {'uniform': [], 'weighted': []}
    for i in range(n_b):
        seeds = pool[i * args.batch:(i + 1) * args.batch]
        for name, smp in (('uniform', su), ('weighted', sw)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            smp.sample_from_nodes(seeds, seed=i)
            b.record()
            torch.cuda.synchronize(dev)
            if i >= args.warmup:
                ms[name].append(a.elapsed_time(b))
    for name, v in ms.items():
        v = sorted(v)
        emit({'what': 'batch', 'sampler': name, 'median_ms': round(v[len(v) // 2], 4),
              'min_ms': round(v[0], 4), 'n': len(v)})

    # -- the hop kernels alone, on the frontiers of one batch ------------------------------------
    seeds = pool[:args.batch]
    p = sw.sample_padded(seeds, seed=1)
    torch.cuda.synchronize(dev)
    frontier, n_valid = seeds.to(sw.colptr.dtype), args.batch
    for hop, k in enumerate(fan):
        offsets = p.ptrs[hop]
        cap_e = frontier.numel() * k
        n_edges = int(p.n_edges[hop])
        f = frontier[:n_valid].long()
        deg = (sw.colptr[f + 1] - sw.colptr[f]).long()
        w_bytes = 4 * int(deg[deg > k].sum())
        idx_bytes = idx_b * (5 * n_valid + 4 * n_edges)
        res = {'what': 'kernel', 'hop': hop, 'k': k, 'frontier': n_valid,
               'drawing_nodes': int((deg > k).sum()), 'weights_read': w_bytes // 4,
               'sampled_edges': n_edges}
        for name, wt, nbytes in (('uniform', None, idx_bytes),
                                 ('weighted', sw.edge_weight, idx_bytes + w_bytes)):
            def launch():
                _native.sample_neighbors(sw.colptr, sw.row, frontier, offsets, cap_e, k, 12345,
                                         weight=wt)
            launch()
            t = timed(launch, args.reps, dev)
            res[f'{name}_ms'] = round(t, 5)
            res[f'{name}_bytes'] = nbytes
            res[f'{name}_GBps'] = round(nbytes / t / 1e6, 1)
        emit(res)
        frontier = p.new_nodes[hop]
        n_valid = int(p.n_nodes[hop])

    # -- the box's copy rate ---------------------------------------------------------------------
    src = torch.empty(1 << 30, dtype=torch.float32, device=dev)
    src.fill_(1.0)
    dst = torch.empty_like(src)
    dst.copy_(src)
    t = timed(lambda: dst.copy_(src), 10, dev)
    emit({'what': 'copy', 'bytes': 2 * src.numel() * 4, 'ms': round(t, 4),
          'GBps': round(2 * src.numel() * 4 / t / 1e6, 1)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            for d in lines:
                fh.write(json.dumps(d) + '\n')


if __name__ == '__main__':
    main()
