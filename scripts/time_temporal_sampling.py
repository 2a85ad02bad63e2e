"""Disjoint uniform vs temporal neighbour sampling at the BASELINE config-4 shape (bench.py's
mini-batch mode: ``powerlaw_undirected`` at the ogbn-papers100M shape, generated on the device;
batch 1024, fan-outs [15, 10, 5]), with random integer node times in [0, 1000) and the seeds' own
node times as seed times.

Prints JSON lines:
  graph   — the shape and the one-off cost of the time-sorted CSC (two stable radix sorts);
  batch   — ``sample_from_nodes`` per batch: disjoint-uniform, temporal-uniform and temporal-last
            alternately (device events, after warm-up; median / min over the timed batches);
  window  — ``pygamd_sample_temporal_window`` alone on the frontiers of one temporal batch (device
            events over repeated launches), against ``pygamd_sample_counts`` on the same frontier,
            with the window kernel's byte model: per frontier node the index reads (frontier,
            colptr x 2), the 8-byte seed time and the three index writes (lo, hi, cnt), plus per
            probe the source id and its 8-byte node time; a node of in-degree d <= 64 makes d
            probes, a larger one 64 per round over ceil(log64(d)) rounds (useful bytes, not
            cache lines);
  copy    — the box's device copy rate (read + write bytes of a 4 GiB clone over its time).
Usage: python scripts/time_temporal_sampling.py [--scale 1.0] [--batches 20] [--reps 50]
       [--out FILE]"""
import argparse
import copy
import json
import math
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
    node_time = torch.randint(0, 1000, (N, ), device=dev,
                              generator=torch.Generator(device=dev).manual_seed(7))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    st = NeighborSampler(ei, N, fan, seed=17, node_time=node_time)
    b.record()
    torch.cuda.synchronize(dev)
    build_ms = a.elapsed_time(b)
    del ei
    sl = copy.copy(st)            # the same time-sorted CSC and id map, strategy 'last'
    sl.temporal_strategy = 'last'
    sd = copy.copy(st)            # ... and as a plain disjoint sampler (no time)
    sd.is_temporal, sd.time = False, None
    torch.cuda.synchronize(dev)
    idx_b = st.colptr.element_size()
    emit({'what': 'graph', 'N': N, 'E': E, 'scale': args.scale, 'idx_bytes': idx_b,
          'batch': args.batch, 'fanouts': fan, 'temporal_csc_build_ms': round(build_ms, 1)})
    n_b = args.warmup + args.batches
    pool = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(11))
    pool = pool[:n_b * args.batch].clone()

    # -- whole batches, alternating ------------------------------------------------------------
    ms = {'disjoint_uniform': [], 'temporal_uniform': [], 'temporal_last': []}
    for i in range(n_b):
        seeds = pool[i * args.batch:(i + 1) * args.batch]
        for name, smp in (('disjoint_uniform', sd), ('temporal_uniform', st),
                          ('temporal_last', sl)):
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

    # -- the window kernel alone, on the frontiers of one temporal batch --------------------------
    seeds = pool[:args.batch]
    out = st.sample_from_nodes(seeds, seed=1)
    seed_time = st.seed_time(seeds.to(st.colptr.dtype))
    torch.cuda.synchronize(dev)
    base = 0
    for hop, k in enumerate(fan):
        n_f = out.num_sampled_nodes[hop]
        frontier = out.node[base:base + n_f].contiguous()
        ftime = seed_time[out.batch[base:base + n_f].long()].contiguous()
        base += n_f
        f = frontier.long()
        deg = (st.colptr[f + 1] - st.colptr[f]).double()
        rounds = torch.where(deg > 1, torch.ceil(torch.log(deg.clamp(min=1)) / math.log(64)),
                             torch.ones_like(deg))
        probes = int(torch.where(deg <= 64, deg, 64 * rounds).sum())
        nbytes = n_f * (3 * idx_b + 8 + 3 * idx_b) + probes * (idx_b + 8)
        res = {'what': 'window', 'hop': hop, 'k': k, 'frontier': n_f, 'probes': probes,
               'max_deg': int(deg.max()) if n_f else 0}

        def launch_window():
            _native.sample_temporal_window(st.colptr, st.row, st.time, frontier, ftime, k)

        def launch_counts():
            _native.sample_counts(st.colptr, frontier, k)
        for name, fn in (('window', launch_window), ('counts', launch_counts)):
            fn()
            res[f'{name}_ms'] = round(timed(fn, args.reps, dev), 5)
        res['window_bytes'] = nbytes
        res['window_GBps'] = round(nbytes / res['window_ms'] / 1e6, 1)
        emit(res)

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
