"""Link-level sampling at the BASELINE config-4 shape (bench.py's mini-batch mode:
``powerlaw_undirected`` at the ogbn-papers100M shape, generated on the device; fan-outs
[15, 10, 5]) with 1024 positive edges per batch drawn from the graph.

Prints JSON lines:
  graph    — the shape;
  batch    — ``sample_from_edges`` per batch for no negatives / binary 1.0 / triplet 1, each
             non-disjoint and disjoint, and ``sample_from_nodes`` on the same deduplicated seeds
             (device events, after warm-up; median / min over the timed batches);
  kernels  — ``pygamd_sample_negatives`` (uniform, for the binary batch: 2 x 1024 draws) and the
             unique step (``index_sort`` + ``pygamd_unique_inverse`` on the 4096 seeds of a binary
             batch, host read included) alone, device events over repeated launches; the byte
             model of the negatives kernel is the 8-byte id written per draw, of the unique kernels
             the key reads, the 8-byte rank / inverse traffic and the writes (useful bytes).
Usage: python scripts/time_link_sampling.py [--scale 1.0] [--batches 20] [--reps 200]
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
from pytorch_geometric_amd.sampler import NegativeSampling, NeighborSampler  # noqa: E402


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
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    fan = [15, 10, 5]
    N = int(111_059_956 * args.scale)
    E = int(1_615_685_872 * args.scale) // 2 * 2
    B = args.batch
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    ei = powerlaw_undirected(N, E, seed=3, device=dev)
    n_b = args.warmup + args.batches
    pick = torch.randint(0, E, (n_b * B, ), device=dev,
                         generator=torch.Generator(device=dev).manual_seed(11))
    pos = ei[:, pick].clone()                      # [2, n_b * B] positive edges of the graph
    smp = NeighborSampler(ei, N, fan, seed=17)
    del ei
    sd = copy.copy(smp)                            # the same CSC as a disjoint sampler
    sd.disjoint = True
    torch.cuda.synchronize(dev)
    emit({'what': 'graph', 'N': N, 'E': E, 'scale': args.scale,
          'idx_bytes': smp.colptr.element_size(), 'batch': B, 'fanouts': fan})

    negs = {'none': None, 'binary_1': NegativeSampling('binary', 1.0),
            'triplet_1': NegativeSampling('triplet', 1)}
    ms = {}
    for i in range(n_b):
        edges = pos[:, i * B:(i + 1) * B]
        for disjoint, s in ((False, smp), (True, sd)):
            for name, neg in negs.items():
                key = f"edges_{name}_{'disjoint' if disjoint else 'shared'}"
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = s.sample_from_edges(edges, neg, seed=i)
                b.record()
                torch.cuda.synchronize(dev)
                if i >= args.warmup:
                    ms.setdefault(key, []).append(a.elapsed_time(b))
                if name == 'none' and not disjoint:  # the same deduplicated seeds, node-level
                    seeds = out.node[:out.num_sampled_nodes[0]].clone()
                    a.record()
                    s.sample_from_nodes(seeds, seed=i)
                    b.record()
                    torch.cuda.synchronize(dev)
                    if i >= args.warmup:
                        ms.setdefault('nodes_same_seeds_shared', []).append(a.elapsed_time(b))
    for name, v in ms.items():
        v = sorted(v)
        emit({'what': 'batch', 'sampler': name, 'median_ms': round(v[len(v) // 2], 4),
              'min_ms': round(v[0], 4), 'n': len(v)})

    # -- the link-specific kernels alone ---------------------------------------------------------
    dt = smp.colptr.dtype
    n_neg = 2 * B
    t_neg = timed(lambda: _native.sample_negatives(n_neg, N, 5, dev, dt), args.reps, dev)
    emit({'what': 'kernels', 'step': 'negatives_uniform', 'draws': n_neg,
          'ms': round(t_neg, 5), 'bytes': n_neg * smp.colptr.element_size()})
    edges = pos[:, :B]
    keys = torch.cat([edges[0], edges[1], _native.sample_negatives(n_neg, N, 5, dev, dt)])
    keys = keys.to(dt).contiguous()
    t_sort = timed(lambda: _native.index_sort(keys, max_value=N - 1), args.reps, dev)
    t_uni = timed(lambda: _native.unique_inverse(keys, max_value=N - 1), args.reps, dev)
    n = keys.numel()
    ib = keys.element_size()
    emit({'what': 'kernels', 'step': 'unique_inverse', 'keys': n,
          'index_sort_ms': round(t_sort, 5), 'total_ms': round(t_uni, 5),
          'after_sort_ms': round(t_uni - t_sort, 5),
          'after_sort_bytes': n * (2 * ib + 8) + n * (3 * 8) + n * (ib + 8 + 8)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            for d in lines:
                fh.write(json.dumps(d) + '\n')


if __name__ == '__main__':
    main()
