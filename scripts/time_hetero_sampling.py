"""Heterogeneous neighbour sampling on a synthetic ogbn-mag-like graph generated on the device:
paper 736,389, author 1,134,649, institution 8,740, field 59,965 nodes; cites 5.4 M, writes 7.1 M,
affiliated_with 1.0 M, has_topic 7.5 M edges plus the three ``rev_`` types (uniform random
endpoints); ``input_nodes='paper'``, batch 1024, ``[10, 10]`` for every edge type.

Prints JSON lines:
  graph  — the shape and the CSC build time;
  batch  — ``HeteroNeighborSampler.sample_from_nodes`` per batch, non-disjoint and disjoint
           (device events around each batch after warm-up; median / min over the timed batches),
           with the sampled nodes and edges of the last batch.
``--forward-only`` keeps the four forward edge types (the launch count per hop does not depend on
the number of edge types: compare the kernel traces of the two runs).
Usage: python scripts/time_hetero_sampling.py [--batches 20] [--warmup 3] [--forward-only]
       [--mode both|plain|disjoint] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_geometric_amd.sampler import HeteroNeighborSampler  # noqa: E402

NODES = {'paper': 736_389, 'author': 1_134_649, 'institution': 8_740, 'field_of_study': 59_965}
EDGES = [('paper', 'cites', 'paper', 5_416_271), ('author', 'writes', 'paper', 7_145_660),
         ('author', 'affiliated_with', 'institution', 1_043_998),
         ('paper', 'has_topic', 'field_of_study', 7_505_078)]


def graph(dev, forward_only: bool):
    g = torch.Generator(device=dev).manual_seed(0)
    eid = {}
    for s, r, d, m in EDGES:
        src = torch.randint(0, NODES[s], (m, ), generator=g, device=dev)
        dst = torch.randint(0, NODES[d], (m, ), generator=g, device=dev)
        eid[(s, r, d)] = torch.stack([src, dst])
    if not forward_only:  # the three rev_ types of ogbn-mag (cites stays one type)
        for s, r, d, _ in EDGES[1:]:
            eid[(d, 'rev_' + r, s)] = eid[(s, r, d)].flip(0)
    return eid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--forward-only', action='store_true')
    ap.add_argument('--mode', default='both', choices=['both', 'plain', 'disjoint'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    eid = graph(dev, args.forward_only)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    modes = [False, True] if args.mode == 'both' else [args.mode == 'disjoint']
    for disjoint in modes:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        smp = HeteroNeighborSampler(eid, NODES, [10, 10], seed=1, disjoint=disjoint)
        torch.cuda.synchronize(dev)
        build_ms = (time.perf_counter() - t0) * 1e3
        if disjoint == modes[0]:
            emit({'kind': 'graph', 'node_types': len(NODES), 'edge_types': len(eid),
                  'nodes': sum(NODES.values()), 'edges': sum(v.size(1) for v in eid.values()),
                  'csc_build_ms': round(build_ms, 1)})
        gen = torch.Generator().manual_seed(5)
        ms, out = [], None
        for b in range(args.warmup + args.batches):
            seeds = torch.randperm(NODES['paper'], generator=gen)[:args.batch].to(dev)
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = smp.sample_from_nodes(('paper', seeds))
            z.record()
            torch.cuda.synchronize(dev)
            if b >= args.warmup:
                ms.append(a.elapsed_time(z))
        emit({'kind': 'batch', 'disjoint': disjoint, 'forward_only': args.forward_only,
              'edge_types': len(eid), 'batches': args.batches,
              'ms_median': round(statistics.median(ms), 3), 'ms_min': round(min(ms), 3),
              'nodes': {t: sum(v) for t, v in out.num_sampled_nodes.items()},
              'edges': sum(sum(v) for v in out.num_sampled_edges.values())})
        del smp
    if args.out:
        with open(args.out, 'w') as f:
            for d in lines:
                f.write(json.dumps(d) + '\n')


if __name__ == '__main__':
    main()
