"""Heterogeneous neighbour sampling on a synthetic ogbn-mag-like graph generated on the device:
paper 736,389, author 1,134,649, institution 8,740, field 59,965 nodes; cites 5.4 M, writes 7.1 M,
affiliated_with 1.0 M, has_topic 7.5 M edges plus the three ``rev_`` types (uniform random
endpoints); ``input_nodes='paper'``, batch 1024, ``[10, 10]`` for every edge type.

Prints JSON lines:
  graph  — the shape and the CSC build time;
  batch  — ``HeteroNeighborSampler.sample_from_nodes`` per batch, non-disjoint and disjoint
           (device events around each batch after warm-up; median / min over the timed batches),
           with the sampled nodes and edges of the last batch.
``--temporal node|edge`` adds a pair of lines measured in ONE loop that alternates a non-temporal
``disjoint=True`` batch and a temporal batch on the same seeds: seeded random integer times in
[0, 1000) on the papers and authors (``node``: institutions and fields carry none, so their
out-edges are untimed; seed time = the seed paper's) or on every edge (``edge``: seed times drawn
in [0, 1000)), with the temporal CSC build time (two sorts) next to the plain one (both after a
warm-up build).
``--forward-only`` keeps the four forward edge types (the launch count per hop does not depend on
the number of edge types: compare the kernel traces of the two runs).
Usage: python scripts/time_hetero_sampling.py [--batches 20] [--warmup 3] [--forward-only]
       [--mode both|plain|disjoint|none] [--temporal node|edge] [--strategy uniform|last]
       [--out FILE]"""
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


def timed_build(dev, **kw):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    smp = HeteroNeighborSampler(**kw)
    torch.cuda.synchronize(dev)
    return smp, (time.perf_counter() - t0) * 1e3


def temporal_pair(args, eid, dev, emit):
    """The non-temporal disjoint sampler and the temporal one, alternated batch by batch."""
    g = torch.Generator(device=dev).manual_seed(7)
    kw, seed_time = {}, None
    if args.temporal == 'node':
        kw['node_time'] = {t: torch.randint(0, 1000, (NODES[t], ), generator=g, device=dev)
                           for t in ('paper', 'author')}
    else:
        kw['edge_time'] = {et: torch.randint(0, 1000, (ei.size(1), ), generator=g, device=dev)
                           for et, ei in eid.items()}
    common = dict(edge_index_dict=eid, num_nodes_dict=NODES, num_neighbors=[10, 10], seed=1)
    timed_build(dev, disjoint=True, **common)   # warm-up: the first build pays the allocations
    plain, plain_ms = timed_build(dev, disjoint=True, **common)
    temp, temp_ms = timed_build(dev, temporal_strategy=args.strategy, **kw, **common)
    emit({'kind': 'graph', 'temporal': args.temporal, 'edge_types': len(eid),
          'edges': sum(v.size(1) for v in eid.values()), 'csc_build_ms': round(plain_ms, 1),
          'csc_build_temporal_ms': round(temp_ms, 1)})
    gen = torch.Generator().manual_seed(5)
    ms = {'disjoint': [], 'temporal': []}
    outs = {}
    for b in range(args.warmup + args.batches):
        seeds = torch.randperm(NODES['paper'], generator=gen)[:args.batch].to(dev)
        if args.temporal == 'edge':
            seed_time = torch.randint(0, 1000, (args.batch, ), generator=gen).to(dev)
        for name, smp in (('disjoint', plain), ('temporal', temp)):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if name == 'temporal':
                outs[name] = smp.sample_from_nodes(('paper', seeds), time=seed_time)
            else:
                outs[name] = smp.sample_from_nodes(('paper', seeds))
            z.record()
            torch.cuda.synchronize(dev)
            if b >= args.warmup:
                ms[name].append(a.elapsed_time(z))
    for name, out in outs.items():
        emit({'kind': 'batch', 'disjoint': True, 'alternated': True,
              'temporal': args.temporal if name == 'temporal' else None,
              'strategy': args.strategy if name == 'temporal' else None,
              'forward_only': args.forward_only, 'edge_types': len(eid), 'batches': args.batches,
              'ms_median': round(statistics.median(ms[name]), 3),
              'ms_min': round(min(ms[name]), 3),
              'nodes': {t: sum(v) for t, v in out.num_sampled_nodes.items()},
              'edges': sum(sum(v) for v in out.num_sampled_edges.values())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--forward-only', action='store_true')
    ap.add_argument('--mode', default='both', choices=['both', 'plain', 'disjoint', 'none'])
    ap.add_argument('--temporal', default=None, choices=['node', 'edge'])
    ap.add_argument('--strategy', default='uniform', choices=['uniform', 'last'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    eid = graph(dev, args.forward_only)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    modes = {'both': [False, True], 'none': []}.get(args.mode, [args.mode == 'disjoint'])
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
    if args.temporal:
        temporal_pair(args, eid, dev, emit)
    if args.out:
        with open(args.out, 'w') as f:
            for d in lines:
                f.write(json.dumps(d) + '\n')


if __name__ == '__main__':
    main()
