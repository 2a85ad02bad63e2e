"""Heterogeneous link-level sampling on a user-item graph: milliseconds per batch (device events)
and, under ``rocprofv3 --kernel-trace --stats``, the launches of one batch of every variant.

    python scripts/time_hetero_link_sampling.py [--batches 50 --warmup 5]
    rocprofv3 --kernel-trace --stats -d OUT -o trace --output-format csv -- \\
        python scripts/time_hetero_link_sampling.py --trace
    python scripts/time_hetero_link_sampling.py --summarize OUT/trace_kernel_trace.csv

``--trace`` runs every variant once to warm up, then one batch of each between two MARKER launches
(``torch.lgamma`` on one element: no sampler path uses it); ``--summarize`` cuts the trace at the
markers.  The two ``seed_block_*`` variants are the seed block alone: the one-launch kernel
(``pygamd_hetero_link_seeds``) and the same block composed from ``pygamd_sample_negatives`` and
tensor operations.  Graph: 200k users, 50k items, 'rates' (2M), 'rev_rates' (2M), 'follows' (1M);
batch 1024 links, fan-out [10, 10], int64."""
import argparse
import csv
import json
import sys
from os import path as osp
from types import SimpleNamespace

import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

RATES, REV, FOLLOWS = ('user', 'rates', 'item'), ('item', 'rev_rates', 'user'), \
    ('user', 'follows', 'user')
MARKER = 'lgamma'


def build(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    nn = {'user': 200_000, 'item': 50_000}

    def ei(ns, nd, m):
        return torch.stack([torch.randint(0, ns, (m, ), generator=g),
                            torch.randint(0, nd, (m, ), generator=g)]).to(dev)
    eid = {RATES: ei(nn['user'], nn['item'], 2_000_000), REV: None,
           FOLLOWS: ei(nn['user'], nn['user'], 1_000_000)}
    eid[REV] = eid[RATES].flip(0).contiguous()
    user_time = torch.randint(0, 1000, (nn['user'], ), generator=g).to(dev)
    return eid, nn, user_time


def variants(dev, batch=1024):
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler
    eid, nn, user_time = build(dev)
    fan = [10, 10]
    plain = HeteroNeighborSampler(eid, nn, fan, seed=1)
    disjoint = HeteroNeighborSampler(eid, nn, fan, seed=1, disjoint=True)
    temporal = HeteroNeighborSampler(eid, nn, fan, seed=1, node_time={'user': user_time})
    g = torch.Generator().manual_seed(7)
    pos = {et: eid[et][:, torch.randint(0, eid[et].size(1), (batch, ), generator=g).to(dev)]
           for et in (RATES, FOLLOWS)}
    time = torch.randint(500, 1000, (batch, ), generator=g).to(dev)

    def link(smp, et, neg, t=None):
        inp = SimpleNamespace(row=pos[et][0], col=pos[et][1], input_type=et, time=t)
        return lambda: smp.sample_from_edges(inp, neg)

    ends = [dict(num_nodes=nn['user'], node_base=0),
            dict(num_nodes=nn['item'], node_base=nn['user'])]
    src, dst = pos[RATES][0], pos[RATES][1]

    def composed():   # the seed block of a binary batch without the kernel
        s = torch.cat([src, _native.sample_negatives(batch, nn['user'], 10, dev)])
        d = torch.cat([dst, _native.sample_negatives(batch, nn['item'], 11, dev)])
        return torch.cat([s, d + nn['user']]), time.repeat(2).repeat(2)

    return {
        'link_none': link(plain, RATES, None),
        'link_binary': link(plain, RATES, 'binary'),
        'link_triplet': link(plain, RATES, 'triplet'),
        'link_binary_disjoint': link(disjoint, RATES, 'binary'),
        'link_binary_temporal': link(temporal, RATES, 'binary', time),
        'link_binary_one_type': link(plain, FOLLOWS, 'binary'),
        'nodes_2048_users': lambda: plain.sample_from_nodes(('user', torch.cat([src, src]))),
        'seed_block_kernel': lambda: _native.hetero_link_seeds(src, dst, batch, 'binary', 5, ends,
                                                               link_time=time),
        'seed_block_composed': composed,
    }


def summarize(src):
    """The kernel names between consecutive markers, in launch order."""
    rows = sorted(((int(r['Start_Timestamp']), r['Kernel_Name']) for r in
                   csv.DictReader(open(src))))
    names = [n for _, n in rows]
    cuts = [i for i, n in enumerate(names) if MARKER in n]
    print(json.dumps({'what': 'trace', 'kernels': len(names), 'markers': len(cuts)}))
    return [names[a + 1:b] for a, b in zip(cuts[:-1], cuts[1:])], names


def short(name):
    return name.split('(')[0].replace('void ', '').split('<')[0].split('::')[-1][:48]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    keys = ['link_none', 'link_binary', 'link_triplet', 'link_binary_disjoint',
            'link_binary_temporal', 'link_binary_one_type', 'nodes_2048_users',
            'seed_block_kernel', 'seed_block_composed']
    if args.summarize:
        segs, names = summarize(args.summarize)
        # every variant sits between two markers of its own, in two passes: the segments of the
        # second pass (the first one warms up) are the last 2 * len(keys) - 1, every other one
        if len(segs) != 4 * len(keys) - 1:
            print(json.dumps({'what': 'unexpected_markers', 'distinct_kernels':
                              sorted({short(n) for n in names})}))
            return
        segs = segs[-(2 * len(keys) - 1)::2]
        for k, seg in zip(keys, segs):
            count = {}
            for n in seg:
                count[short(n)] = count.get(short(n), 0) + 1
            rec = {'what': 'launches', 'variant': k, 'launches': len(seg)}
            if k.startswith('seed_block'):
                rec['kernels'] = count
            else:
                rec['sampling_kernels'] = {n: c for n, c in count.items()
                                           if n.startswith(('hetero_', 'sample_', 'unique_'))}
            print(json.dumps(rec))
        return
    assert torch.cuda.is_available(), 'this script needs a GPU'
    dev = torch.device('cuda:0')
    run = variants(dev)
    assert list(run) == keys
    one = torch.ones(1, device=dev)
    if args.trace:
        for _ in range(2):          # pass 1 warms up, pass 2 is the one that is read
            for k in keys:
                torch.lgamma(one)
                torch.cuda.synchronize()
                run[k]()
                torch.cuda.synchronize()
                torch.lgamma(one)
                torch.cuda.synchronize()
        print(json.dumps({'what': 'trace_run', 'variants': keys}))
        return
    for k in keys:
        for _ in range(args.warmup):
            run[k]()
        ms = []
        for _ in range(args.batches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run[k]()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        print(json.dumps({'what': 'batch', 'variant': k, 'median_ms': round(ms[len(ms) // 2], 4),
                          'min_ms': round(ms[0], 4), 'n': len(ms)}))


if __name__ == '__main__':
    main()
