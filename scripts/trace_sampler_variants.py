"""Launches and synchronising calls of ONE batch of every sampler variant (homogeneous: bounded,
``-1``, disjoint, temporal uniform / last, weighted, link-level; heterogeneous: plain, disjoint,
node- and edge-level temporal, link-level), to compare two builds of the package.

    rocprofv3 --kernel-trace --stats -d OUT -o trace --output-format csv -- \\
        python scripts/trace_sampler_variants.py OUT
    python scripts/trace_sampler_variants.py --summarize OUT
    python scripts/trace_sampler_variants.py --syncs OUT

The first form runs every variant twice (the first pass warms up), each batch between two MARKER
launches (``torch.lgamma`` on one element: no sampler path uses it); ``--summarize`` cuts the kernel
trace at the markers and prints the launches per variant with the sampler's own kernels by name.
``--syncs`` counts the synchronising torch calls of a batch (``torch.cuda.set_sync_debug_mode``).
The package is imported from the CURRENT WORKING DIRECTORY, so the same file measures another
checkout: run it from that checkout's root.  Graphs: 200k nodes / 2M random edges; 200k users, 50k
items, 'rates' (2M), 'rev_rates', 'follows' (1M); batch 512, fan-out [10, 5]."""
import csv
import glob
import json
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.getcwd())
MARKER = 'lgamma'


def variants(dev):
    import torch
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler, NeighborSampler
    g = torch.Generator().manual_seed(0)
    N, E, B = 200_000, 2_000_000, 512
    ei = torch.stack([torch.randint(0, N, (E, ), generator=g),
                      torch.randint(0, N, (E, ), generator=g)]).to(dev)
    w = torch.rand(E, generator=g).to(dev)
    nt = torch.randint(0, 1000, (N, ), generator=g).to(dev)
    seeds = torch.randperm(N, generator=g)[:B].to(dev)
    fan = [10, 5]
    pos = ei[:, torch.randint(0, E, (B, ), generator=g).to(dev)]
    ltime = torch.randint(500, 1000, (B, ), generator=g).to(dev)
    S = NeighborSampler
    plain, allk = S(ei, N, fan, seed=1), S(ei, N, [-1, -1], seed=1)
    disj = S(ei, N, fan, seed=1, disjoint=True)
    tu = S(ei, N, fan, seed=1, node_time=nt)
    tl = S(ei, N, fan, seed=1, node_time=nt, temporal_strategy='last')
    wt = S(ei, N, fan, seed=1, edge_weight=w)
    run = {
        'homo_plain': lambda: plain.sample_from_nodes(seeds, seed=3),
        'homo_all': lambda: allk.sample_from_nodes(seeds[:32], seed=3),
        'homo_disjoint': lambda: disj.sample_from_nodes(seeds, seed=3),
        'homo_temporal_uniform': lambda: tu.sample_from_nodes(seeds, seed=3),
        'homo_temporal_last': lambda: tl.sample_from_nodes(seeds, seed=3),
        'homo_weighted': lambda: wt.sample_from_nodes(seeds, seed=3),
        'homo_link_binary': lambda: plain.sample_from_edges(pos, 'binary', seed=3),
        'homo_link_triplet_disjoint': lambda: disj.sample_from_edges(pos, 'triplet', seed=3),
        'homo_link_binary_temporal': lambda: tu.sample_from_edges(
            SimpleNamespace(row=pos[0], col=pos[1], time=ltime), 'binary', seed=3),
    }
    nn = {'user': 200_000, 'item': 50_000}
    R, V, F = ('user', 'rates', 'item'), ('item', 'rev_rates', 'user'), ('user', 'follows', 'user')

    def hei(ns, nd, m):
        return torch.stack([torch.randint(0, ns, (m, ), generator=g),
                            torch.randint(0, nd, (m, ), generator=g)]).to(dev)
    eid = {R: hei(nn['user'], nn['item'], 2_000_000), V: None, F: hei(nn['user'], nn['user'], 1_000_000)}
    eid[V] = eid[R].flip(0).contiguous()
    ut = torch.randint(0, 1000, (nn['user'], ), generator=g).to(dev)
    et = {k: torch.randint(0, 1000, (v.size(1), ), generator=g).to(dev) for k, v in eid.items()}
    H = HeteroNeighborSampler
    hp, hd = H(eid, nn, fan, seed=1), H(eid, nn, fan, seed=1, disjoint=True)
    hn, he = H(eid, nn, fan, seed=1, node_time={'user': ut}), H(eid, nn, fan, seed=1, edge_time=et)
    hseeds = torch.randperm(nn['user'], generator=g)[:B].to(dev)
    htime = torch.randint(500, 1000, (B, ), generator=g).to(dev)
    hpos = {k: eid[k][:, torch.randint(0, eid[k].size(1), (B, ), generator=g).to(dev)]
            for k in (R, F)}

    def link(smp, k, neg, t=None):
        inp = SimpleNamespace(row=hpos[k][0], col=hpos[k][1], input_type=k, time=t)
        return lambda: smp.sample_from_edges(inp, neg, seed=3)
    run.update({
        'hetero_plain': lambda: hp.sample_from_nodes(('user', hseeds), seed=3),
        'hetero_disjoint': lambda: hd.sample_from_nodes(('user', hseeds), seed=3),
        'hetero_temporal_node': lambda: hn.sample_from_nodes(('user', hseeds), seed=3),
        'hetero_temporal_edge': lambda: he.sample_from_nodes(('user', hseeds), seed=3, time=htime),
        'hetero_link_none': link(hp, R, None),
        'hetero_link_binary': link(hp, R, 'binary'),
        'hetero_link_triplet': link(hp, R, 'triplet'),
        'hetero_link_binary_disjoint': link(hd, R, 'binary'),
        'hetero_link_triplet_disjoint': link(hd, R, 'triplet'),
        'hetero_link_binary_temporal': link(hn, R, 'binary', htime),
        'hetero_link_binary_one_type': link(hp, F, 'binary'),
    })
    return run


def short(name):
    return name.split('(')[0].replace('void ', '').split('<')[0].split('::')[-1][:48]


def summarize(d, keys):
    kfile = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    rows = sorted((int(r['Start_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(kfile[0])))
    cuts = [i for i, (_, n) in enumerate(rows) if MARKER in n]
    out = {'markers': len(cuts), 'kernels': len(rows)}
    # two passes of (marker, batch, marker) per variant: 4 * len(keys) markers; read pass 2
    if len(cuts) != 4 * len(keys):
        out['error'] = 'unexpected number of markers'
        return out
    for j, k in enumerate(keys):
        a, b = cuts[2 * len(keys) + 2 * j], cuts[2 * len(keys) + 2 * j + 1]
        seg = [short(n) for _, n in rows[a + 1:b]]
        own = {}
        for n in seg:
            if n.startswith(('hetero_', 'sample_', 'unique_', 'relabel_')):
                own[n] = own.get(n, 0) + 1
        out[k] = {'launches': len(seg), 'own': own}
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--summarize':
        keys = json.load(open(os.path.join(sys.argv[2], 'keys.json')))
        res = summarize(sys.argv[2], keys)
        json.dump(res, open(os.path.join(sys.argv[2], 'summary.json'), 'w'), indent=1)
        for k in keys:
            print(k, json.dumps(res.get(k)))
        print({k: v for k, v in res.items() if k not in keys})
        return
    import torch
    dev = torch.device('cuda:0')
    run = variants(dev)
    keys = list(run)
    if sys.argv[1] == '--syncs':  # synchronising torch calls per batch (torch's sync debug mode)
        import warnings
        res = {}
        for k in keys:
            run[k]()
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode('warn')
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter('always')
                run[k]()
            torch.cuda.set_sync_debug_mode('default')
            torch.cuda.synchronize()
            res[k] = sum(1 for x in w if 'synchroniz' in str(x.message).lower())
        print(json.dumps(res))
        os.makedirs(sys.argv[2], exist_ok=True)
        json.dump(res, open(os.path.join(sys.argv[2], 'syncs.json'), 'w'), indent=1)
        return
    os.makedirs(sys.argv[1], exist_ok=True)
    json.dump(keys, open(os.path.join(sys.argv[1], 'keys.json'), 'w'))
    one = torch.ones(1, device=dev)
    for _ in range(2):
        for k in keys:
            torch.lgamma(one)
            torch.cuda.synchronize()
            run[k]()
            torch.cuda.synchronize()
            torch.lgamma(one)
            torch.cuda.synchronize()
    print('traced', len(keys))


if __name__ == '__main__':
    main()
