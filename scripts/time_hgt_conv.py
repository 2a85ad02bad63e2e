"""One training step of a 2-layer Heterogeneous Graph Transformer on a sampled user-item batch:
milliseconds per step (device events), the relation-transform kernel's achieved bytes per second
and, under ``rocprofv3 --kernel-trace --stats``, the launches of one step of both routes.

    python scripts/time_hgt_conv.py [--steps 50 --warmup 5]
    rocprofv3 --kernel-trace --stats -d OUT -o trace --output-format csv -- \\
        python scripts/time_hgt_conv.py --trace
    python scripts/time_hgt_conv.py --summarize OUT/trace_kernel_trace.csv

Graph and batch are those of scripts/time_hetero_conv.py (profiles/hetero_conv.md): 200k users,
50k items, 'rates' (2M), 'rev_rates' (2M), 'follows' (1M); 1,024 user seeds, fan-out [10, 10].  The
model: 2 x ``nn.HGTConv`` (128 wide, 4 heads), cross-entropy on the seed rows, backward (no
optimizer step), on fresh copies of the batch's ``edge_index`` tensors, so that every step pays for
its stacked handle as a step on a new batch does.  Two routes with the SAME parameter objects in
one process: ``fused`` (csrc/hgt.hip + csrc/transformer.hip) and ``generic`` (``fuse = False``:
the reference's formulation over HeteroLinear, softmax and propagate).
``--trace`` runs both once to warm up, then one step of each between two MARKER launches
(``torch.lgamma`` on one element); ``--summarize`` cuts the trace at the markers."""
import argparse
import json
import sys
from os import path as osp

import torch
import torch.nn.functional as F

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
sys.path.insert(0, osp.dirname(osp.abspath(__file__)))

from time_hetero_conv import ETS, SEEDS, WIDTHS, build, short, summarize  # noqa: E402

HIDDEN, HEADS = 128, 4


def variants(dev):
    from pytorch_geometric_amd.loader import HeteroNeighborLoader
    from pytorch_geometric_amd.nn import HGTConv
    x, eid, y = build(dev)
    loader = HeteroNeighborLoader(x, eid, [10, 10], 'user', batch_size=SEEDS, y=y, seed=1)
    batch = next(iter(loader))
    target = batch.y[:SEEDS].long()
    torch.manual_seed(0)
    meta = (list(WIDTHS), ETS)
    layers = torch.nn.ModuleList([HGTConv(WIDTHS, HIDDEN, meta, heads=HEADS),
                                  HGTConv(HIDDEN, HIDDEN, meta, heads=HEADS)]).to(dev)

    def step(fuse):
        def run():
            for p in layers.parameters():
                p.grad = None
            ei = {et: v.clone() for et, v in batch.edge_index_dict.items()}
            h = batch.x_dict
            for layer in layers:
                layer.fuse = fuse
                h = layer(h, ei)
            loss = F.cross_entropy(h['user'][:SEEDS], target)
            loss.backward()
            return loss
        return run
    nodes = {t: int(v.size(0)) for t, v in batch.x_dict.items()}
    info = {'nodes': nodes,
            'edges': {'__'.join(et): int(v.size(1)) for et, v in batch.edge_index_dict.items()},
            # the relation kernel's algorithmic traffic: k and v of every source node type read
            # once, the packed table of the stacked source rows written once
            'relation_bytes': (sum(nodes[t] for t in {et[0] for et in ETS}) * HIDDEN * 4 * 2
                               + sum(nodes[et[0]] for et in ETS) * 2 * HIDDEN * 4)}
    return {'fused': step(True), 'generic': step(False)}, info


def relation_rate(run, info, steps):
    """Device-event time of the relation-transform launches of ``steps`` fused steps."""
    from pytorch_geometric_amd import _native
    sink = []
    _native.timing_sink = sink
    try:
        for _ in range(steps):
            run()
        torch.cuda.synchronize()
    finally:
        _native.timing_sink = None
    for op in ('relation_forward', 'relation_backward'):
        ms = sorted(a.elapsed_time(b) for i, a, b in sink
                    if i.get('kind') == 'hgt' and i.get('op') == op)
        if not ms:
            continue
        med = ms[len(ms) // 2]
        rec = {'what': 'relation_kernel', 'op': op, 'launches': len(ms),
               'median_ms': round(med, 4), 'min_ms': round(ms[0], 4)}
        if op == 'relation_forward':
            rec['algorithmic_bytes'] = info['relation_bytes']
            rec['GB_per_s_at_median'] = round(info['relation_bytes'] / med / 1e6, 1)
        print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    keys = ['fused', 'generic']
    if args.summarize:
        segs, names = summarize(args.summarize)
        if len(segs) != 4 * len(keys) - 1:
            print(json.dumps({'what': 'unexpected_markers', 'distinct_kernels':
                              sorted({short(n) for n in names})}))
            return
        segs = segs[-(2 * len(keys) - 1)::2]
        for k, seg in zip(keys, segs):
            count = {}
            for n in seg:
                count[short(n)] = count.get(short(n), 0) + 1
            top = dict(sorted(count.items(), key=lambda kv: -kv[1])[:14])
            own = {n: c for n, c in count.items() if n.startswith(('hgt_', 'transformer_'))}
            print(json.dumps({'what': 'launches', 'variant': k, 'launches': len(seg),
                              'hgt_and_attention_kernels': own, 'kernels': top}))
        return
    assert torch.cuda.is_available(), 'this script needs a GPU'
    dev = torch.device('cuda:0')
    run, info = variants(dev)
    print(json.dumps({'what': 'batch', **info}))
    losses = {k: float(run[k]()) for k in keys}
    print(json.dumps({'what': 'loss', **{k: round(v, 6) for k, v in losses.items()}}))
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
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run[k]()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        print(json.dumps({'what': 'step', 'variant': k, 'median_ms': round(ms[len(ms) // 2], 4),
                          'min_ms': round(ms[0], 4), 'n': len(ms)}))
    relation_rate(run['fused'], info, args.steps)


if __name__ == '__main__':
    main()
