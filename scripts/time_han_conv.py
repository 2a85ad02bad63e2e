"""One training step of ``nn.HANConv`` models, fused against generic, at three shapes: milliseconds
per step (device events) and the three attention kernels' achieved bytes per second.

    python scripts/time_han_conv.py [--shape batch|full|many] [--steps 50 --warmup 5 --repeats 2]
    rocprofv3 --kernel-trace --stats -d OUT -o trace --output-format csv -- \\
        python scripts/time_han_conv.py --shape full --trace

Shapes:

* ``batch``: the sampled user-item batch of scripts/time_hetero_conv.py (200k users, 50k items,
  'rates' 2M, 'rev_rates' 2M, 'follows' 1M; 1,024 user seeds, fan-out [10, 10]); 2 layers, 128
  wide, 8 heads; fresh copies of the batch's ``edge_index`` tensors every step, so that a step pays
  for its stacked handle as a step on a new batch does;
* ``full``: a full typed graph, 3 node types x 500,000 nodes, 6 edge types x 5,000,000 edges; 1
  layer, 256 wide, 8 heads; the handle is cached after the first step;
* ``many``: 8 node types x 4,000 nodes, 16 edge types x 40,000 edges (the launch-count regime); 2
  layers, 128 wide, 8 heads; fresh ``edge_index`` copies every step.

A step is forward, cross-entropy on the first 1,024 rows of the first node type, backward (no
optimizer step).  Both routes use the SAME parameter objects in one process and ALTERNATE step by
step; every shape is measured ``--repeats`` times to show the spread.  The kernels' times are the
device events of ``_native.timing_sink`` around each ``pygamd_han_*`` call (the merge launches of
long rows included); their bytes are the algorithmic ones, computed from the shapes below.
``--trace`` warms up and then runs three fused steps, for a profiler to read."""
import argparse
import json
import sys
from os import path as osp

import torch
import torch.nn.functional as F

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
sys.path.insert(0, osp.dirname(osp.abspath(__file__)))

SEEDS, CLASSES = 1024, 128
PEAK_HBM = 8.0e12   # bytes per second, MI355X


def _random_typed(dev, n_types, n_nodes, n_ets, n_edges, width, dst_step, seed=0):
    g = torch.Generator().manual_seed(seed)
    types = [f'n{i}' for i in range(n_types)]
    # edge type k: node type k -> node type dst_step * k + 1 (mod the number of node types)
    ets = [(types[k % n_types], f'r{k}', types[(k * dst_step + 1) % n_types])
           for k in range(n_ets)]
    x = {t: torch.randn(n_nodes, width, generator=g).to(dev) for t in types}
    ei = {et: torch.stack([torch.randint(0, n_nodes, (n_edges, ), generator=g),
                           torch.randint(0, n_nodes, (n_edges, ), generator=g)]).to(dev)
          for et in ets}
    y = torch.randint(0, CLASSES, (SEEDS, ), generator=g).to(dev)
    return x, ei, y, (types, ets)


def shape(name, dev):
    """(x_dict, edge_index_dict, target, layers, seed type, fresh edge tensors per step)"""
    from pytorch_geometric_amd.nn import HANConv
    torch.manual_seed(0)
    if name == 'batch':
        from time_hetero_conv import ETS, WIDTHS, build
        from pytorch_geometric_amd.loader import HeteroNeighborLoader
        x, eid, y = build(dev)
        loader = HeteroNeighborLoader(x, eid, [10, 10], 'user', batch_size=SEEDS, y=y, seed=1)
        batch = next(iter(loader))
        meta = (list(WIDTHS), ETS)
        layers = [HANConv(WIDTHS, 128, meta, heads=8), HANConv(128, 128, meta, heads=8)]
        return batch.x_dict, batch.edge_index_dict, batch.y[:SEEDS].long(), layers, 'user', True
    if name == 'full':
        x, ei, y, meta = _random_typed(dev, 3, 500_000, 6, 5_000_000, 256, 1)
        return x, ei, y, [HANConv(256, 256, meta, heads=8)], 'n0', False
    x, ei, y, meta = _random_typed(dev, 8, 4_000, 16, 40_000, 128, 3)
    return x, ei, y, [HANConv(128, 128, meta, heads=8), HANConv(128, 128, meta, heads=8)], 'n0', \
        True


def kernel_bytes(x, ei, layer):
    """The algorithmic bytes of the three launches of one layer step, from the shapes alone: every
    slot gathers one row and its logits once, every edge-sized tensor is written or read once."""
    W, H = layer.out_channels, layer.heads
    ets = list(ei)
    E = sum(int(v.size(1)) for v in ei.values())
    idx = next(iter(ei.values())).element_size()
    R = sum(int(x[et[-1]].size(0)) for et in ets)       # stacked (edge type, destination) rows
    C = sum(int(x[et[0]].size(0)) for et in ets)        # stacked (edge type, source) columns
    f = 4
    return {
        # x row + a_src + col per slot, alpha written; a_dst read and out written per row
        'forward': E * (W * f + H * f + idx) + E * H * f + R * (W + H) * f + R * idx,
        # x row + a_src + alpha + col per slot, grad_s written; grad_out, out, a_dst read and
        # grad_a_dst written per row
        'backward_dst': E * (W * f + 2 * H * f + idx) + E * H * f + R * (2 * W + 2 * H) * f
        + R * idx,
        # grad_out and out rows + alpha + grad_s + col + slot map per slot; grad_xv and grad_a_src
        # written per column
        'backward_src': E * (2 * W * f + 2 * H * f + 2 * idx) + C * (W + H) * f + C * idx,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='all', choices=['all', 'batch', 'full', 'many'])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--trace', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this script needs a GPU'
    from pytorch_geometric_amd import _native
    dev = torch.device('cuda:0')
    for name in (['batch', 'full', 'many'] if args.shape == 'all' else [args.shape]):
        x, ei, target, layers, seed_type, fresh = shape(name, dev)
        layers = torch.nn.ModuleList(layers).to(dev)

        def run(fuse):
            for p in layers.parameters():
                p.grad = None
            e = {et: v.clone() for et, v in ei.items()} if fresh else ei
            h = x
            for layer in layers:
                layer.fuse = fuse
                h = layer(h, e)
            loss = F.cross_entropy(h[seed_type][:SEEDS], target)
            loss.backward()
            return loss

        E = sum(int(v.size(1)) for v in ei.values())
        print(json.dumps({'what': 'shape', 'shape': name, 'layers': len(layers),
                          'width': layers[0].out_channels, 'heads': layers[0].heads,
                          'nodes': {t: int(v.size(0)) for t, v in x.items()},
                          'edge_types': len(ei), 'edges': E}), flush=True)
        print(json.dumps({'what': 'loss', 'shape': name, 'fused': round(float(run(True).detach()), 6),
                          'generic': round(float(run(False).detach()), 6)}), flush=True)
        if args.trace:
            for _ in range(3):
                run(True)
            torch.cuda.synchronize()
            print(json.dumps({'what': 'trace_run', 'shape': name, 'fused_steps': 3}))
            continue
        for rep in range(args.repeats):
            for _ in range(args.warmup):
                run(True)
                run(False)
            ms = {True: [], False: []}
            for _ in range(args.steps):
                for fuse in (True, False):          # alternating
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    run(fuse)
                    b.record()
                    ms[fuse].append((a, b))
            torch.cuda.synchronize()
            rec = {'what': 'step', 'shape': name, 'repeat': rep, 'n': args.steps}
            for fuse, key in ((True, 'fused'), (False, 'generic')):
                t = sorted(a.elapsed_time(b) for a, b in ms[fuse])
                rec[f'{key}_median_ms'] = round(t[len(t) // 2], 4)
                rec[f'{key}_min_ms'] = round(t[0], 4)
            rec['generic_over_fused'] = round(rec['generic_median_ms'] / rec['fused_median_ms'], 3)
            print(json.dumps(rec), flush=True)
        # the kernels of the LAST layer (whose input width is the hidden width), fused steps alone
        sink = []
        _native.timing_sink = sink
        try:
            for _ in range(min(args.steps, 20)):
                run(True)
            torch.cuda.synchronize()
        finally:
            _native.timing_sink = None
        nbytes = kernel_bytes(x, ei, layers[-1])
        for op in ('forward', 'backward_dst', 'backward_src'):
            t = sorted(a.elapsed_time(b) for i, a, b in sink
                       if i.get('kind') == 'han' and i.get('op') == op)
            if not t:
                continue
            med = t[len(t) // 2]
            rate = nbytes[op] / (med * 1e-3)
            print(json.dumps({'what': 'kernel', 'shape': name, 'op': op, 'launches': len(t),
                              'median_ms': round(med, 4), 'min_ms': round(t[0], 4),
                              'algorithmic_bytes': nbytes[op],
                              'GB_per_s_at_median': round(rate / 1e9, 1),
                              'share_of_peak_hbm': round(rate / PEAK_HBM, 3)}), flush=True)


if __name__ == '__main__':
    main()
