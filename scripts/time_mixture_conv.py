"""GMMConv and NNConv: the fused aggregate-first route (csrc/mixture.hip) against the generic route
of the same layer (``fuse = False``), forward + backward, on one device in one process — the
figures of profiles/mixture_conv.md.

    python scripts/time_mixture_conv.py [--out FILE] [--iters 20] [--warmup 5] [--shapes ...]

Shapes: a superpixel batch for GMMConv (4,800 nodes, 38,400 edges, 2 pseudo-coordinates, 25
kernels, in = out = 64); the node and edge counts of ogbn-arxiv (uniformly random edges) with 2
pseudo-coordinates, 8 kernels and in = out = 64; a QM9-like batch for NNConv (2,300 nodes, 4,800
edges, in = out = 64, the edge network ``Linear(5, 128)``, ``ReLU``, ``Linear(128, 4096)``).  Per
shape and route: ``torch.cuda.Event``s around one forward + backward (gradients of ``x``, of
``edge_attr`` and of every parameter), median over ``--iters`` calls after ``--warmup``, the two
routes alternated twice (both medians are printed); the peak memory above the inputs of one call;
for the fused route the time of its mixture launches from the records of ``_native.timing_sink``.
One JSON line per shape.  A route that runs out of memory is recorded as such, not skipped
silently."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_geometric_amd import _native, as_edge_index  # noqa: E402
from pytorch_geometric_amd.nn import GMMConv, NNConv  # noqa: E402

SHAPES = {
    'superpixels': dict(layer='gmm', N=4800, E=38400, channels=64, dim=2, kernel_size=25),
    'arxiv': dict(layer='gmm', N=169343, E=1166243, channels=64, dim=2, kernel_size=8),
    'qm9_like': dict(layer='nn', N=2300, E=4800, channels=64, dim=5, hidden=128),
}


def problem(shape, dev):
    g = torch.Generator().manual_seed(1)
    N, E, C = shape['N'], shape['E'], shape['channels']
    ei = torch.randint(0, N, (2, E), generator=g)
    torch.manual_seed(2)
    if shape['layer'] == 'gmm':
        conv = GMMConv(C, C, dim=shape['dim'], kernel_size=shape['kernel_size'])
        conv.sigma.data.uniform_(0.5, 1.5)       # (glorot draws sigma around 0: every weight 0)
    else:
        net = torch.nn.Sequential(torch.nn.Linear(shape['dim'], shape['hidden']), torch.nn.ReLU(),
                                  torch.nn.Linear(shape['hidden'], C * C))
        conv = NNConv(C, C, net, aggr='add')
    conv = conv.to(dev)
    x = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
    ea = torch.randn(E, shape['dim'], generator=g).to(dev).requires_grad_(True)
    graph = as_edge_index(ei.to(dev), N, N)
    graph.fill_cache_()
    graph.by_src()
    go = torch.randn(N, C, generator=g).to(dev)
    return conv, x, ea, graph, go


def step(conv, x, ea, graph, go):
    out = conv(x, graph, ea)
    params = [p for p in conv.parameters() if p.requires_grad]
    torch.autograd.grad(out, [x, ea] + params, go)
    return out


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def peak(conv, args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step(conv, *args)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def kernel_times(conv, args):
    sink = []
    _native.timing_sink = sink
    try:
        step(conv, *args)
        torch.cuda.synchronize()
    finally:
        _native.timing_sink = None
    return [[i['op'], i['n_rows'], i['F'], i['K'], round(a.elapsed_time(b), 4)]
            for i, a, b in sink if i.get('kind') == 'mixture']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--shapes', nargs='*', default=list(SHAPES))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs a GPU'
    dev = torch.device('cuda:0')
    for name in opt.shapes:
        conv, *args = problem(SHAPES[name], dev)
        rec = {'shape': name, **SHAPES[name], 'device': torch.cuda.get_device_name(0),
               'fused_ms': [], 'generic_ms': []}
        try:
            with torch.no_grad():
                conv.fuse = True
                a = conv(args[0], args[2], args[1])
                conv.fuse = False
                b = conv(args[0], args[2], args[1])
            rec['max_abs_diff'] = float((a - b).abs().max())
            rec['out_scale'] = float(b.abs().max())
            del a, b
            for _ in range(2):      # alternate the routes
                for fuse, key in ((True, 'fused_ms'), (False, 'generic_ms')):
                    conv.fuse = fuse
                    rec[key].append(round(median_ms(lambda: step(conv, *args), opt.iters,
                                                    opt.warmup), 4))
            conv.fuse = False
            rec['generic_peak_mib'] = round(peak(conv, args), 1)
            rec['ratio_generic_over_fused'] = round(min(rec['generic_ms']) / max(rec['fused_ms']),
                                                    3)
        except torch.OutOfMemoryError:
            rec['generic'] = 'out of memory'
            torch.cuda.empty_cache()
            conv.fuse = True
            if not rec['fused_ms']:
                rec['fused_ms'].append(round(median_ms(lambda: step(conv, *args), opt.iters,
                                                       opt.warmup), 4))
        conv.fuse = True
        rec['fused_peak_mib'] = round(peak(conv, args), 1)
        rec['fused_kernel_ms'] = kernel_times(conv, args)
        line = json.dumps(rec)
        print(line, flush=True)
        if opt.out:
            with open(opt.out, 'a') as f:
                f.write(line + '\n')
        del conv, args
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
