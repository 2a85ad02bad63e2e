"""SplineConv: the fused route (csrc/spline.hip) against the generic route of the same layer
(``fuse = False``), forward + backward, on one device in one process — the figures of
profiles/spline_conv.md.

    python scripts/time_spline_conv.py [--out FILE] [--iters 20] [--warmup 5] [--shapes ...]

Shapes: a batch of 64 superpixel graphs (75 nodes and 1,400 edges each, edges inside their graph;
dim 2, kernel_size 5) at 1 -> 32 and at 32 -> 64 channels; one FAUST-sized mesh (6,890 nodes, 41,328
edges; dim 3, kernel_size 5, 32 -> 64); a power-law graph (100,000 nodes, 1,000,000 edges, hub rows
on both sides; dim 2, kernel_size 5, 64 -> 64).  degree 1, ``aggr='mean'``.  Per shape and route:
``torch.cuda.Event``s around one forward + backward (gradients of ``x`` and of every parameter),
median over ``--iters`` calls after ``--warmup``, the two routes alternated twice (both medians
are printed); the peak memory above the inputs of one call; the launches this package makes in one
call with their times (records of ``_native.timing_sink``: the spline kernels and the package's
own dense products; launches torch makes itself, all of the generic route's, are not in them).
One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_geometric_amd import _native, as_edge_index  # noqa: E402
from pytorch_geometric_amd.nn import SplineConv  # noqa: E402

SHAPES = {
    'superpixels_1_32': dict(kind='batch', graphs=64, nodes=75, edges=1400, dim=2, cin=1, cout=32),
    'superpixels_32_64': dict(kind='batch', graphs=64, nodes=75, edges=1400, dim=2, cin=32, cout=64),
    'faust': dict(kind='uniform', N=6890, E=41328, dim=3, cin=32, cout=64),
    'power_law': dict(kind='power', N=100000, E=1000000, dim=2, cin=64, cout=64),
}


def edges(shape, g):
    if shape['kind'] == 'batch':
        B, n, e = shape['graphs'], shape['nodes'], shape['edges']
        base = (torch.arange(B) * n).repeat_interleave(e)
        return torch.randint(0, n, (2, B * e), generator=g) + base, B * n
    N, E = shape['N'], shape['E']
    if shape['kind'] == 'uniform':
        return torch.randint(0, N, (2, E), generator=g), N
    skew = torch.rand(2, E, generator=g) ** torch.tensor([[2.0], [4.0]])   # hubs on both sides
    return (skew * N).long().clamp(max=N - 1), N


def problem(shape, dev):
    g = torch.Generator().manual_seed(1)
    ei, N = edges(shape, g)
    torch.manual_seed(2)
    conv = SplineConv(shape['cin'], shape['cout'], dim=shape['dim'], kernel_size=5).to(dev)
    x = torch.randn(N, shape['cin'], generator=g).to(dev).requires_grad_(True)
    pseudo = torch.rand(ei.size(1), shape['dim'], generator=g).to(dev)
    graph = as_edge_index(ei.to(dev), N, N)
    graph.fill_cache_()
    graph.by_src()
    go = torch.randn(N, shape['cout'], generator=g).to(dev)
    return conv, x, pseudo, graph, go


def step(conv, x, pseudo, graph, go):
    out = conv(x, graph, pseudo)
    torch.autograd.grad(out, [x] + list(conv.parameters()), go)
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
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def launches(conv, args):
    sink = []
    _native.timing_sink = sink
    try:
        step(conv, *args)
        torch.cuda.synchronize()
    finally:
        _native.timing_sink = None
    return [[i.get('kind'), i.get('op'), round(a.elapsed_time(b), 4)] for i, a, b in sink]


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
        rec = {'shape': name, **SHAPES[name], 'E': args[1].size(0),
               'device': torch.cuda.get_device_name(0), 'fused_ms': [], 'generic_ms': []}
        outs = {}
        with torch.no_grad():
            for fuse in (True, False):
                conv.fuse = fuse
                outs[fuse] = conv(args[0], args[2], args[1])
        rec['max_abs_diff'] = float((outs[True] - outs[False]).abs().max())
        rec['out_scale'] = float(outs[False].abs().max())
        del outs
        for _ in range(2):      # alternate the routes
            for fuse, key in ((True, 'fused_ms'), (False, 'generic_ms')):
                conv.fuse = fuse
                rec[key].append(round(median_ms(lambda: step(conv, *args), opt.iters,
                                                opt.warmup), 4))
        rec['ratio_generic_over_fused'] = round(min(rec['generic_ms']) / max(rec['fused_ms']), 3)
        for fuse, key in ((False, 'generic'), (True, 'fused')):
            conv.fuse = fuse
            rec[key + '_peak_mib'] = peak(conv, args)
            rec[key + '_launches'] = launches(conv, args)
        line = json.dumps(rec)
        print(line, flush=True)
        if opt.out:
            with open(opt.out, 'a') as f:
                f.write(line + '\n')
        del conv, args
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
