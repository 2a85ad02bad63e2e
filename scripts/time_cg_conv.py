"""CGConv: the fused route (csrc/cg.hip) against the generic route of the same layer (``fuse =
False``), forward + backward, on one device in one process — the figures of profiles/cg_conv.md.

    python scripts/time_cg_conv.py [--out FILE] [--iters 20] [--warmup 5] [--shapes ...]

Shapes, one per edge mode of the fused route:

* ``cgcnn`` — a CGCNN-like batch: 32,768 nodes with 12 in-edges each (uniformly random sources),
  64 channels and 41 edge features, the Gaussian-expanded distances of the paper: past the register
  envelope, so the dense edge terms (``wide``);
* ``powerlaw_dim8`` — 200,000 nodes and 2,000,000 edges whose destinations follow a power law
  (``N * u^3``, the longest rows hold thousands of slots), 128 channels, 8 raw edge features
  (``linear``);
* ``powerlaw`` — the same graph without edge features (``none``).

Per shape and route: ``torch.cuda.Event``s around one forward + backward (gradients of ``x``, of
``edge_attr`` and of every parameter: a training step of a layer inside a model), median over
``--iters`` calls after ``--warmup``, the two routes alternated twice (both medians are printed);
the peak memory above the inputs of one call; for the fused route the time of the three launches
from the records of ``_native.timing_sink``.  One JSON line per shape.  A route that runs out of
memory is recorded as such, not skipped silently."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_geometric_amd import _native, as_edge_index  # noqa: E402
from pytorch_geometric_amd.nn import CGConv  # noqa: E402

SHAPES = {
    'cgcnn': dict(N=32768, degree=12, channels=64, dim=41),
    'powerlaw_dim8': dict(N=200000, E=2000000, channels=128, dim=8),
    'powerlaw': dict(N=200000, E=2000000, channels=128, dim=0),
}


def edges(shape, g):
    N = shape['N']
    if 'degree' in shape:       # every node has `degree` in-edges
        dst = torch.arange(N).repeat_interleave(shape['degree'])
        src = torch.randint(0, N, (dst.numel(), ), generator=g)
        perm = torch.randperm(dst.numel(), generator=g)
        return torch.stack([src, dst])[:, perm].contiguous()
    E = shape['E']
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    return torch.stack([src, dst])


def problem(shape, dev):
    g = torch.Generator().manual_seed(1)
    N, C, dim = shape['N'], shape['channels'], shape['dim']
    ei = edges(shape, g)
    torch.manual_seed(2)
    conv = CGConv(C, dim=dim).to(dev)
    x = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
    ea = None
    if dim:
        ea = torch.randn(ei.size(1), dim, generator=g).to(dev).requires_grad_(True)
    graph = as_edge_index(ei.to(dev), N, N)
    graph.fill_cache_()
    graph.by_src()
    go = torch.randn(N, C, generator=g).to(dev)
    deg = torch.bincount(ei[1], minlength=N)
    return conv, (x, ea, graph, go), {'E': ei.size(1), 'max_in_degree': int(deg.max())}


def step(conv, x, ea, graph, go):
    out = conv(x, graph, ea)
    leaves = [x] + ([] if ea is None else [ea]) + [p for p in conv.parameters() if p.requires_grad]
    torch.autograd.grad(out, leaves, go)
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
    return {i['op']: round(a.elapsed_time(b), 4) for i, a, b in sink if i.get('kind') == 'cg'}


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
        conv, args, facts = problem(SHAPES[name], dev)
        rec = {'shape': name, **SHAPES[name], **facts, 'edge_mode': conv.edge_mode,
               'device': torch.cuda.get_device_name(0), 'fused_ms': [], 'generic_ms': []}
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
