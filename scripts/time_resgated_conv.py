"""ResGatedGraphConv: the fused route (csrc/resgated.hip) against the generic route of the same
layer (``fuse = False``), forward + backward, on one device in one process — the figures of
profiles/resgated_conv.md.

    python scripts/time_resgated_conv.py [--out FILE] [--iters 20] [--warmup 5] [--shapes ...]

Shapes: those of scripts/time_gen_conv.py — the node and edge counts of ogbn-arxiv (uniformly random
edges) with in = out = 128; a proteins-like shape (132,534 nodes, mean in-degree 75, F = 64); a
molecule batch (3,000 nodes, 6,500 edges, F = 64) — each without ``edge_dim`` and with it (8, 8 and
4).  Per shape and route: ``torch.cuda.Event``s around one forward + backward, median over
``--iters`` calls after ``--warmup``, the two routes alternated twice (both medians are printed);
the peak memory above the inputs of one call; for the fused route the time of the three launches
from the records of ``_native.timing_sink``; and the by-source backward with its two gathered
rows per slot (K and grad_out in place) against one row of a packed ``[N_dst, 2F]`` plane, the
``torch.cat`` that packs it included.  One JSON line per shape.  A route that runs out of memory
is recorded as such, not skipped silently."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_geometric_amd import _native, as_edge_index  # noqa: E402
from pytorch_geometric_amd.nn import ResGatedGraphConv  # noqa: E402

_BASE = {
    'arxiv': dict(N=169343, E=1166243, channels=128, edge_dim=8),
    'proteins_like': dict(N=132534, E=132534 * 75, channels=64, edge_dim=8),
    'molecules': dict(N=3000, E=6500, channels=64, edge_dim=4),
}
SHAPES = {}
for _name, _shape in _BASE.items():
    SHAPES[_name] = dict(_shape, edge_dim=None)
    SHAPES[_name + '_edge'] = dict(_shape)


def problem(shape, dev):
    g = torch.Generator().manual_seed(1)
    N, E, C = shape['N'], shape['E'], shape['channels']
    ei = torch.randint(0, N, (2, E), generator=g)
    torch.manual_seed(2)
    conv = ResGatedGraphConv(C, C, edge_dim=shape['edge_dim']).to(dev)
    x = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
    ea = None
    if shape['edge_dim']:
        ea = torch.randn(E, shape['edge_dim'], generator=g).to(dev)
    graph = as_edge_index(ei.to(dev), N, N)
    graph.fill_cache_()
    graph.by_src()
    go = torch.randn(N, C, generator=g).to(dev)
    return conv, x, ea, graph, go


def step(conv, x, ea, graph, go):
    out = conv(x, graph, ea)
    params = [p for p in conv.parameters() if p.requires_grad]
    torch.autograd.grad(out, [x] + params, go)
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
    return {i['op']: round(a.elapsed_time(b), 4) for i, a, b in sink
            if i.get('kind') == 'resgated'}


def source_pass(shape, graph, ea, dev, iters, warmup):
    """the by-source backward alone: K and grad_out gathered as two rows in place, or as one row
    of a plane packed by ``torch.cat`` inside the timed region"""
    g = torch.Generator().manual_seed(3)
    N, C, De = shape['N'], shape['channels'], shape['edge_dim'] or 0
    k = torch.randn(N, C, generator=g).to(dev)
    qv = torch.randn(N, 2 * C, generator=g).to(dev)
    go = torch.randn(N, C, generator=g).to(dev)
    w = torch.randn(2, C, De, generator=g).to(dev) if De else None
    bwd = graph.by_src()
    eid = bwd.perm if De else None

    def two_rows():
        return _native.resgated_backward_src(bwd.ptr, bwd.idx, eid, k, qv, ea, w, go, hub=bwd.hub)

    def packed():
        plane = torch.cat([k, go], dim=1)
        return _native.resgated_backward_src(bwd.ptr, bwd.idx, eid, plane[:, :C], qv, ea, w,
                                             plane[:, C:], hub=bwd.hub)

    assert torch.equal(two_rows(), packed())
    out = {'two_rows_ms': [], 'packed_ms': []}
    for _ in range(2):
        out['two_rows_ms'].append(round(median_ms(two_rows, iters, warmup), 4))
        out['packed_ms'].append(round(median_ms(packed, iters, warmup), 4))
    return out


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
        rec['source_pass'] = source_pass(SHAPES[name], args[2], args[1], dev, opt.iters,
                                         opt.warmup)
        line = json.dumps(rec)
        print(line, flush=True)
        if opt.out:
            with open(opt.out, 'a') as f:
                f.write(line + '\n')
        del conv, args
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
