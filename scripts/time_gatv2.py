"""Informational: one GATv2Conv layer at BASELINE config 3's shape (ogbn-arxiv: N = 169,343,
E = 1,166,243 + N self-loops, heads = 8, C = 32, so H*C = 256), forward and forward + backward, on
a uniform and on a power-law graph:

* the fused route (one pass per destination),
* the score-mode route (alpha from the same kernel, multi-head weighted SpMM),
* the same class with ``fuse = False`` — kernels that predate the fused route: the yardstick,
* ``GATConv`` fused at the same shape, for scale.

Warm-up, HIP events around every repetition, medians.  Also prints the forward pass's achieved
fraction of the measured row-gather rate (5.5 TB/s) from its algorithmic bytes
``E (4 HC + b + 4 H) + N (3 * 4 HC)``.  ``python scripts/time_gatv2.py [--reps 15]``."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_geometric_amd.nn import GATConv, GATv2Conv  # noqa: E402

GATHER_RATE = 5.5e12  # bytes / s, rows in flight per wave at 16 waves per CU


def graphs(n, e, dev):
    g = torch.Generator().manual_seed(0)
    uniform = torch.randint(0, n, (2, e), generator=g)
    # power law: destinations ~ u^6 (a few rows of tens of thousands of edges), sources u^2
    dst = (torch.rand(e, generator=g).pow(6) * n).long().clamp(max=n - 1)
    src = (torch.rand(e, generator=g).pow(2) * n).long().clamp(max=n - 1)
    return {'uniform': uniform.to(dev), 'power-law': torch.stack([src, dst]).to(dev)}


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=None, help='also append the table to this file')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n, e, K, H, C = 169_343, 1_166_243, 256, 8, 32
    x = torch.randn(n, K, generator=torch.Generator().manual_seed(1)).to(dev)
    lines = [f'GATv2Conv({K}, {C}, heads={H}) at N = {n}, E = {e} + N loops, '
             f'{torch.cuda.get_device_name(0)}, medians of {args.reps}', '',
             '| graph | route | forward ms | forward + backward ms |', '|---|---|---|---|']
    for gname, ei in graphs(n, e, dev).items():
        torch.manual_seed(0)
        v2 = GATv2Conv(K, C, heads=H).to(dev)
        v1 = GATConv(K, C, heads=H).to(dev)
        routes = {'fused': (v2, True, {}), 'score mode': (v2, True, {'return_attention_weights': True}),
                  'fuse = False': (v2, False, {}), 'GATConv fused': (v1, True, {})}
        fwd_ms = {}
        for rname, (conv, fuse, kw) in routes.items():
            conv.fuse = fuse

            def out():
                res = conv(x, ei, **kw)
                return res[0] if isinstance(res, tuple) else res

            def fwd():
                with torch.no_grad():
                    out()

            def both():
                conv.zero_grad()
                out().sum().backward()

            f, fb = median_ms(fwd, args.reps), median_ms(both, args.reps)
            fwd_ms[rname] = f
            lines.append(f'| {gname} | {rname} | {f:.3f} | {fb:.3f} |')
        # the attention part of the fused forward alone: the layer minus its two projections
        conv = v2
        conv.fuse = True
        x_l = conv.lin_l(x).view(-1, H, C).detach()
        x_r = conv.lin_r(x).view(-1, H, C).detach()
        from pytorch_geometric_amd import as_edge_index
        from pytorch_geometric_amd._functions import Gatv2AttendFunction
        from pytorch_geometric_amd.nn.conv.gatv2_conv import _LOOPS
        looped = next(v[3] for v in _LOOPS.values() if v[0]() is ei)
        graph = as_edge_index(looped, n, n)
        t = median_ms(lambda: Gatv2AttendFunction.apply(x_l, x_r, conv.att.detach(), graph, 0.2, n),
                      args.reps)
        E = looped.size(1)
        alg = E * (4 * H * C + 8 + 4 * H) + n * 3 * 4 * H * C
        lines.append(f'| {gname} | fused kernel alone | {t:.3f} | — |')
        lines.append(f'|  | algorithmic bytes {alg / 1e9:.3f} GB -> {alg / t / 1e9:.0f} GB/s = '
                     f'{alg / (t * 1e-3) / GATHER_RATE:.2f} of the gather rate |  |  |')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
