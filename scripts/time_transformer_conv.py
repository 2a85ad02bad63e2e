"""Informational: one TransformerConv layer at BASELINE config 3's shape (ogbn-arxiv: N = 169,343,
E = 1,166,243, heads = 8, C = 32, so H*C = 256), forward and forward + backward, on a uniform and
on a power-law graph, all in one process:

* the fused route (one projection for key | value, one pass per destination),
* the score-mode route (alpha from the same kernel, multi-head weighted SpMM),
* the same class with ``fuse = False`` — gather / softmax / scatter kernels that predate the fused
  route: the yardstick.

Warm-up, HIP events around every repetition, medians.  Also times the fused forward kernel alone
and sets its algorithmic bytes ``E (8 HC + b + 4 H) + N (3 * 4 HC)`` (b = index bytes) against the
row-gather rate measured in the same run (``gather_rows`` of ``[N, 2 HC]`` rows by the same
sources), and the per-step ``cat`` of the key and value weights.
``python scripts/time_transformer_conv.py [--reps 15] [--out profiles/transformer_conv.md]``.

``--edge-dim D`` times the same layer with ``edge_dim = D`` and ``edge_attr [E, D]`` instead: with
``fuse_edge = True`` (edge features inside the one-pass kernels), in score mode, and with
``fuse_edge = False`` — the generic gather / ``message`` / scatter route such a layer takes by
default, code unchanged: the yardstick.  All in one process, same graphs."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_geometric_amd import _native, as_edge_index  # noqa: E402
from pytorch_geometric_amd._functions import TransformerAttendFunction  # noqa: E402
from pytorch_geometric_amd.nn import TransformerConv  # noqa: E402


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
    ap.add_argument('--out', default=None, help='also write the table to this file')
    ap.add_argument('--edge-dim', type=int, default=None,
                    help='time the layer with edge_dim = D: fuse_edge on, score mode, off')
    args = ap.parse_args()
    if args.edge_dim is not None:
        return main_edge(args)
    dev = torch.device('cuda:0')
    n, e, K, H, C = 169_343, 1_166_243, 256, 8, 32
    W = H * C
    x = torch.randn(n, K, generator=torch.Generator().manual_seed(1)).to(dev)
    lines = [f'TransformerConv({K}, {C}, heads={H}) at N = {n}, E = {e}, '
             f'{torch.cuda.get_device_name(0)}, medians of {args.reps}', '',
             '| graph | route | forward ms | forward + backward ms |', '|---|---|---|---|']
    for gname, ei in graphs(n, e, dev).items():
        torch.manual_seed(0)
        conv = TransformerConv(K, C, heads=H).to(dev).eval()
        routes = {'fused': (True, {}), 'score mode': (True, {'return_attention_weights': True}),
                  'fuse = False': (False, {})}
        for rname, (fuse, kw) in routes.items():
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
            lines.append(f'| {gname} | {rname} | {f:.3f} | {fb:.3f} |')
        # the attention part of the fused forward alone: the layer minus its projections
        conv.fuse = True
        with torch.no_grad():
            query = conv.lin_query(x).view(-1, H, C)
            kv = conv._project_key_value(x).view(-1, 2, H, C)
        graph = as_edge_index(ei, n, n)
        scale = 1 / math.sqrt(C)
        t = median_ms(lambda: TransformerAttendFunction.apply(query, kv, None, graph, scale, n),
                      args.reps)
        # the row-gather rate of this run: [N, 2 HC] rows gathered by the same sources
        col = graph.by_dst().idx
        rows = kv.view(n, 2 * W)
        tg = median_ms(lambda: _native.gather_rows(rows, col), args.reps)
        idx_bytes = col.element_size()
        rate = (e * (2 * 2 * W * 4 + idx_bytes)) / (tg * 1e-3)      # read + write of every row
        alg = e * (8 * W + idx_bytes + 4 * H) + n * 3 * 4 * W
        tc = median_ms(lambda: (torch.cat([conv.lin_key.weight, conv.lin_value.weight]),
                                torch.cat([conv.lin_key.bias, conv.lin_value.bias])), args.reps)
        lines.append(f'| {gname} | fused kernel alone | {t:.3f} | — |')
        lines.append(f'|  | algorithmic bytes {alg / 1e9:.3f} GB -> {alg / t / 1e6:.0f} GB/s = '
                     f'{alg / (t * 1e-3) / rate:.2f} of the row-gather rate measured here '
                     f'({rate / 1e12:.2f} TB/s, gather_rows of [N, {2 * W}] in {tg:.3f} ms) |  |  |')
        lines.append(f'|  | cat of the key and value weights, per step | {tc:.3f} | — |')
    emit(lines, args.out)


def main_edge(args):
    dev = torch.device('cuda:0')
    n, e, K, H, C, D = 169_343, 1_166_243, 256, 8, 32, args.edge_dim
    x = torch.randn(n, K, generator=torch.Generator().manual_seed(1)).to(dev)
    ea = torch.randn(e, D, generator=torch.Generator().manual_seed(2)).to(dev).requires_grad_(True)
    lines = [f'TransformerConv({K}, {C}, heads={H}, edge_dim={D}) at N = {n}, E = {e}, '
             f'{torch.cuda.get_device_name(0)}, medians of {args.reps}; edge_attr requires grad',
             '', '| graph | route | forward ms | forward + backward ms |', '|---|---|---|---|']
    for gname, ei in graphs(n, e, dev).items():
        torch.manual_seed(0)
        conv = TransformerConv(K, C, heads=H, edge_dim=D).to(dev).eval()
        routes = {'fuse_edge = True': (True, {}),
                  'fuse_edge = True, score mode': (True, {'return_attention_weights': True}),
                  'fuse_edge = False': (False, {})}
        for rname, (fuse_edge, kw) in routes.items():
            conv.fuse_edge = fuse_edge

            def out():
                res = conv(x, ei, ea, **kw)
                return res[0] if isinstance(res, tuple) else res

            def fwd():
                with torch.no_grad():
                    out()

            def both():
                conv.zero_grad()
                ea.grad = None
                out().sum().backward()

            f, fb = median_ms(fwd, args.reps), median_ms(both, args.reps)
            lines.append(f'| {gname} | {rname} | {f:.3f} | {fb:.3f} |')
    emit(lines, args.out)


def emit(lines, path):
    text = '\n'.join(lines)
    print(text)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
