"""The geometric searches at the shapes of profiles/point_cloud.md: kernel route against the torch
fallback on the same device, with peak memory, plus the bare kernel time of each search.

    python scripts/time_point_cloud.py [--reps 20] [--out FILE]

``call`` times are host clocks around whole public calls ending in a device synchronise (a call
reads the example sizes or the output size on the host, so device events alone would miss that
wait); ``kernel`` times are device events around the C-ABI launch alone.  Routes alternate inside
one process after a warm-up of every shape and route."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_geometric_amd.nn as nn  # noqa: E402
from pytorch_geometric_amd import _native  # noqa: E402
from pytorch_geometric_amd.nn.pool import cluster  # noqa: E402


def host_timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def device_timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def both_routes(row, fn, reps, fallback_reps):
    for name, flag, n in (('kernel', True, reps), ('fallback', False, fallback_reps)):
        cluster.KERNELS = flag
        try:
            row[f'{name}_call_ms'] = host_timed(fn, n)
            row[f'{name}_peak_mib'] = peak(fn)
        finally:
            cluster.KERNELS = True
    row['speedup'] = row['fallback_call_ms'] / row['kernel_call_ms']
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    B, n = 32, 1024
    batch = torch.arange(B).repeat_interleave(n).to(dev)
    ptr = (torch.arange(B + 1) * n).to(dev)
    rows = []
    for F in (3, 64, 128):
        x = torch.randn(B * n, F, generator=g).to(dev)
        row = {'op': 'knn_graph', 'B': B, 'n': n, 'F': F, 'k': 20}
        row['kernel_ms'] = device_timed(lambda: _native.knn(x, x, ptr, ptr, 20, False, True),
                                        args.reps)
        # the plain dense alternative a user would write: cdist + topk per cloud (ties unpinned)
        row['cdist_topk_ms'] = device_timed(
            lambda: torch.cdist(x.view(B, n, F), x.view(B, n, F)).topk(21, largest=False), args.reps)
        rows.append(both_routes(row, lambda: nn.knn_graph(x, 20, batch, batch_size=B), args.reps, 3))
    x = torch.randn(B * n, 3, generator=g).to(dev)
    y = torch.randn(B * 512, 3, generator=g).to(dev)
    by = torch.arange(B).repeat_interleave(512).to(dev)
    ptr_y = (torch.arange(B + 1) * 512).to(dev)
    for r in (0.2, 0.5):
        row = {'op': 'radius', 'B': B, 'n': n, 'centres': 512, 'F': 3, 'cap': 64, 'r': r}
        row['kernel_ms'] = device_timed(lambda: _native.radius(x, y, ptr, ptr_y, r, 64), args.reps)
        row['edges'] = int(nn.radius(x, y, r, batch, by, 64, batch_size=B).size(1))
        rows.append(both_routes(
            row, lambda: nn.radius(x, y, r, batch, by, max_num_neighbors=64, batch_size=B),
            args.reps, 3))
    row = {'op': 'fps', 'B': B, 'n': n, 'F': 3, 'ratio': 0.5}
    out_ptr = (torch.arange(B + 1) * (n // 2)).to(dev)
    row['kernel_ms'] = device_timed(
        lambda: _native.fps(x, ptr, out_ptr, ptr[:-1].contiguous(), B * n // 2), args.reps)
    rows.append(both_routes(
        row, lambda: nn.fps(x, batch, ratio=0.5, random_start=False, batch_size=B), args.reps, 1))
    big = torch.randn(100_000, 3, generator=g).to(dev)
    row = {'op': 'fps', 'B': 1, 'n': 100_000, 'F': 3, 'ratio': 0.25}
    rows.append(both_routes(row, lambda: nn.fps(big, ratio=0.25, random_start=False), 2, 1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
