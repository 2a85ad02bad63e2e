"""Forward + backward of GraphNorm and LayerNorm(mode='graph'), fused against generic, at the three
shapes of profiles/graph_norm.md, with peak memory, the C-ABI launches per call and — in the same
run — the time of a streaming read + write of the same bytes (``y = 2 x`` on the [N, F] plane, the
traffic of one pass) to put the kernels' rate against.

    python scripts/time_graph_norm.py [--reps 30] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_graph_norm.py --trace small

``--trace small | medium | single`` runs nothing but ``reps`` fused forward + backward calls of
GraphNorm and of LayerNorm at that shape, for a kernel trace taken in a run of its own.

Routes alternate inside one process; times are device events around ``reps`` calls after a warm-up
of every shape and route."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_geometric_amd.nn as nn  # noqa: E402
from pytorch_geometric_amd import _lib, _native  # noqa: E402


def shapes(dev):
    g = torch.Generator().manual_seed(0)
    small = torch.randint(20, 31, (4096, ), generator=g)
    medium = torch.randint(4800, 5201, (64, ), generator=g)
    yield 'small graphs', small, 128, True
    yield 'medium graphs', medium, 256, True
    yield 'one graph, batch=None', torch.tensor([2_000_000]), 128, False


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def peak(fn, drop):
    """peak of one ``fn()`` above what is allocated before it; ``drop()`` frees what the warm-up
    call left (the previous ``x.grad``), so that ``grad_x`` counts"""
    fn()
    drop()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


class Counter:
    def __init__(self, lib):
        self.lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith('pygamd_') or not callable(fn):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', default=None, choices=('small', 'medium', 'single'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    rows = []
    for what, sizes, F, with_batch in shapes(dev):
        if args.trace is not None and not what.startswith(
                {'small': 'small', 'medium': 'medium', 'single': 'one graph'}[args.trace]):
            continue
        N = int(sizes.sum())
        batch = torch.repeat_interleave(torch.arange(sizes.numel()), sizes).to(dev) \
            if with_batch else None
        x = torch.randn(N, F, device=dev).requires_grad_(True)
        go = torch.randn(N, F, device=dev)
        plane = x.detach()
        copy_ms = timed(lambda: torch.mul(plane, 2.0), args.reps)
        for cls in (nn.GraphNorm, nn.LayerNorm):
            layer = cls(F).to(dev)

            def step():
                x.grad = None
                out = layer(x, batch) if with_batch else layer(x)
                out.backward(go)

            if args.trace is not None:
                for _ in range(args.reps):
                    step()
                torch.cuda.synchronize()
                continue
            row = {'shape': what, 'layer': cls.__name__, 'N': N, 'F': F, 'B': sizes.numel(),
                   'copy_ms': copy_ms}
            for fuse in (True, False):
                layer.fuse = fuse
                key = 'fused' if fuse else 'generic'
                row[f'{key}_ms'] = timed(step, args.reps)
                row[f'{key}_peak_mib'] = peak(step, lambda: setattr(x, 'grad', None)) / 2 ** 20
            layer.fuse = True
            real = _lib.load
            counter = Counter(real())
            _lib.load = lambda: counter
            try:
                step()
                torch.cuda.synchronize()
            finally:
                _lib.load = real
            row['fused_calls'] = {k: v for k, v in counter.calls.items() if 'graph_norm' in k}
            handle_plan = _native.graph_norm_plan(
                _native.index2ptr(batch, sizes.numel())) if with_batch else None
            row['n_hub'] = handle_plan.n_hub if handle_plan is not None else 1
            # forward reads x twice and writes y; backward reads x and grad_y twice and writes
            # grad_x: 8 plane passes against the copy's 2
            row['fused_share_of_stream'] = 4 * copy_ms / row['fused_ms']
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0),
                       'threshold': _native.GRAPH_NORM_THRESHOLD,
                       'chunk': _native.GRAPH_NORM_CHUNK, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
