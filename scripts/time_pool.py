"""Times a training step (forward + backward) of TopKPooling and SAGPooling, fused against generic
route, and counts launches and peak memory (profiles/hier_pool.md).  The graphs are built here:

* ``molecules``  — 1,024 graphs of 10 .. 40 nodes, about 2.2 edges per node (a molecule-like batch);
* ``hundreds``   — 64 graphs of 200 .. 400 nodes, 8 edges per node;
* ``one_large``  — one graph of 1,024 nodes (the select kernel's envelope), 16 edges per node.

    python scripts/time_pool.py [--features 64] [--rounds 5] [--steps 50]

Both routes run interleaved in one process, ``--rounds`` rounds of ``--steps`` steps each after a
warm-up; the figure is the median over the rounds of the mean step time.  Launches are counted
with ``torch.profiler`` over one step (kernels and memsets / memcpys)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_geometric_amd.nn as nn  # noqa: E402


def make_batch(sizes, degree, features, seed, device):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.tensor(sizes)
    batch = torch.repeat_interleave(torch.arange(sizes.numel()), sizes)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    n = int(ptr[-1])
    e = int(n * degree)
    graph = torch.multinomial(sizes.float(), e, replacement=True, generator=g)
    lo, size = ptr[graph], sizes[graph]
    ends = [lo + (torch.rand(e, generator=g) * size).long().clamp(max=size - 1) for _ in range(2)]
    x = torch.randn(n, features, generator=g)
    return x.to(device), torch.stack(ends).to(device), batch.to(device)


def shapes(features, device):
    g = torch.Generator().manual_seed(0)
    mol = torch.randint(10, 41, (1024, ), generator=g).tolist()
    mid = torch.randint(200, 401, (64, ), generator=g).tolist()
    return {'molecules': make_batch(mol, 2.2, features, 1, device),
            'hundreds': make_batch(mid, 8, features, 2, device),
            'one_large': make_batch([1024], 16, features, 3, device)}


def step(layer, x, edge_index, batch):
    x = x.detach().requires_grad_(True)
    out, _, _, _, _, score = layer(x, edge_index, None, batch)
    (out.sum() + score.sum()).backward()


def timed(layer, data, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(layer, *data)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def launches(layer, data):
    from torch.profiler import ProfilerActivity, profile
    step(layer, *data)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(layer, *data)
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type.name != 'CPU')


def peak_mib(layer, data):
    step(layer, *data)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(layer, *data)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--features', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_pool.py measures on the GPU'
    dev = torch.device('cuda:0')
    rows = []
    for shape, data in shapes(args.features, dev).items():
        for kind in ('TopKPooling', 'SAGPooling'):
            layers = {}
            for fuse in (True, False):
                torch.manual_seed(0)
                layer = getattr(nn, kind)(args.features, ratio=0.5).to(dev)
                layer.fuse = fuse
                layers[fuse] = layer
            for layer in layers.values():      # warm-up: code objects, allocator, handle cache
                for _ in range(10):
                    step(layer, *data)
            times = {True: [], False: []}
            for _ in range(args.rounds):
                for fuse, layer in layers.items():
                    times[fuse].append(timed(layer, data, args.steps))
            row = {'shape': shape, 'layer': kind, 'nodes': data[0].size(0),
                   'edges': data[1].size(1), 'graphs': int(data[2].max()) + 1}
            for fuse, tag in ((True, 'fused'), (False, 'generic')):
                row[f'{tag}_us'] = round(statistics.median(times[fuse]), 1)
                row[f'{tag}_us_min'] = round(min(times[fuse]), 1)
                row[f'{tag}_launches'] = launches(layers[fuse], data)
                row[f'{tag}_peak_mib'] = round(peak_mib(layers[fuse], data), 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
