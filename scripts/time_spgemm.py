"""Times the sparse-sparse product ``A @ A`` (csrc/spgemm.hip) against the reference's expression
(``torch.sparse`` CSR ``adj @ adj`` on the device; on the CPU where that does not run) at three
shapes, and one training step of ``GraphUNet(depth=3)`` with ``fuse`` on against off.  Routes are
interleaved in one process; median and minimum over the rounds.  Prints one JSON line per figure.

    python scripts/time_spgemm.py [--rounds 15] [--small]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_geometric_amd import _native  # noqa: E402
from pytorch_geometric_amd.nn import GraphUNet  # noqa: E402
from pytorch_geometric_amd.utils import coalesce  # noqa: E402

DEV = 'cuda'


def graph(kind, small):
    g = torch.Generator().manual_seed(0)
    if kind == 'cora':
        n, e = 2708, 10556
        ei = torch.randint(0, n, (2, e), generator=g)
    elif kind == 'molecules':   # 1,024 graphs of 23 nodes, 50 edges inside each
        b, k = (64 if small else 1024), 23
        n = b * k
        ei = torch.randint(0, k, (2, b * 50), generator=g) + (torch.arange(b * 50) // 50) * k
    else:                       # power law: ~100 k nodes, ~1 M edges
        n, e = (10_000, 100_000) if small else (100_000, 1_000_000)
        dst = (torch.rand(e, generator=g).pow(4) * n).long().clamp(max=n - 1)
        ei = torch.stack([dst, torch.randint(0, n, (e, ), generator=g)])   # (hub ROWS)
    ei = coalesce(ei.to(DEV), num_nodes=n)
    return ei, n


def timed(fn, device=True):
    if device:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if device:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4)}


def product(kind, rounds, small):
    ei, n = graph(kind, small)
    ptr = _native.index2ptr(ei[0].contiguous(), n)
    col = ei[1].contiguous()
    val = torch.rand(col.numel(), device=DEV)
    fused = lambda: _native.spgemm(ptr, col, val, ptr, col, val, n, n, n)
    where = 'device'
    adj = torch.sparse_csr_tensor(ptr, col, val, (n, n))
    try:
        timed(lambda: adj @ adj)
    except Exception as exc:   # the expression does not run on this build: the CPU's time instead
        where = f'cpu ({type(exc).__name__}: {str(exc)[:80]})'
        adj = adj.cpu()
    generic = lambda: adj @ adj
    fused()
    ms = {'fused': [], 'generic': []}
    sink = []
    for _ in range(rounds):
        for name, fn in (('fused', fused), ('generic', generic)):
            ms[name].append(timed(fn, name == 'fused' or where == 'device')[0])
    _native.timing_sink = sink
    torch.cuda.reset_peak_memory_stats()
    rowptr_c, col_c, _ = fused()
    torch.cuda.synchronize()
    _native.timing_sink = None
    phases = {info['op']: round(e0.elapsed_time(e1), 4) for info, e0, e1 in sink}
    products = int(sink[-1][0].get('long_products', 0))
    lens = ptr.diff()
    ub = torch.zeros(n, dtype=torch.long, device=DEV).index_add_(
        0, torch.repeat_interleave(torch.arange(n, device=DEV), lens), lens[col])
    total = int(ub.sum())
    tiers = [int(((ub >= lo) & (ub <= hi)).sum()) for lo, hi in (
        (0, 0), (1, _native.SPGEMM_WAVE_UB),
        (_native.SPGEMM_WAVE_UB + 1, _native.SPGEMM_GROUP_SMALL_UB),
        (_native.SPGEMM_GROUP_SMALL_UB + 1, _native.SPGEMM_GROUP_UB),
        (_native.SPGEMM_GROUP_UB + 1, 2 ** 62))]
    # the serial-k rule: a step of the walk uses |B_k| of 64 lanes
    steps = int(((lens[col] + 63) // 64).sum())
    print(json.dumps({
        'what': 'A@A', 'shape': kind, 'n': n, 'nnz': col.numel(), 'nnz_c': col_c.numel(),
        'products': total, 'rows_per_tier': tiers, 'long_products': products,
        'lane_use': round(total / max(64 * steps, 1), 4), 'phases_ms': phases,
        'peak_MiB': round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
        'fused': summary(ms['fused']), 'generic': summary(ms['generic']), 'generic_on': where,
        'products_per_s': round(total / (statistics.median(ms['fused']) * 1e-3), 0)}), flush=True)


def unet_step(rounds, small):
    ei, n = graph('molecules', small)
    batch = torch.arange(n, device=DEV) // 23
    x = torch.randn(n, 32, device=DEV)
    model = GraphUNet(32, 64, 8, depth=3).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)

    def step():
        opt.zero_grad()
        model(x, ei, batch).square().mean().backward()
        opt.step()

    ms = {True: [], False: []}
    skipped = None
    for r in range(rounds + 1):
        for fuse in (True, False):
            model.fuse = fuse
            try:
                t = timed(step)[0]
            except Exception as exc:
                skipped = f'{type(exc).__name__}: {str(exc)[:80]}'
                continue
            if r:
                ms[fuse].append(t)
    print(json.dumps({'what': 'GraphUNet(depth=3) step', 'n': n, 'edges': ei.size(1),
                      'fuse_on': summary(ms[True]) if ms[True] else None,
                      'fuse_off': summary(ms[False]) if ms[False] else skipped}), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    for kind in ('cora', 'molecules', 'power_law'):
        product(kind, args.rounds, args.small)
    unet_step(args.rounds, args.small)
