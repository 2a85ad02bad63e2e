"""Forward + backward of ``utils.spmm`` (sum, mean) on 16-bit device features: the native 16-bit
kernels (PYGAMD_SPMM_LP=1) against widen -> float32 kernels -> narrow (=0), and the float32 kernels
on float32 data for orientation.  Three graphs (Cora-sized, arxiv-sized, a power-law graph of 1 M
edges with hub rows) x F in {64, 128, 256} x {float16, bfloat16}.  The routes of one cell are timed
alternately, ROUNDS windows each (device events around ITERS steps after a warm-up); the table
holds the median window and the peak allocation of one step.  Writes the markdown table to the
path given (default: stdout).  What profiles/spmm_lp.md records."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_geometric_amd as pga  # noqa: E402
from pytorch_geometric_amd import _functions  # noqa: E402

ROUNDS = 5


def graphs(dev):
    g = torch.Generator().manual_seed(0)
    yield 'cora-sized', 2708, torch.randint(0, 2708, (2, 10556), generator=g).to(dev), 400
    yield 'arxiv-sized', 169343, torch.randint(0, 169343, (2, 1166243), generator=g).to(dev), 40
    n, e = 100000, 1000000   # Zipf-like endpoints: the first nodes collect tens of thousands of edges
    ends = (torch.rand(2, e, generator=g).pow(3) * n).long().clamp(max=n - 1)
    yield 'power-law 1M', n, ends.to(dev), 40


def window(h, x, go, reduce, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        out = pga.utils.spmm(h, x, reduce)
        torch.autograd.grad(out, [x], go)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3   # us per forward + backward


def main():
    dev = torch.device('cuda:0')
    lines = ['| graph | hubs dst/src | F | reduce | dtype | native us | widen us | widen/native | '
             'float32 us | native MiB | widen MiB |', '|' + '---|' * 11]
    for name, n, ei, iters in graphs(dev):
        h = pga.EdgeIndex(ei, (n, n)).fill_cache_()
        hubs = f'{h.by_dst().hub.n_hub}/{h.by_src().hub.n_hub}'
        for F in (64, 128, 256):
            x32 = torch.randn(n, F, device=dev)
            go32 = torch.randn(n, F, device=dev)
            for reduce in ('sum', 'mean'):
                for dtype in (torch.float16, torch.bfloat16):
                    cells = {'native': (True, dtype), 'widen': (False, dtype),
                             'float32': (None, torch.float32)}
                    times = {k: [] for k in cells}
                    peak = {}
                    for r in range(ROUNDS + 1):   # round 0 warms every route up
                        for k, (flag, dt) in cells.items():
                            _functions.SPMM_LP = flag
                            x = x32.to(dt).requires_grad_(True)
                            go = go32.to(dt)
                            torch.cuda.synchronize()
                            base = torch.cuda.memory_allocated()
                            torch.cuda.reset_peak_memory_stats()
                            t = window(h, x, go, reduce, 1 if r == 0 else iters)
                            peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                            if r:
                                times[k].append(t)
                    med = {k: statistics.median(v) for k, v in times.items()}
                    lines.append(
                        f'| {name} | {hubs} | {F} | {reduce} | {str(dtype)[6:]} | '
                        f'{med["native"]:.1f} | {med["widen"]:.1f} | '
                        f'{med["widen"] / med["native"]:.2f} | {med["float32"]:.1f} | '
                        f'{peak["native"]:.1f} | {peak["widen"]:.1f} |')
                    spread = max(max(v) / min(v) for v in times.values())
                    print(lines[-1], f'(max/min over windows <= {spread:.2f})', flush=True)
    text = '\n'.join(lines) + '\n'
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
