"""Forward + backward of one ``SAGEConv`` layer on 16-bit storage: the one-kernel 16-bit layer
(``fuse_lp = True``, csrc/sage_fused_lp.hip) against the generic 16-bit route (``fuse_lp = False``:
16-bit SpMM, two ``torch`` linears and an add).  The arxiv-sized graph and the power-law graph of
1 M edges of profiles/spmm_lp.md x F = Fo in {64, 128, 256} x {float16, bfloat16}, mean.  The two
routes of a cell are timed alternately in one process, ROUNDS windows each after a warm-up round
(device events around ITERS steps, a quarter of a second); the table holds the median window, the
max / min over the forward + backward windows of either route (the spread), the same median for the
forward alone under ``torch.no_grad`` (FWD_ITERS steps; the new route then writes no ``agg``), the
device kernels of one recording forward and of one backward as ``torch.profiler`` lists them, traced
in a pass of its own after the cell's timed windows, and the peak allocation of one step above the
inputs.  Writes the markdown table to the path given (default: stdout).  What
profiles/sage_layer_lp.md records."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_geometric_amd as pga  # noqa: E402

ROUNDS, ITERS, FWD_ITERS = 5, 200, 800


def graphs(dev):
    g = torch.Generator().manual_seed(0)
    torch.randint(0, 2708, (2, 10556), generator=g)   # (the generator state of spmm_lp_probe.py)
    yield 'arxiv-sized', 169343, torch.randint(0, 169343, (2, 1166243), generator=g).to(dev)
    n, e = 100000, 1000000   # Zipf-like endpoints: the first nodes collect tens of thousands of edges
    ends = (torch.rand(2, e, generator=g).pow(3) * n).long().clamp(max=n - 1)
    yield 'power-law 1M', n, ends.to(dev)


def window(conv, h, x, iters, backward=True):
    params = [x] + list(conv.parameters())
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        if backward:
            out = conv(x, h)
            torch.autograd.grad(out, params, out.detach())
        else:
            with torch.no_grad():
                conv(x, h)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3   # us per step


def kernels(fn):
    """device kernels (copies and fills left out) that ``fn`` launches, from a profiler trace"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    on_device = torch.autograd.DeviceType.CUDA   # (the runtime's own calls are listed as host events)
    return sum(1 for ev in prof.events() if ev.device_type == on_device
               and 'Memcpy' not in ev.name and 'Memset' not in ev.name)


def launches(conv, h, x):
    """'forward+backward' kernels of one step (the forward recording, as in a training step)"""
    params = [x] + list(conv.parameters())
    kept = []
    fwd = kernels(lambda: kept.append(conv(x, h)))
    bwd = kernels(lambda: torch.autograd.grad(kept[0], params, kept[0].detach()))
    return f'{fwd}+{bwd}'


def main():
    dev = torch.device('cuda:0')
    lines = ['| graph | hubs dst/src | F = Fo | dtype | new us | generic us | generic/new | spread | '
             'launches new fwd+bwd | launches generic fwd+bwd | new MiB | generic MiB | '
             'forward only: new us | generic us |', '|' + '---|' * 14]
    for name, n, ei in graphs(dev):
        h = pga.EdgeIndex(ei, (n, n)).fill_cache_()
        hubs = f'{h.by_dst().hub.n_hub}/{h.by_src().hub.n_hub}'
        for F in (64, 128, 256):
            x32 = torch.randn(n, F, device=dev)
            for dtype in (torch.float16, torch.bfloat16):
                torch.manual_seed(0)
                conv = pga.nn.SAGEConv(F, F).to(dev).to(dtype)
                x = x32.to(dtype).requires_grad_(True)
                times, peak = {'new': [], 'generic': []}, {}
                fwd = {'new': [], 'generic': []}   # (inference: torch.no_grad, no agg written)
                for r in range(ROUNDS + 1):   # round 0 warms both routes up
                    for k in times:
                        conv.fuse_lp = k == 'new'
                        torch.cuda.synchronize()
                        base = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        t = window(conv, h, x, 1 if r == 0 else ITERS)
                        peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                        tf = window(conv, h, x, 1 if r == 0 else FWD_ITERS, backward=False)
                        if r:
                            times[k].append(t)
                            fwd[k].append(tf)
                med = {k: statistics.median(v) for k, v in times.items()}
                spread = max(max(v) / min(v) for v in times.values())
                counts = {}
                for k in times:   # traced after the timed windows, never inside one
                    conv.fuse_lp = k == 'new'
                    counts[k] = launches(conv, h, x)
                lines.append(
                    f'| {name} | {hubs} | {F} | {str(dtype)[6:]} | {med["new"]:.1f} | '
                    f'{med["generic"]:.1f} | {med["generic"] / med["new"]:.2f} | {spread:.2f} | '
                    f'{counts["new"]} | {counts["generic"]} | {peak["new"]:.1f} | '
                    f'{peak["generic"]:.1f} | {statistics.median(fwd["new"]):.1f} | '
                    f'{statistics.median(fwd["generic"]):.1f} |')
                print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
