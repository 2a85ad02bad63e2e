"""Forward + backward of ``segment_matmul_sum`` (the transform-and-sum tail of RGCNConv) on 16-bit
device operands: the native route (csrc/segmm_lp.hip + the 16-bit SpMM) against what a caller can do
without it — cast rows and weights to float32, run the float32 route, cast the result back (the
casts are part of the step, their gradients come back 16-bit).  Two shapes x {float16, bfloat16}:
the FB15k-237 RGCN layer of bench_configs.py config 5 (474 relations, 5 blocks of 100 x 100 on the
(relation, destination) pair rows) and a dense-ish one (8 groups, K = N = 256, 131,072 rows onto
16,384 destinations).  The two routes of a cell are timed alternately in one process, ROUNDS
windows each after a warm-up round (device events around ITERS steps); the table holds the median
window, the max / min over either route's windows (the spread) and the peak allocation of one step
above the inputs.  Writes the markdown table to the path given (default: stdout).  What
profiles/segmm_lp.md records."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_geometric_amd as pga  # noqa: E402
from pytorch_geometric_amd.nn.conv.rgcn_conv import RelationalHandle  # noqa: E402
from pytorch_geometric_amd.utils._segment_matmul import segment_matmul_sum  # noqa: E402

ROUNDS, ITERS = 5, 50


def shapes(dev):
    g = torch.Generator().manual_seed(4)   # (the graph of bench_configs.config5)
    n, e, R = 14_541, 544_230, 474
    ei = torch.randint(0, n, (2, e), generator=g)
    et = (torch.rand(e, generator=g).pow(4) * R).long().clamp(max=R - 1)
    h = RelationalHandle(ei.to(dev), et.to(dev), n, n, R)
    yield 'FB15k-237 RGCN (474 x 5 blocks of 100 x 100)', h.num_pairs, h.rel_ptr, (R, 5, 100, 100), \
        h.out_graph
    S, n, G = 131072, 16384, 8
    dst = torch.randint(0, n, (S, ), generator=g).to(dev)
    graph = pga.EdgeIndex(torch.stack([torch.arange(S, device=dev), dst]), (S, n),
                          sort_order='row', validate=False)
    yield 'dense-ish (8 groups of 256 x 256)', S, tuple(range(0, S + 1, S // G)), (G, 256, 256), graph


def window(step, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        step()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3   # us per step


def main():
    dev = torch.device('cuda:0')
    lines = ['| shape | rows | dtype | native us | widened us | widened/native | spread | '
             'native MiB | widened MiB |', '|' + '---|' * 9]
    for name, S, ptr, wshape, graph in shapes(dev):
        graph.fill_cache_()
        width = wshape[-2] * (wshape[1] if len(wshape) == 4 else 1)
        for dtype in (torch.float16, torch.bfloat16):
            torch.manual_seed(0)
            x = torch.randn(S, width, device=dev).to(dtype).requires_grad_(True)
            w = (torch.randn(wshape, device=dev) / wshape[-2] ** 0.5).to(dtype).requires_grad_(True)

            def native():
                out = segment_matmul_sum(x, ptr, w, graph)
                torch.autograd.grad(out, (x, w), out.detach())

            def widened():
                out = segment_matmul_sum(x.float(), ptr, w.float(), graph).to(dtype)
                torch.autograd.grad(out, (x, w), out.detach())

            routes = {'native': native, 'widened': widened}
            times, peak = {k: [] for k in routes}, {}
            for r in range(ROUNDS + 1):   # round 0 warms both routes up
                for k, step in routes.items():
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    t = window(step, 2 if r == 0 else ITERS)
                    peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                    if r:
                        times[k].append(t)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = max(max(v) / min(v) for v in times.values())
            lines.append(f'| {name} | {S} | {str(dtype)[6:]} | {med["native"]:.1f} | '
                         f'{med["widened"]:.1f} | {med["widened"] / med["native"]:.2f} | '
                         f'{spread:.2f} | {peak["native"]:.1f} | {peak["widened"]:.1f} |')
            print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
