"""RGATConv: the fused route (csrc/rgat.hip) against the generic route of the same layer (``fuse =
False``: the restatement through ``propagate``), forward + backward, on one device in one process
— the figures of profiles/rgat_conv.md.

    python scripts/time_rgat_conv.py [--out FILE] [--iters 20] [--warmup 5] [--shapes ...]

Shapes (``mechanism``: across-relation unless the name says within):

* ``powerlaw_r4`` — 200,000 nodes and 2,000,000 edges whose destinations follow a power law
  (``N * u^3``, the longest rows hold thousands of slots), 4 relations drawn uniformly, 128 input
  channels, 4 heads of 32 channels;
* ``powerlaw_r4_within`` — the same with the softmax within every relation;
* ``powerlaw_r16`` — the same graph with 16 relations, 64 input channels, 1 head of 64 channels;
* ``sampled_r64`` — a sampled-batch-sized sparse graph (100,000 nodes, 300,000 edges, uniform end
  points) with 64 relations, 64 input channels, 2 heads of 32 channels: the ``[N, R (H C + 2 H)]``
  plane at its most wasteful.

Per shape and route: ``torch.cuda.Event``s around one forward + backward (gradients of ``x`` and
of every parameter the forward reaches: a training step of a layer inside a model) with the
layer's handles warm, median over ``--iters`` calls after ``--warmup``, the two routes alternated
twice (both medians are printed); the peak memory above the inputs of one call; the number of
C-ABI calls and of launch records (``_native.timing_sink``: the dense products go through the
compiled binding and show up there only) of one call; for the fused route the time of its
launches.  One JSON line per shape.  A route that runs out of memory is recorded as such, not
skipped silently."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_geometric_amd import _lib, _native  # noqa: E402
from pytorch_geometric_amd.nn import RGATConv  # noqa: E402

ACROSS, WITHIN = 'across-relation', 'within-relation'
SHAPES = {
    'powerlaw_r4': dict(N=200000, E=2000000, in_channels=128, R=4, H=4, C=32, graph='powerlaw',
                        mechanism=ACROSS),
    'powerlaw_r4_within': dict(N=200000, E=2000000, in_channels=128, R=4, H=4, C=32,
                               graph='powerlaw', mechanism=WITHIN),
    'powerlaw_r16': dict(N=200000, E=2000000, in_channels=64, R=16, H=1, C=64, graph='powerlaw',
                         mechanism=ACROSS),
    'sampled_r64': dict(N=100000, E=300000, in_channels=64, R=64, H=2, C=32, graph='uniform',
                        mechanism=ACROSS),
}


def edges(shape, g):
    N, E = shape['N'], shape['E']
    src = torch.randint(0, N, (E, ), generator=g)
    if shape['graph'] == 'uniform':
        dst = torch.randint(0, N, (E, ), generator=g)
    else:
        dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    return torch.stack([src, dst])


def problem(shape, dev):
    g = torch.Generator().manual_seed(1)
    N, R, H, C = shape['N'], shape['R'], shape['H'], shape['C']
    ei = edges(shape, g)
    et = torch.randint(0, R, (ei.size(1), ), generator=g)
    torch.manual_seed(2)
    conv = RGATConv(shape['in_channels'], C, R, heads=H,
                    attention_mechanism=shape['mechanism']).to(dev)
    x = torch.randn(N, shape['in_channels'], generator=g).to(dev).requires_grad_(True)
    go = torch.randn(N, H * C, generator=g).to(dev)
    deg = torch.bincount(ei[1], minlength=N)
    return conv, (x, ei.to(dev), et.to(dev), go), {'max_in_degree': int(deg.max())}


def step(conv, x, ei, et, go):
    out = conv(x, ei, et)
    torch.autograd.grad(out, [x] + [p for p in conv.parameters() if p.requires_grad], go,
                        allow_unused=True)   # (w, l1, b1, l2, b2 belong to the mod variants)
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


class _Counting:
    """stands in for the ctypes library and counts the C-ABI calls made through it"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('pygamd_') or not callable(fn):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def launches(conv, args):
    """(C-ABI calls, launch records, {rgat op: ms}) of one warm step"""
    load, counter, sink = _lib.load, _Counting(_lib.load()), []
    _lib.load, _native.timing_sink = (lambda: counter), sink
    try:
        step(conv, *args)
        torch.cuda.synchronize()
    finally:
        _lib.load, _native.timing_sink = load, None
    rgat = {}
    for i, a, b in sink:
        if i.get('kind') == 'rgat':   # (backward_src runs twice across-relation: summed)
            rgat[i['op']] = round(rgat.get(i['op'], 0.0) + a.elapsed_time(b), 4)
    return sum(counter.calls.values()), len(sink), rgat


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
        conv, args, facts = problem(SHAPES[name], dev)
        rec = {'shape': name, **SHAPES[name], **facts, 'device': torch.cuda.get_device_name(0),
               'fused_ms': [], 'generic_ms': []}
        try:
            with torch.no_grad():
                conv.fuse = True
                a = conv(*args[:3])
                conv.fuse = False
                b = conv(*args[:3])
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
            rec['generic_calls'], rec['generic_records'], _ = launches(conv, args)
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
        rec['fused_calls'], rec['fused_records'], rec['fused_kernel_ms'] = launches(conv, args)
        line = json.dumps(rec)
        print(line, flush=True)
        if opt.out:
            with open(opt.out, 'a') as f:
                f.write(line + '\n')
        del conv, args
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
