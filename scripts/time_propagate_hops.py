"""Forward + backward of the layers built on the propagation step of csrc/hop.hip (APPNP, SGConv,
SSGConv, TAGConv, LGConv, a stack of GCN2Conv) against what a user of this package writes WITHOUT
them: a ``MessagePassing.propagate`` per step on the normalised handle plus torch arithmetic, in the
reference's order (appnp.py:111-133, sg_conv.py:93-95, ssg_conv.py:102-106, tag_conv.py:87-91,
lg_conv.py:50, gcn2_conv.py:138-153).
The baseline leg uses only names that exist before the layers were added (``MessagePassing``,
``gcn_norm``, ``EdgeIndex``, ``_functions.spmm_node``, ``nn.Linear``), so it can be run on an older
checkout for cross-checking: ``--baseline-only``.

    python scripts/time_propagate_hops.py [--reps 20] [--out FILE] [--only NAME] [--baseline-only]

Both legs get the graph as a handle and are normalised ONCE (the layers keep the normalised graph
with the handle, the baseline normalises before the loop), share their parameters, alternate inside
one process and are timed with device events around ``reps`` calls after a warm-up of every shape
and leg.  Per shape the script also times a streaming read + write of one ``[N, F]`` plane (``y = 2
x``, two plane passes) in the same run, and counts, for ONE forward + backward of each leg, the
package's launches (the records of ``_native.timing_sink``) and the torch operators that produce a
plane of ``N x F`` elements or more in the forward.

The store hint of ``out``: build with ``PYGAMD_EXTRA_HIPCC_FLAGS=-DPYGAMD_HOP_NT_STORE=1`` and run
again; the rows then carry ``"nt_store": true``."""
import argparse
import json
import math
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_geometric_amd.nn as nn  # noqa: E402
from pytorch_geometric_amd import _native  # noqa: E402
from pytorch_geometric_amd._functions import spmm_node  # noqa: E402
from pytorch_geometric_amd.edge_index import EdgeIndex  # noqa: E402


class Propagate(nn.MessagePassing):
    """One weighted sum aggregation, as a user's own layer: the CSR SpMM of the package"""

    def __init__(self):
        super().__init__(aggr='add')

    def forward(self, x, graph, w):
        return self.propagate(graph, x=x, edge_weight=w)

    def message(self, x_j, edge_weight):
        return edge_weight.view(-1, 1) * x_j

    def message_and_aggregate(self, graph, x, edge_weight):
        return spmm_node(x, edge_weight, graph, 'sum', 'coo')


def normalised(ei, n, add_self_loops):
    """(handle, weights) of D^-1/2 (A [+ I]) D^-1/2, once"""
    ei2, w = nn.gcn_norm(ei, None, n, False, add_self_loops)
    return EdgeIndex(ei2, (n, n), validate=False), w


# ---- the baseline legs: the reference's loops --------------------------------------------------------
def appnp_baseline(prop, K, alpha):
    def run(x, graph, w):
        h = x
        for _ in range(K):
            x = prop(x, graph, w)
            x = x * (1 - alpha)
            x = x + alpha * h
        return x
    return run


def sg_baseline(prop, K, lin):
    def run(x, graph, w):
        for _ in range(K):
            x = prop(x, graph, w)
        return lin(x)
    return run


def ssg_baseline(prop, K, alpha, lin):
    def run(x, graph, w):
        h = x * alpha
        for _ in range(K):
            x = prop(x, graph, w)
            h = h + (1 - alpha) / K * x
        return lin(h)
    return run


def lg_baseline(prop):
    def run(x, graph, w):
        return prop(x, graph, w)
    return run


def tag_baseline(prop, lins, bias):
    def run(x, graph, w):
        out = lins[0](x)
        for lin in lins[1:]:
            x = prop(x, graph, w)
            out = out + lin(x)
        return out + bias
    return run


def gcn2_baseline(prop, weights, alpha, betas):
    def run(x, graph, w):
        x_0 = x
        for weight, beta in zip(weights, betas):
            h = prop(x, graph, w)
            h = h * (1 - alpha)
            h = h + alpha * x_0
            x = torch.addmm(h, h, weight, beta=1. - beta, alpha=beta).relu()
        return x
    return run


# ---- shapes ------------------------------------------------------------------------------------------
def uniform_graph(n, e, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n, (e, ), generator=g),
                        torch.randint(0, n, (e, ), generator=g)]).to(dev)


def power_law_graph(n, e, seed, dev):
    g = torch.Generator().manual_seed(seed)
    dst = (torch.rand(e, generator=g).pow(6) * n).long().clamp(max=n - 1)
    return torch.stack([torch.randint(0, n, (e, ), generator=g), dst]).to(dev)


class Gcn2Stack(torch.nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = torch.nn.ModuleList(layers)

    def forward(self, x, graph):
        x_0 = x
        for layer in self.layers:
            x = layer(x, x_0, graph).relu()
        return x


def cases(dev):
    """name, edge list, N, F, the baseline leg, a builder of the fused layer (called with x and the
    raw handle) on the SAME parameters, self-loops of the normalisation.  The parameters are made
    with names every checkout has; the fused layer is built only when it is asked for."""
    torch.manual_seed(0)
    prop = Propagate()

    def appnp():
        return nn.APPNP(10, 0.1)

    cora = uniform_graph(2708, 10_556, 1, dev)
    yield 'cora-like APPNP K=10', cora, 2708, 7, appnp_baseline(prop, 10, 0.1), appnp, True
    arxiv = uniform_graph(169_343, 2_315_598, 2, dev)
    yield 'arxiv-like APPNP K=10', arxiv, 169_343, 40, appnp_baseline(prop, 10, 0.1), appnp, True
    power = power_law_graph(250_000, 2_000_000, 3, dev)
    lin = nn.Linear(128, 16).to(dev)

    def sg():
        layer = nn.SGConv(128, 16, K=2).to(dev)
        layer.lin = lin
        return layer

    yield 'power-law SGConv K=2 128->16', power, 250_000, 128, sg_baseline(prop, 2, lin), sg, True

    def ssg():
        layer = nn.SSGConv(128, 16, alpha=0.1, K=2).to(dev)
        layer.lin = lin
        return layer

    yield 'power-law SSGConv K=2 128->16', power, 250_000, 128, \
        ssg_baseline(prop, 2, 0.1, lin), ssg, True
    yield 'arxiv-like LGConv', arxiv, 169_343, 40, lg_baseline(prop), lambda: nn.LGConv(), False
    yield 'power-law LGConv F=128', power, 250_000, 128, lg_baseline(prop), \
        lambda: nn.LGConv(), False
    lins = torch.nn.ModuleList([nn.Linear(128, 16, bias=False) for _ in range(4)]).to(dev)
    bias = torch.nn.Parameter(torch.zeros(16, device=dev))

    def tag():
        layer = nn.TAGConv(128, 16, K=3).to(dev)
        layer.lins, layer.bias = lins, bias
        return layer

    yield 'power-law TAGConv K=3 128->16', power, 250_000, 128, tag_baseline(prop, lins, bias), \
        tag, False
    weights = [torch.nn.Parameter(torch.empty(64, 64, device=dev).uniform_(-0.2, 0.2))
               for _ in range(64)]
    betas = [math.log(0.5 / (i + 1) + 1) for i in range(64)]

    def gcn2():
        layers = [nn.GCN2Conv(64, 0.1, theta=0.5, layer=i + 1).to(dev) for i in range(64)]
        for layer, weight in zip(layers, weights):
            layer.weight1 = weight
        return Gcn2Stack(layers)

    yield 'arxiv-like 64 x GCN2Conv F=64', arxiv, 169_343, 64, \
        gcn2_baseline(prop, weights, 0.1, betas), gcn2, True


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


class Planes(TorchDispatchMode):
    """torch operators whose result has at least ``numel`` elements (allocations and views aside)"""
    FREE = ('empty', 'empty_like', 'empty_strided', 'new_empty', 'view', '_unsafe_view', 'reshape',
            'alias', 'detach', 'as_strided', 'slice', 'select', 'expand', 't', 'transpose',
            'permute', 'unsqueeze', 'squeeze', 'narrow', 'split', 'split_with_sizes')

    def __init__(self, numel):
        super().__init__()
        self.numel, self.count = numel, 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if (isinstance(out, torch.Tensor) and out.numel() >= self.numel
                and func.overloadpacket.__name__ not in self.FREE):
            self.count += 1
        return out


def counts(step, forward, numel):
    """(the package's launches of one forward + backward, torch plane operators of one forward)"""
    sink = []
    _native.timing_sink = sink
    try:
        step()
        torch.cuda.synchronize()
    finally:
        _native.timing_sink = None
    kinds = {}
    for info, _, _ in sink:
        kind = info.get('kind', 'spmm' if 'reduce' in info else 'other')
        kinds[kind] = kinds.get(kind, 0) + 1
    with torch.no_grad(), Planes(numel) as planes:
        forward()
    return kinds, planes.count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', default=None)
    ap.add_argument('--baseline-only', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    nt = 'PYGAMD_HOP_NT_STORE' in os.environ.get('PYGAMD_EXTRA_HIPCC_FLAGS', '')
    rows = []
    for name, ei, n, F, baseline, make_layer, loops in cases(dev):
        if args.only is not None and args.only not in name:
            continue
        x = torch.randn(n, F, device=dev).requires_grad_(True)
        raw = EdgeIndex(ei, (n, n))
        graph, w = normalised(ei, n, loops)
        graph.fill_cache_()
        layer = None
        if not args.baseline_only:
            layer = make_layer()
            for m in layer.modules():
                if hasattr(m, 'fuse'):
                    m.fuse = True
        go = torch.randn_like(baseline(x, graph, w).detach())
        plane = x.detach()

        def fused_step():
            x.grad = None
            layer(x, raw).backward(go)

        def baseline_step():
            x.grad = None
            baseline(x, graph, w).backward(go)

        row = {'shape': name, 'N': n, 'E': ei.size(1), 'F': F, 'nt_store': nt,
               'copy_ms': timed(lambda: torch.mul(plane, 2.0), args.reps)}
        legs = [('baseline', baseline_step, lambda: baseline(x, graph, w))]
        if not args.baseline_only:
            legs.insert(0, ('fused', fused_step, lambda: layer(x, raw)))
            got, want = layer(x, raw), baseline(x, graph, w)
            row['max_abs_diff'] = float((got - want).detach().abs().max())
            row['scale'] = float(want.detach().abs().max())
        for _ in range(2):                      # the legs alternate; the second round is reported
            for leg, step, _ in legs:
                row[f'{leg}_ms'] = timed(step, args.reps)
        for leg, step, forward in legs:
            row[f'{leg}_launches'], row[f'{leg}_plane_ops_forward'] = counts(step, forward, n * F)
        if not args.baseline_only:
            row['ratio'] = row['baseline_ms'] / row['fused_ms']
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
