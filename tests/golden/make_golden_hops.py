"""Generates tests/golden/golden_hops_v1.pt by running the REAL reference (PyG) on CPU: ``APPNP``,
``SGConv``, ``SSGConv``, ``TAGConv``, ``LGConv`` and ``GCN2Conv`` (nn/conv/appnp.py, sg_conv.py,
ssg_conv.py, tag_conv.py, lg_conv.py, gcn2_conv.py) in their default settings and in the settings
that change the route or the arithmetic, and one 3-layer stack with ReLU.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_hops.py

The graph is the one of make_golden_gin.py (48 nodes, 16 features, 400 edges with skewed
destinations, destinations without edges and some self-loops).  A case names the class, its
constructor arguments and what it is called with: the feature width (16, or the first 4 columns),
given positive edge weights (which then take a gradient), a second call with other features and
the flipped edge list (``cached``: what the cache holds decides the second result), a longer
``x_0``.  The stack's ReLU arguments are formed in float64 and its seed is advanced until ``min
|pre| >= 1e-4`` (the rule of make_golden_cg.py); the seed that was taken is recorded.  Tensors and
constructor arguments only: inputs, state dicts, outputs, the gradients of ``x``, ``x_0``, the given
``edge_weight`` and every parameter, and ``repr``.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric import nn as ref_nn  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E, N_X0 = 48, 16, 400, 56
MARGIN = 1e-4

# name: (class, constructor arguments, options).  Options: width (default 16), weights (given edge
# weights), calls (default 1), x0_rows (GCN2Conv: rows of x_0, default N)
CASES = {
    'appnp': ('APPNP', dict(K=10, alpha=0.1), {}),
    'appnp_k1': ('APPNP', dict(K=1, alpha=0.2), {}),
    'appnp_given': ('APPNP', dict(K=3, alpha=0.1, normalize=False), {'weights': True}),
    'appnp_given_norm': ('APPNP', dict(K=3, alpha=0.1), {'weights': True}),
    'appnp_no_loops': ('APPNP', dict(K=10, alpha=0.1, add_self_loops=False), {}),
    'appnp_cached': ('APPNP', dict(K=10, alpha=0.1, cached=True), {'calls': 2}),
    'appnp_mean': ('APPNP', dict(K=3, alpha=0.1, aggr='mean'), {}),
    'sg_k1': ('SGConv', dict(in_channels=16, out_channels=4), {}),
    'sg_k3': ('SGConv', dict(in_channels=16, out_channels=4, K=3), {}),
    'sg_k3_wide': ('SGConv', dict(in_channels=4, out_channels=16, K=3), {'width': 4}),
    'sg_cached': ('SGConv', dict(in_channels=16, out_channels=4, K=3, cached=True), {'calls': 2}),
    'sg_no_bias': ('SGConv', dict(in_channels=16, out_channels=4, K=3, bias=False), {}),
    'sg_mean': ('SGConv', dict(in_channels=16, out_channels=4, K=3, aggr='mean'), {}),
    'ssg_k1': ('SSGConv', dict(in_channels=16, out_channels=4, alpha=0.2), {}),
    'ssg_k3': ('SSGConv', dict(in_channels=16, out_channels=4, alpha=0.2, K=3), {}),
    'ssg_k3_wide': ('SSGConv', dict(in_channels=4, out_channels=16, alpha=0.2, K=3), {'width': 4}),
    'ssg_cached': ('SSGConv', dict(in_channels=16, out_channels=4, alpha=0.2, K=3, cached=True),
                   {'calls': 2}),
    'ssg_no_bias': ('SSGConv', dict(in_channels=16, out_channels=4, alpha=0.2, K=3, bias=False), {}),
    'ssg_mean': ('SSGConv', dict(in_channels=16, out_channels=4, alpha=0.2, K=3, aggr='mean'), {}),
    'tag_k0': ('TAGConv', dict(in_channels=16, out_channels=4, K=0), {}),
    'tag_k3': ('TAGConv', dict(in_channels=16, out_channels=4, K=3), {}),
    'tag_k3_wide': ('TAGConv', dict(in_channels=4, out_channels=16, K=3), {'width': 4}),
    'tag_given': ('TAGConv', dict(in_channels=16, out_channels=4, K=3, normalize=False),
                  {'weights': True}),
    'tag_no_bias': ('TAGConv', dict(in_channels=16, out_channels=4, K=2, bias=False), {}),
    'tag_mean': ('TAGConv', dict(in_channels=16, out_channels=4, K=3, aggr='mean'), {}),
    'lg': ('LGConv', dict(), {}),
    'lg_given': ('LGConv', dict(), {'weights': True}),
    'lg_given_raw': ('LGConv', dict(normalize=False), {'weights': True}),
    'gcn2_shared': ('GCN2Conv', dict(channels=16, alpha=0.1), {}),
    'gcn2_separate': ('GCN2Conv', dict(channels=16, alpha=0.1, shared_weights=False), {}),
    'gcn2_theta': ('GCN2Conv', dict(channels=16, alpha=0.2, theta=0.5, layer=2), {}),
    'gcn2_theta_separate': ('GCN2Conv', dict(channels=16, alpha=0.2, theta=0.5, layer=3,
                                             shared_weights=False), {}),
    'gcn2_x0_rows': ('GCN2Conv', dict(channels=16, alpha=0.1, theta=0.5, layer=1),
                     {'x0_rows': N_X0}),
    'gcn2_cached': ('GCN2Conv', dict(channels=16, alpha=0.1, cached=True), {'calls': 2}),
}

# the stack: (class, constructor arguments) with a ReLU between the layers
STACK = [('TAGConv', dict(in_channels=16, out_channels=8, K=2)),
         ('SGConv', dict(in_channels=8, out_channels=12, K=2)),
         ('APPNP', dict(K=3, alpha=0.1))]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_graph(seed):
    g = gen(seed)
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    src[:12] = dst[:12]                                   # some self-loops
    return {'x': torch.randn(N, K, generator=g), 'x2': torch.randn(N, K, generator=g),
            'x_0': torch.randn(N_X0, K, generator=g), 'edge_index': torch.stack([src, dst]),
            'edge_weight': torch.rand(E, generator=g) + 0.5}


def run_case(cls, kw, opt, graph, seed):
    torch.manual_seed(seed)
    conv = getattr(ref_nn, cls)(**kw)
    width = opt.get('width', K)
    case = {'cls': cls, 'kwargs': dict(kw), 'options': dict(opt), 'seed': seed,
            'repr': repr(conv),
            'state': {k: v.detach().clone() for k, v in conv.state_dict().items()}, 'calls': []}
    names = [n for n, _ in conv.named_parameters()]
    params = [p for _, p in conv.named_parameters()]
    for call in range(opt.get('calls', 1)):
        x = graph['x' if call == 0 else 'x2'][:, :width].clone().requires_grad_(True)
        ei = graph['edge_index'] if call == 0 else graph['edge_index'].flip(0)
        leaves, args = {'x': x}, [x]
        if cls == 'GCN2Conv':
            x_0 = graph['x_0'][:opt.get('x0_rows', N)].clone().requires_grad_(True)
            leaves['x_0'] = x_0
            args.append(x_0)
        args.append(ei)
        if opt.get('weights'):
            w = graph['edge_weight'].clone().requires_grad_(True)
            leaves['edge_weight'] = w
            args.append(w)
        out = conv(*args)
        go = torch.randn(out.shape, generator=gen(seed + 1 + call))
        grads = torch.autograd.grad(out, list(leaves.values()) + params, go, allow_unused=True)
        rec = {'out': out.detach().clone(), 'grad_out': go}
        for name, g in zip(list(leaves) + [f'param {n}' for n in names], grads):
            rec[f'grad {name}'] = None if g is None else g.detach().clone()
        case['calls'].append(rec)
    return case


def run_stack(graph, seed):
    torch.manual_seed(seed)
    layers = [getattr(ref_nn, cls)(**kw) for cls, kw in STACK]
    x = graph['x'].clone().requires_grad_(True)
    h, margin = x, float('inf')
    for i, conv in enumerate(layers):
        h = conv(h, graph['edge_index'])
        if i + 1 < len(layers):
            margin = min(margin, float(h.detach().double().abs().min()))
            h = h.relu()
    if margin < MARGIN:
        return None
    go = torch.randn(h.shape, generator=gen(seed + 1))
    params = [(f'{i}.{n}', p) for i, conv in enumerate(layers) for n, p in conv.named_parameters()]
    grads = torch.autograd.grad(h, [x] + [p for _, p in params], go)
    return {'layers': [(cls, dict(kw)) for cls, kw in STACK], 'seed': seed, 'margin': margin,
            'state': [{k: v.detach().clone() for k, v in conv.state_dict().items()}
                      for conv in layers],
            'out': h.detach().clone(), 'grad_out': go, 'grad x': grads[0].detach().clone(),
            'grad_params': {n: g.detach().clone() for (n, _), g in zip(params, grads[1:])}}


graph = make_graph(2)
deg = torch.bincount(graph['edge_index'][1], minlength=N)
assert int((deg == 0).sum()) > 0 and int(deg.max()) > 40

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'N': N, 'K': K,
              'margin': MARGIN}, **graph, 'cases': {}}
for i, (name, (cls, kw, opt)) in enumerate(CASES.items()):
    case = run_case(cls, kw, opt, graph, 7000 + 10 * i)
    G['cases'][name] = case
    out = case['calls'][-1]['out']
    print(f"{name}: {case['repr']}  out {tuple(out.shape)}  |out| max {float(out.abs().max()):.3f}")

seed = 9000
stack = run_stack(graph, seed)
while stack is None:
    seed += 1
    stack = run_stack(graph, seed)
G['stack'] = stack
print(f"stack: seed {stack['seed']}  margin {stack['margin']:.2e}")

out_path = os.path.join(HERE, 'golden_hops_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
