"""Generates tests/golden/golden_resgated_v1.pt by running the REAL reference (PyG) on CPU:
``ResGatedGraphConv`` (nn/conv/res_gated_graph_conv.py:13-148) in nine settings and one two-layer
stack with a ReLU between.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_resgated.py

The graph is the one of make_golden_gin.py (48 nodes, 16 features, 400 edges with skewed
destinations, empty destinations and some self-loops, a 20-node destination set for the pair
cases, whose destinations read the first 12 columns of ``x_dst``).  A case with ``edge_dim = D``
draws its own ``edge_attr [400, D]`` from its seed.  Tensors only (and each case's constructor
arguments; a gate other than the sigmoid by its class name): inputs, state dicts, outputs and the
gradients of every ``x``, of ``edge_attr`` and of every parameter.  An fp32 kernel may round the
argument of the stack's ReLU across zero, which flips a mask and changes a gradient by a whole
entry: the stack's seed is advanced until ``min |pre| >= 1e-4`` and the seed taken is recorded.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import ResGatedGraphConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E, N_PAIR_DST, K_PAIR_DST = 48, 16, 400, 20, 12
MARGIN = 1e-4

# in_channels, out_channels, constructor arguments, gate (None: the default sigmoid), x: 'one' | 'pair'
CASES = {
    'defaults': (K, K, dict(), None, 'one'),
    'no_root': (K, K, dict(root_weight=False), None, 'one'),
    'no_bias': (K, K, dict(bias=False), None, 'one'),
    'wider_out': (K, 24, dict(), None, 'one'),
    'edge_dim': (K, K, dict(edge_dim=3), None, 'one'),
    'pair': ((K, K_PAIR_DST), K, dict(), None, 'pair'),
    'pair_edge_dim': ((K, K_PAIR_DST), 8, dict(edge_dim=3), None, 'pair'),
    'tanh': (K, K, dict(), 'Tanh', 'one'),
    'mean': (K, K, dict(aggr='mean'), None, 'one'),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_graph(seed):  # (make_golden_gin.py's)
    g = gen(seed)
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    src[:12] = dst[:12]                                   # some self-loops
    pair_dst = (torch.rand(E, generator=g).pow(3) * N_PAIR_DST).long().clamp(max=N_PAIR_DST - 1)
    return {'x': torch.randn(N, K, generator=g), 'x_dst': torch.randn(N_PAIR_DST, K, generator=g),
            'edge_index': torch.stack([src, dst]), 'edge_index_pair': torch.stack([src, pair_dst])}


def record(case, module, out, leaves, n_x, seed):
    go = torch.randn(out.shape, generator=gen(seed + 1))
    params = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(out, leaves + [p for _, p in params], go)
    case.update({'state': {k: v.detach().clone() for k, v in module.state_dict().items()},
                 'out': out.detach(), 'grad_out': go,
                 'grad_x': [g.detach() for g in grads[:n_x]],
                 'grad_params': {n: g.detach() for (n, _), g in zip(params, grads[len(leaves):])}})
    if len(leaves) > n_x:
        case['grad_edge_attr'] = grads[n_x].detach()
    return case


def run_conv(cin, cout, kw, act, mode, graph, seed):
    torch.manual_seed(seed)
    extra = {} if act is None else {'act': getattr(torch.nn, act)()}
    conv = ResGatedGraphConv(cin, cout, **kw, **extra)
    # (the reference zeroes the bias; a non-zero one is what a trained layer holds)
    if conv.bias is not None:
        conv.bias.data.normal_(0, 0.3, generator=gen(seed + 2))
    xs = [graph['x'].clone().requires_grad_(True)]
    if mode == 'pair':
        xs.append(graph['x_dst'][:, :K_PAIR_DST].clone().requires_grad_(True))
    ei = graph['edge_index'] if mode == 'one' else graph['edge_index_pair']
    case = {'in_channels': cin, 'out_channels': cout, 'kwargs': dict(kw), 'act': act,
            'mode': mode, 'seed': seed, 'repr': repr(conv)}
    leaves = list(xs)
    ea = None
    if kw.get('edge_dim'):
        ea = torch.randn(E, kw['edge_dim'], generator=gen(seed + 100)).requires_grad_(True)
        case['edge_attr'] = ea.detach().clone()
        leaves.append(ea)
    out = conv(xs[0] if mode == 'one' else (xs[0], xs[1]), ei, edge_attr=ea)
    return record(case, conv, out, leaves, len(xs), seed)


def make_stack():
    return torch.nn.ModuleList([ResGatedGraphConv(K, 24, edge_dim=3), ResGatedGraphConv(24, K)])


def run_stack(graph, seed):
    torch.manual_seed(seed)
    layers = make_stack()
    for i, layer in enumerate(layers):
        layer.bias.data.normal_(0, 0.3, generator=gen(seed + 2 + i))
    x = graph['x'].clone().requires_grad_(True)
    ea = torch.randn(E, 3, generator=gen(seed + 100)).requires_grad_(True)
    pre = layers[0](x, graph['edge_index'], edge_attr=ea)
    h = layers[1](pre.relu(), graph['edge_index'])
    case = {'seed': seed, 'edge_attr': ea.detach().clone(),
            'margin': float(pre.detach().abs().min())}
    if case['margin'] < MARGIN:
        return None
    return record(case, layers, h, [x, ea], 1, seed)


graph = make_graph(2)
deg = torch.bincount(graph['edge_index'][1], minlength=N)
assert int((deg == 0).sum()) > 0 and int(deg.max()) > 40

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'N': N, 'K': K},
     **graph, 'cases': {}}
for i, (name, (cin, cout, kw, act, mode)) in enumerate(CASES.items()):
    case = run_conv(cin, cout, kw, act, mode, graph, 8000 + 200 * i)
    G['cases'][name] = case
    print(f"{name}: out {tuple(case['out'].shape)}  |out| max "
          f"{float(case['out'].abs().max()):.3f}  params {list(case['grad_params'])}")
seed = 9900
stack = run_stack(graph, seed)
while stack is None:
    seed += 1
    stack = run_stack(graph, seed)
G['stack'] = stack
print(f"stack: seed {stack['seed']}  margin {stack['margin']:.2e}  keys {len(stack['state'])}")

out_path = os.path.join(HERE, 'golden_resgated_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
