"""Generates tests/golden/golden_gin_v1.pt by running the REAL reference (PyG) on CPU: ``GINConv``
and ``GINEConv`` (nn/conv/gin_conv.py:19-207) in ten settings.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_gin.py

The graph is the one of make_golden_transformer_edge.py (48 nodes, 16 features, 400 edges with
skewed destinations and some self-loops, a 20-node destination set for the pair cases, here of the
same width 16); ``nn = Sequential(Linear(16, 12), ReLU(), Linear(12, 8))``.  Every GINE case draws
its own ``edge_attr [400, 16]`` from its seed (a case with ``edge_dim = D`` reads the first ``D``
columns).  An fp32 kernel may round a pre-activation ``x_j + e`` across zero, which flips a mask
and changes a gradient by a whole ``grad_out`` entry: the pre-activations are formed in float64 and
a case's seed is advanced until ``min |pre| >= 1e-4`` (two orders above fp32 rounding at these
magnitudes); the seed that was taken is recorded.  Tensors only: inputs, state dicts, outputs and
the gradients of every ``x``, of ``edge_attr`` and of every parameter.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import GINConv, GINEConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E, N_PAIR_DST = 48, 16, 400, 20
MARGIN = 1e-4

# kind, constructor arguments, x: 'one' | 'pair' | 'pair_none'
CASES = {
    'gin': ('gin', dict(), 'one'),
    'gin_eps': ('gin', dict(eps=0.3, train_eps=True), 'one'),
    'gin_pair': ('gin', dict(), 'pair'),
    'gin_pair_none': ('gin', dict(), 'pair_none'),
    'gine': ('gine', dict(), 'one'),
    'gine_eps': ('gine', dict(eps=0.3, train_eps=True), 'one'),
    'gine_lin': ('gine', dict(edge_dim=3), 'one'),
    'gine_lin_wide': ('gine', dict(edge_dim=9), 'one'),
    'gine_lin_pair': ('gine', dict(edge_dim=3), 'pair'),
    'gine_pair_none': ('gine', dict(), 'pair_none'),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_graph(seed):
    g = gen(seed)
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    src[:12] = dst[:12]                                   # some self-loops
    pair_dst = (torch.rand(E, generator=g).pow(3) * N_PAIR_DST).long().clamp(max=N_PAIR_DST - 1)
    return {'x': torch.randn(N, K, generator=g), 'x_dst': torch.randn(N_PAIR_DST, K, generator=g),
            'edge_index': torch.stack([src, dst]), 'edge_index_pair': torch.stack([src, pair_dst])}


def make_nn():
    return torch.nn.Sequential(torch.nn.Linear(K, 12), torch.nn.ReLU(), torch.nn.Linear(12, 8))


def run_conv(kind, kw, mode, graph, seed):
    torch.manual_seed(seed)
    conv = (GINConv if kind == 'gin' else GINEConv)(make_nn(), **kw)
    xs = [graph['x'].clone().requires_grad_(True)]
    if mode == 'pair':
        xs.append(graph['x_dst'].clone().requires_grad_(True))
    ei = graph['edge_index'] if mode == 'one' else graph['edge_index_pair']
    size = None if mode == 'one' else (N, N_PAIR_DST)
    x_in = xs[0] if mode == 'one' else (xs[0], xs[1] if mode == 'pair' else None)
    case = {'kind': kind, 'kwargs': dict(kw), 'mode': mode, 'seed': seed}
    leaves = list(xs)
    if kind == 'gine':
        D = kw.get('edge_dim') or K
        ea = torch.randn(E, K, generator=gen(seed + 100))[:, :D].clone().requires_grad_(True)
        # the margin of the ReLU's argument, in float64
        e64 = ea.detach().double()
        if conv.lin is not None:
            e64 = e64 @ conv.lin.weight.detach().double().t() + conv.lin.bias.detach().double()
        pre = graph['x'].double()[ei[0]] + e64
        case['margin'] = float(pre.abs().min())
        if case['margin'] < MARGIN:
            return None
        out = conv(x_in, ei, edge_attr=ea, size=size)
        case['edge_attr'] = ea.detach().clone()
        leaves.append(ea)
    else:
        out = conv(x_in, ei, size=size)
    go = torch.randn(out.shape, generator=gen(seed + 1))
    names = [n for n, _ in conv.named_parameters()]
    grads = torch.autograd.grad(out, leaves + [p for _, p in conv.named_parameters()], go)
    nx = len(xs)
    case.update({'state': {k: v.detach().clone() for k, v in conv.state_dict().items()},
                 'out': out.detach(), 'grad_out': go,
                 'grad_x': [g.detach() for g in grads[:nx]],
                 'grad_params': {n: g.detach() for n, g in zip(names, grads[len(leaves):])}})
    if kind == 'gine':
        case['grad_edge_attr'] = grads[nx].detach()
    return case


graph = make_graph(2)
deg = torch.bincount(graph['edge_index'][1], minlength=N)
assert int((deg == 0).sum()) > 0 and int(deg.max()) > 40

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'N': N, 'K': K,
              'margin': MARGIN}, **graph, 'cases': {}}
for i, (name, (kind, kw, mode)) in enumerate(CASES.items()):
    seed = 5000 + 200 * i
    case = run_conv(kind, kw, mode, graph, seed)
    while case is None:
        seed += 1
        case = run_conv(kind, kw, mode, graph, seed)
    G['cases'][name] = case
    assert ('eps' in case['grad_params']) == bool(kw.get('train_eps')), name
    assert ('lin.weight' in case['grad_params']) == ('edge_dim' in kw), name
    assert kind == 'gin' or case['margin'] >= MARGIN
    print(f"{name}: seed {case['seed']}  out {tuple(case['out'].shape)}  |out| max "
          f"{float(case['out'].abs().max()):.3f}  margin {case.get('margin')}")

out_path = os.path.join(HERE, 'golden_gin_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
