"""Generates tests/golden/golden_mixture_v1.pt by running the REAL reference (PyG) on CPU:
``GMMConv`` (nn/conv/gmm_conv.py:13-202) in eight settings and ``NNConv`` (nn/conv/nn_conv.py:13-126)
in seven.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_mixture.py

The graph is the one of make_golden_resgated.py (48 nodes, 16 features, 400 edges with skewed
destinations, empty destinations and some self-loops, a 20-node destination set for the pair
cases, whose destinations read the first 12 columns of ``x_dst``).  Every case draws its own
``edge_attr`` from its seed: pseudo-coordinates ``[400, 2]`` for GMMConv, ``[400, 3]`` edge
features for NNConv.  Tensors and constructor arguments only (an edge network as a list of
``('Linear', in, out, bias)`` / ``('ReLU', )`` entries): inputs, state dicts, outputs and the
gradients of every ``x``, of ``edge_attr`` and of every parameter.

Two things a trained layer holds and a fresh one does not: a non-zero bias, and for GMMConv
``sigma`` away from 0 (glorot draws it around 0, where ``1 / sigma^2`` makes every weight vanish
and the gradients of ``sigma`` explode): ``sigma`` is redrawn from U(0.5, 1.5) and ``mu`` from
N(0, 0.5).  The reference's GMMConv with ``root_weight=False`` never assigns ``self.root`` and its
forward then raises; the 'no_root' case sets ``conv.root = None`` on the reference object, which is
what the forward's own test (``self.root is not None``) expects.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import GMMConv, NNConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E, N_PAIR_DST, K_PAIR_DST = 48, 16, 400, 20, 12
DIM, KERNELS, DE, OUT_NN = 2, 3, 3, 8

# in_channels, out_channels, constructor arguments, x: 'one' | 'pair'
GMM_CASES = {
    'gmm_defaults': (K, K, dict(), 'one'),
    'gmm_add': (K, K, dict(aggr='add'), 'one'),
    'gmm_no_root': (K, K, dict(root_weight=False), 'one'),
    'gmm_no_bias': (K, K, dict(bias=False), 'one'),
    'gmm_wider_out': (K, 24, dict(), 'one'),
    'gmm_pair': ((K, K_PAIR_DST), K, dict(), 'pair'),
    'gmm_separate': (K, 8, dict(separate_gaussians=True), 'one'),
    'gmm_max': (K, K, dict(aggr='max'), 'one'),
}

MLP = [('Linear', DE, 10, True), ('ReLU', ), ('Linear', 10, K * OUT_NN, True)]
# in_channels, out_channels, the edge network, constructor arguments, x
NN_CASES = {
    'nn_linear': (K, OUT_NN, [('Linear', DE, K * OUT_NN, True)], dict(), 'one'),
    'nn_mlp': (K, OUT_NN, MLP, dict(), 'one'),
    'nn_last_no_bias': (K, OUT_NN, MLP[:2] + [('Linear', 10, K * OUT_NN, False)], dict(), 'one'),
    'nn_mean': (K, OUT_NN, MLP, dict(aggr='mean'), 'one'),
    'nn_pair': ((K, K_PAIR_DST), OUT_NN, MLP, dict(), 'pair'),
    'nn_max': (K, OUT_NN, MLP, dict(aggr='max'), 'one'),
    'nn_ends_relu': (K, OUT_NN, [('Linear', DE, K * OUT_NN, True), ('ReLU', )], dict(), 'one'),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_graph(seed):  # (make_golden_resgated.py's)
    g = gen(seed)
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    src[:12] = dst[:12]                                   # some self-loops
    pair_dst = (torch.rand(E, generator=g).pow(3) * N_PAIR_DST).long().clamp(max=N_PAIR_DST - 1)
    return {'x': torch.randn(N, K, generator=g), 'x_dst': torch.randn(N_PAIR_DST, K, generator=g),
            'edge_index': torch.stack([src, dst]), 'edge_index_pair': torch.stack([src, pair_dst])}


def edge_network(spec):
    layers = []
    for entry in spec:
        if entry[0] == 'Linear':
            layers.append(torch.nn.Linear(entry[1], entry[2], bias=entry[3]))
        else:
            layers.append(getattr(torch.nn, entry[0])())
    return layers[0] if len(layers) == 1 else torch.nn.Sequential(*layers)


def run(kind, cin, cout, spec, kw, mode, graph, seed):
    torch.manual_seed(seed)
    if kind == 'gmm':
        conv = GMMConv(cin, cout, dim=DIM, kernel_size=KERNELS, **kw)
        if not kw.get('root_weight', True):
            conv.root = None
        conv.sigma.data.uniform_(0.5, 1.5, generator=gen(seed + 3))
        conv.mu.data.normal_(0, 0.5, generator=gen(seed + 4))
        width = DIM
    else:
        conv = NNConv(cin, cout, edge_network(spec), **kw)
        width = DE
    if conv.bias is not None:
        conv.bias.data.normal_(0, 0.3, generator=gen(seed + 2))
    xs = [graph['x'].clone().requires_grad_(True)]
    if mode == 'pair':
        xs.append(graph['x_dst'][:, :K_PAIR_DST].clone().requires_grad_(True))
    ei = graph['edge_index'] if mode == 'one' else graph['edge_index_pair']
    ea = torch.randn(E, width, generator=gen(seed + 100)).requires_grad_(True)
    out = conv(xs[0] if mode == 'one' else (xs[0], xs[1]), ei, edge_attr=ea)
    go = torch.randn(out.shape, generator=gen(seed + 1))
    params = [(n, p) for n, p in conv.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(out, xs + [ea] + [p for _, p in params], go)
    n_x = len(xs)
    return {'kind': kind, 'in_channels': cin, 'out_channels': cout, 'kwargs': dict(kw),
            'nn': spec, 'mode': mode, 'seed': seed, 'repr': repr(conv),
            'edge_attr': ea.detach().clone(),
            'state': {k: v.detach().clone() for k, v in conv.state_dict().items()},
            'out': out.detach(), 'grad_out': go, 'grad_x': [g.detach() for g in grads[:n_x]],
            'grad_edge_attr': grads[n_x].detach(),
            'grad_params': {n: g.detach() for (n, _), g in zip(params, grads[n_x + 1:])}}


graph = make_graph(2)
deg = torch.bincount(graph['edge_index'][1], minlength=N)
assert int((deg == 0).sum()) > 0 and int(deg.max()) > 40

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'N': N, 'K': K,
              'dim': DIM, 'kernel_size': KERNELS},
     **graph, 'cases': {}}
for i, (name, (cin, cout, kw, mode)) in enumerate(GMM_CASES.items()):
    G['cases'][name] = run('gmm', cin, cout, None, kw, mode, graph, 12000 + 200 * i)
for i, (name, (cin, cout, spec, kw, mode)) in enumerate(NN_CASES.items()):
    G['cases'][name] = run('nn', cin, cout, spec, kw, mode, graph, 16000 + 200 * i)
for name, case in G['cases'].items():
    print(f"{name}: out {tuple(case['out'].shape)}  |out| max "
          f"{float(case['out'].abs().max()):.3f}  params {list(case['grad_params'])}")

out_path = os.path.join(HERE, 'golden_mixture_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
