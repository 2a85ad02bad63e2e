"""Generates tests/golden/golden_cg_v1.pt by running the REAL reference (PyG) on CPU: ``CGConv``
(nn/conv/cg_conv.py:12-101) in nine settings and one two-layer stack with a ReLU between.  Build
container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_cg.py

The graph is the one of make_golden_resgated.py (48 nodes, 16 features, 400 edges with skewed
destinations, empty destinations and some self-loops, a 20-node destination set for the pair
cases, whose destinations read the first 12 columns of ``x_dst``).  A case with ``dim = D`` draws
its own ``edge_attr [400, D]`` from its seed; ``dim = 41`` at 16 channels lies past the envelope
in which the kernels keep the edge matrices in registers.  The ``batch_norm`` case runs in
training mode with drawn affine parameters; its state dict is recorded BEFORE the forward and the
running statistics after it separately.  Tensors only (and each case's constructor arguments):
inputs, state dicts, outputs and the gradients of every ``x``, of ``edge_attr`` and of every
parameter.  The file is 601,848 bytes, twice golden_resgated_v1.pt: the ``dim = 41`` case alone
holds ``edge_attr`` and its gradient at ``[400, 41]`` (131 KB), and there are ten records.  An
fp32 kernel may round the argument of the stack's ReLU across zero, which flips a mask and changes
a gradient by a whole entry: the stack's seed is advanced until ``min |pre| >= 1e-4`` and the seed
taken is recorded.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import CGConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E, N_PAIR_DST, K_PAIR_DST = 48, 16, 400, 20, 12
MARGIN = 1e-4

# channels, constructor arguments, x: 'one' | 'pair'
CASES = {
    'defaults': (K, dict(), 'one'),
    'no_bias': (K, dict(bias=False), 'one'),
    'dim': (K, dict(dim=3), 'one'),
    'dim_wide': (K, dict(dim=41), 'one'),
    'mean': (K, dict(aggr='mean'), 'one'),
    'max': (K, dict(aggr='max'), 'one'),
    'batch_norm': (K, dict(batch_norm=True), 'one'),
    'pair': ((K, K_PAIR_DST), dict(), 'pair'),
    'pair_dim': ((K, K_PAIR_DST), dict(dim=3, aggr='mean'), 'pair'),
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


def record(case, module, state, out, leaves, n_x, seed):
    go = torch.randn(out.shape, generator=gen(seed + 1))
    params = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(out, leaves + [p for _, p in params], go)
    case.update({'state': state, 'out': out.detach(), 'grad_out': go,
                 'grad_x': [g.detach() for g in grads[:n_x]],
                 'grad_params': {n: g.detach() for (n, _), g in zip(params, grads[len(leaves):])}})
    if len(leaves) > n_x:
        case['grad_edge_attr'] = grads[n_x].detach()
    return case


def snapshot(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def run_conv(channels, kw, mode, graph, seed):
    torch.manual_seed(seed)
    conv = CGConv(channels, **kw)
    conv.train()
    if conv.bn is not None:  # (what a trained layer holds)
        conv.bn.weight.data.normal_(1.0, 0.2, generator=gen(seed + 2))
        conv.bn.bias.data.normal_(0, 0.3, generator=gen(seed + 3))
    xs = [graph['x'].clone().requires_grad_(True)]
    if mode == 'pair':
        xs.append(graph['x_dst'][:, :K_PAIR_DST].clone().requires_grad_(True))
    ei = graph['edge_index'] if mode == 'one' else graph['edge_index_pair']
    case = {'channels': channels, 'kwargs': dict(kw), 'mode': mode, 'seed': seed,
            'repr': repr(conv)}
    leaves = list(xs)
    ea = None
    if kw.get('dim'):
        ea = torch.randn(E, kw['dim'], generator=gen(seed + 100)).requires_grad_(True)
        case['edge_attr'] = ea.detach().clone()
        leaves.append(ea)
    state = snapshot(conv)
    out = conv(xs[0] if mode == 'one' else (xs[0], xs[1]), ei, edge_attr=ea)
    if conv.bn is not None:
        case['bn_after'] = {k: v for k, v in snapshot(conv).items() if k.startswith('bn.running')}
    return record(case, conv, state, out, leaves, len(xs), seed)


def make_stack():
    return torch.nn.ModuleList([CGConv(K, dim=3), CGConv(K)])


def run_stack(graph, seed):
    torch.manual_seed(seed)
    layers = make_stack()
    x = graph['x'].clone().requires_grad_(True)
    ea = torch.randn(E, 3, generator=gen(seed + 100)).requires_grad_(True)
    pre = layers[0](x, graph['edge_index'], edge_attr=ea)
    h = layers[1](pre.relu(), graph['edge_index'])
    case = {'seed': seed, 'edge_attr': ea.detach().clone(),
            'margin': float(pre.detach().abs().min())}
    if case['margin'] < MARGIN:
        return None
    return record(case, layers, snapshot(layers), h, [x, ea], 1, seed)


graph = make_graph(2)
deg = torch.bincount(graph['edge_index'][1], minlength=N)
assert int((deg == 0).sum()) > 0 and int(deg.max()) > 40

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'N': N, 'K': K},
     **graph, 'cases': {}}
for i, (name, (channels, kw, mode)) in enumerate(CASES.items()):
    case = run_conv(channels, kw, mode, graph, 8500 + 200 * i)
    G['cases'][name] = case
    print(f"{name}: out {tuple(case['out'].shape)}  |out| max "
          f"{float(case['out'].abs().max()):.3f}  params {list(case['grad_params'])}")
seed = 9950
stack = run_stack(graph, seed)
while stack is None:
    seed += 1
    stack = run_stack(graph, seed)
G['stack'] = stack
print(f"stack: seed {stack['seed']}  margin {stack['margin']:.2e}  keys {len(stack['state'])}")

out_path = os.path.join(HERE, 'golden_cg_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
