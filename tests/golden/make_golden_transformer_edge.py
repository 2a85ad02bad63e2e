"""Generates tests/golden/golden_transformer_edge_v1.pt by running the REAL reference (PyG) on CPU:
``TransformerConv(edge_dim=...)`` (nn/conv/transformer_conv.py:16-287) in eight settings, all in
``eval()``.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_transformer_edge.py

The graph is the one of make_golden_transformer.py (48 nodes, 16 features, 400 edges with skewed
destinations, a 20-node destination set for the bipartite case) with ``edge_attr [400, 9]``; a case
with ``edge_dim = D`` reads its first ``D`` columns.  Unlike golden_transformer_v1.pt every case
also records the gradient of ``edge_attr``.  Tensors only: inputs, state dicts, outputs and the
gradients of the inputs, of the edge features and of every parameter.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import TransformerConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E, N_PAIR_DST, K_DST, DE_MAX = 48, 16, 400, 20, 12, 9

CASES = {
    'e': dict(heads=2, out_channels=6, edge_dim=3),
    'e_wide': dict(heads=2, out_channels=6, edge_dim=9),           # wider than C
    'e_mean': dict(heads=2, out_channels=6, edge_dim=3, concat=False),
    'e_beta': dict(heads=2, out_channels=6, edge_dim=3, beta=True),
    'e_noroot': dict(heads=2, out_channels=6, edge_dim=3, root_weight=False),
    'e_nobias': dict(heads=3, out_channels=5, edge_dim=3, bias=False),
    'e_pair': dict(heads=2, out_channels=6, edge_dim=3, in_channels=(K, K_DST)),
    'e_attention': dict(heads=2, out_channels=6, edge_dim=3),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_graph(seed):
    g = gen(seed)
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    src[:12] = dst[:12]                                   # some self-loops
    pair_dst = (torch.rand(E, generator=g).pow(3) * N_PAIR_DST).long().clamp(max=N_PAIR_DST - 1)
    return {'x': torch.randn(N, K, generator=g), 'x_dst': torch.randn(N_PAIR_DST, K_DST, generator=g),
            'edge_index': torch.stack([src, dst]), 'edge_index_pair': torch.stack([src, pair_dst]),
            'edge_attr': torch.randn(E, DE_MAX, generator=gen(seed + 100))}


def run_conv(name, kw, graph, seed):
    kw = dict(kw)
    pair = isinstance(kw.get('in_channels'), tuple)
    in_channels = kw.pop('in_channels', K)
    torch.manual_seed(seed)
    conv = TransformerConv(in_channels, **kw)
    conv.eval()
    xs = [graph['x'].clone().requires_grad_(True)]
    if pair:
        xs.append(graph['x_dst'].clone().requires_grad_(True))
    ei = graph['edge_index_pair'] if pair else graph['edge_index']
    ea = graph['edge_attr'][:, :kw['edge_dim']].clone().requires_grad_(True)
    x_in = tuple(xs) if pair else xs[0]
    attention = name == 'e_attention'
    res = conv(x_in, ei, edge_attr=ea, return_attention_weights=True if attention else None)
    out, att = res if attention else (res, None)
    go = torch.randn(out.shape, generator=gen(seed + 1))
    names = [n for n, _ in conv.named_parameters()]
    # (lin_skip exists without root_weight but takes no part: no gradient is recorded for it)
    grads = torch.autograd.grad(out, xs + [ea] + [p for _, p in conv.named_parameters()], go,
                                allow_unused=True)
    nx = len(xs)
    case = {'kwargs': dict(kw, in_channels=in_channels), 'pair': pair,
            'state': {k: v.detach().clone() for k, v in conv.state_dict().items()},
            'out': out.detach(), 'grad_out': go,
            'grad_x': [g.detach() for g in grads[:nx]],
            'grad_edge_attr': grads[nx].detach(),
            'grad_params': {n: g.detach() for n, g in zip(names, grads[nx + 1:])
                            if g is not None},
            'seed': seed}
    if attention:
        case['attention'] = (att[0].detach(), att[1].detach())
    return case


graph = make_graph(2)
deg = torch.bincount(graph['edge_index'][1], minlength=N)
assert int((deg == 0).sum()) > 0 and int(deg.max()) > 40

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'N': N, 'K': K},
     **graph, 'cases': {}}
for i, (name, kw) in enumerate(CASES.items()):
    G['cases'][name] = run_conv(name, kw, graph, 3000 + 200 * i)
    c = G['cases'][name]
    assert 'lin_edge.weight' in c['grad_params'], name
    print(f"{name}: |out| max {float(c['out'].abs().max()):.3f}  |grad_edge_attr| max "
          f"{float(c['grad_edge_attr'].abs().max()):.3f}")
assert 'lin_skip.weight' not in G['cases']['e_noroot']['grad_params']


out_path = os.path.join(HERE, 'golden_transformer_edge_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
