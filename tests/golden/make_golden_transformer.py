"""Generates tests/golden/golden_transformer_v1.pt by running the REAL reference (PyG) on CPU:
``TransformerConv`` (nn/conv/transformer_conv.py:16-287) in ten settings, all in ``eval()``.  Build
container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_transformer.py

The graph is the one of make_golden_gatv2.py: 48 nodes, 16 features, 400 edges with skewed
destinations (a few long rows, some empty ones), a 20-node destination set for the bipartite case
and ``edge_attr [400, 3]``.  The layer has no kinked non-linearity (scaled dot product, softmax,
sigmoid gate), so unlike the GATv2 file no gap guard is needed.  Tensors only: inputs, state dicts,
outputs and the gradients of the inputs and of every parameter.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ.get('PYG_REFERENCE', '/root/reference'))
import torch_geometric  # noqa: E402
from torch_geometric.nn import TransformerConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E, N_PAIR_DST, K_DST = 48, 16, 400, 20, 12

CASES = {
    't': dict(heads=4, out_channels=6),
    't_mean': dict(heads=4, out_channels=6, concat=False),
    't_beta': dict(heads=2, out_channels=6, beta=True),
    't_beta_mean': dict(heads=2, out_channels=6, beta=True, concat=False),
    't_noroot': dict(heads=2, out_channels=6, root_weight=False, beta=True),
    't_nobias': dict(heads=3, out_channels=6, bias=False),
    't_c5': dict(heads=3, out_channels=5),
    't_pair': dict(heads=2, out_channels=6, in_channels=(K, K_DST)),
    't_edge': dict(heads=2, out_channels=6, edge_dim=3),
    't_attention': dict(heads=2, out_channels=6),
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
            'edge_attr': torch.randn(E, 3, generator=g)}


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
    ea = graph['edge_attr'] if kw.get('edge_dim') else None
    x_in = tuple(xs) if pair else xs[0]
    attention = name == 't_attention'
    res = conv(x_in, ei, edge_attr=ea, return_attention_weights=True if attention else None)
    out, att = res if attention else (res, None)
    go = torch.randn(out.shape, generator=gen(seed + 1))
    names = [n for n, _ in conv.named_parameters()]
    # (lin_skip exists without root_weight but takes no part: no gradient is recorded for it)
    grads = torch.autograd.grad(out, xs + [p for _, p in conv.named_parameters()], go,
                                allow_unused=True)
    case = {'kwargs': dict(kw, in_channels=in_channels), 'pair': pair, 'edge_attr': ea is not None,
            'state': {k: v.detach().clone() for k, v in conv.state_dict().items()},
            'out': out.detach(), 'grad_out': go,
            'grad_x': [g.detach() for g in grads[:len(xs)]],
            'grad_params': {n: g.detach() for n, g in zip(names, grads[len(xs):]) if g is not None},
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
    G['cases'][name] = run_conv(name, kw, graph, 1000 + 200 * i)
    print(f"{name}: |out| max {float(G['cases'][name]['out'].abs().max()):.3f}")
assert 'lin_beta.weight' not in G['cases']['t_noroot']['state']    # beta and root_weight
assert 'lin_skip.weight' not in G['cases']['t_noroot']['grad_params']

out_path = os.path.join(HERE, 'golden_transformer_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
