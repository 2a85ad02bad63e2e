"""Generates tests/golden/golden_hetero_conv_v1.pt by running the REAL reference (PyG,
/root/reference) on CPU: ``HeteroConv({edge_type: SAGEConv((K, K), N)})``
(nn/conv/hetero_conv.py:13-172 over nn/conv/sage_conv.py:68-152) on a small typed graph.  Build
container only:

    PYTHONPATH=/root/reference python tests/golden/make_golden_hetero_conv.py

The graph: three node types, of which ``c`` is never a destination; five edge types, two of them
parallel between the same pair of types (``a -> b``), one self-typed (``b -> b``) and one with
zero edges (``c -> b``), whose bias and root term still count in the group.  Cases: the six group
modes x conv ``aggr`` mean / sum; in every case one conv has ``root_weight=False`` and one
``bias=False``."""
import os
import sys
import warnings

import torch

sys.path.insert(0, os.environ.get('PYG_REFERENCE', '/root/reference'))
import torch_geometric  # noqa: E402
from torch_geometric.nn import HeteroConv, SAGEConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
K, N_OUT = 8, 6
NUM_NODES = {'a': 40, 'b': 32, 'c': 24}
EDGE_TYPES = [('a', 'to', 'b'), ('a', 'also', 'b'), ('c', 'feeds', 'a'), ('b', 'self', 'b'),
              ('c', 'empty', 'b')]
NUM_EDGES = [160, 100, 120, 140, 0]
CONV_KWARGS = {('a', 'also', 'b'): {'root_weight': False}, ('b', 'self', 'b'): {'bias': False}}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def key(edge_type):
    return '__'.join(edge_type)


x_dict = {t: torch.randn(n, K, generator=gen(10 + i)) for i, (t, n) in enumerate(NUM_NODES.items())}
edge_index_dict = {}
for i, (et, e) in enumerate(zip(EDGE_TYPES, NUM_EDGES)):
    g = gen(20 + i)
    src = torch.randint(0, NUM_NODES[et[0]], (e, ), generator=g)
    # skewed destinations: a few long rows, many empty ones
    dst = (torch.rand(e, generator=g).pow(3) * NUM_NODES[et[2]]).long().clamp(max=NUM_NODES[et[2]] - 1)
    edge_index_dict[et] = torch.stack([src, dst])

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'K': K,
              'N_out': N_OUT, 'edge_types': EDGE_TYPES,
              'conv_kwargs': {key(et): kw for et, kw in CONV_KWARGS.items()}},
     'x_dict': x_dict,
     'edge_index_dict': {key(et): ei for et, ei in edge_index_dict.items()},
     'cases': {}}

for gi, group_aggr in enumerate(['sum', 'mean', 'min', 'max', 'cat', None]):
    for ci, conv_aggr in enumerate(['mean', 'sum']):
        torch.manual_seed(100 + 10 * gi + ci)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')  # 'c' is never a destination: the reference warns
            conv = HeteroConv({et: SAGEConv((K, K), N_OUT, aggr=conv_aggr,
                                            **CONV_KWARGS.get(et, {})) for et in EDGE_TYPES},
                              aggr=group_aggr)
        conv.eval()
        xs = {t: v.clone().requires_grad_(True) for t, v in x_dict.items()}
        out = conv(xs, edge_index_dict)
        order = list(out.keys())
        gos = {t: torch.randn(out[t].shape, generator=gen(200 + 10 * gi + ci + 50 * j))
               for j, t in enumerate(order)}
        names = [n for n, _ in conv.named_parameters()]
        leaves = [xs[t] for t in NUM_NODES] + [p for _, p in conv.named_parameters()]
        grads = torch.autograd.grad([out[t] for t in order], leaves, [gos[t] for t in order],
                                    allow_unused=True)
        nx = len(NUM_NODES)
        G['cases'][f'{group_aggr}-{conv_aggr}'] = {
            'group_aggr': group_aggr, 'conv_aggr': conv_aggr,
            'state': {k: v.detach().clone() for k, v in conv.state_dict().items()},
            'out_order': order,
            'out': {t: out[t].detach() for t in order},
            'grad_out': gos,
            'grad_x': {t: (None if g_ is None else g_.detach())
                       for t, g_ in zip(NUM_NODES, grads[:nx])},
            'grad_params': {n: (None if g_ is None else g_.detach())
                            for n, g_ in zip(names, grads[nx:])},
        }

out_path = os.path.join(HERE, 'golden_hetero_conv_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
