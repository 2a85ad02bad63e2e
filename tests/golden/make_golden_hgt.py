"""Generates tests/golden/golden_hgt_v1.pt by running the REAL reference (PyG) on CPU: ``HGTConv``
(nn/conv/hgt_conv.py:17-236) on seven small typed graphs, all in ``eval()``.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_hgt.py

Every case has tens of nodes per type and skewed destinations (a few long rows, some empty ones).
The parameters the reference initialises to one (``skip``, ``p_rel``) are drawn at random first, so
that their place in the formula is pinned.  Tensors only: inputs, state dicts, outputs and the
gradients of the inputs and of every parameter the call uses.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ.get('PYG_REFERENCE', '/root/reference'))
import torch_geometric  # noqa: E402
from torch_geometric.nn import HGTConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

AWP = ('author', 'writes', 'paper')
PRA = ('paper', 'rev_writes', 'author')
PCP = ('paper', 'cites', 'paper')
PIV = ('paper', 'in', 'venue')
VHP = ('venue', 'hosts', 'paper')
SIZES = {'author': 20, 'paper': 30, 'venue': 6}

# name -> (in_channels, out_channels, heads, node types, metadata edge types,
#          {edge type of the call: number of edges})
CASES = {
    # (a) three node types, four edge types, unequal widths: no skip mix.  paper is the source of
    # three edge types and the destination of two
    'three_types': ({'author': 8, 'paper': 12, 'venue': 5}, 16, 2, ['author', 'paper', 'venue'],
                    [AWP, PRA, PCP, PIV], {AWP: 90, PRA: 70, PCP: 120, PIV: 40}),
    # (b) one width everywhere, equal to out_channels: the sigmoid(skip) mix is active
    'skip': (16, 16, 4, ['author', 'paper'], [AWP, PRA, PCP], {AWP: 80, PRA: 60, PCP: 100}),
    # (c) two edge types with one source AND one destination type, next to a third
    'shared': ({'author': 8, 'paper': 12}, 12, 2, ['author', 'paper'],
               [AWP, ('author', 'reviews', 'paper'), PRA],
               {AWP: 70, ('author', 'reviews', 'paper'): 50, PRA: 60}),
    # (d) an edge type with an empty edge_index and one missing from the dict
    'empty_missing': ({'author': 8, 'paper': 12, 'venue': 5}, 16, 2, ['author', 'paper', 'venue'],
                      [AWP, PRA, PCP, PIV], {AWP: 90, PRA: 0, PIV: 40}),
    # (e) venue is only ever a source: it is absent from the output
    'source_only': ({'author': 8, 'paper': 12, 'venue': 5}, 16, 2, ['author', 'paper', 'venue'],
                    [AWP, PRA, VHP], {AWP: 90, PRA: 70, VHP: 50}),
    # (f) one head
    'heads1': ({'author': 8, 'paper': 12}, 8, 1, ['author', 'paper'], [AWP, PRA, PCP],
               {AWP: 80, PRA: 60, PCP: 100}),
    # (g) D = 5: no multiple of any tile
    'd5': ({'author': 8, 'paper': 12}, 15, 3, ['author', 'paper'], [AWP, PRA, PCP],
           {AWP: 80, PRA: 60, PCP: 100}),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def run_case(name, spec, seed):
    in_channels, out_channels, heads, node_types, edge_types, edges = spec
    g = gen(seed)
    widths = in_channels if isinstance(in_channels, dict) else {t: in_channels for t in node_types}
    x_dict = {t: torch.randn(SIZES[t], widths[t], generator=g) for t in node_types}
    edge_index_dict = {}
    for et, e in edges.items():
        src = torch.randint(0, SIZES[et[0]], (e, ), generator=g)
        n_dst = SIZES[et[-1]]
        dst = (torch.rand(e, generator=g).pow(3) * n_dst).long().clamp(max=n_dst - 1)
        edge_index_dict[et] = torch.stack([src, dst])
    torch.manual_seed(seed)
    conv = HGTConv(in_channels, out_channels, (node_types, edge_types), heads=heads)
    with torch.no_grad():
        for p in list(conv.skip.values()) + list(conv.p_rel.values()):
            p.copy_(torch.randn(p.shape, generator=g))
    conv.eval()
    xs = {t: v.clone().requires_grad_(True) for t, v in x_dict.items()}
    out = conv(xs, edge_index_dict)
    keys = list(out)
    grad_out = {t: torch.randn(out[t].shape, generator=gen(seed + 1)) for t in keys}
    names = [n for n, _ in conv.named_parameters()]
    grads = torch.autograd.grad([out[t] for t in keys],
                                list(xs.values()) + [p for _, p in conv.named_parameters()],
                                [grad_out[t] for t in keys], allow_unused=True)
    g_x, g_p = grads[:len(xs)], grads[len(xs):]
    return {'kwargs': {'in_channels': in_channels, 'out_channels': out_channels,
                       'metadata': (node_types, edge_types), 'heads': heads},
            'x_dict': x_dict, 'edge_index_dict': edge_index_dict,
            'state': {k: v.detach().clone() for k, v in conv.state_dict().items()},
            'out': {t: out[t].detach() for t in keys}, 'grad_out': grad_out,
            'grad_x': {t: g.detach() for t, g in zip(xs, g_x) if g is not None},
            'grad_params': {n: g.detach() for n, g in zip(names, g_p) if g is not None},
            'seed': seed}


def main():
    cases = {name: run_case(name, spec, 4100 + i) for i, (name, spec) in enumerate(CASES.items())}
    path = os.path.join(HERE, 'golden_hgt_v1.pt')
    torch.save({'cases': cases, 'torch': torch.__version__,
                'reference': torch_geometric.__version__}, path)
    print(path, os.path.getsize(path), 'bytes')
    for name, c in cases.items():
        print(name, {t: tuple(v.shape) for t, v in c['out'].items()}, len(c['grad_params']),
              'parameter gradients')


if __name__ == '__main__':
    main()
