"""Generates tests/golden/golden_han_v1.pt by running the REAL reference (PyG) on CPU: ``HANConv``
(nn/conv/han_conv.py:34-183) on seven small typed graphs, all in ``eval()``.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_han.py

Node sizes and edge counts are those of make_golden_hgt.py: tens of nodes per type and skewed
destinations (a few long rows, some empty ones).  ``lin_src``, ``lin_dst`` and ``q`` are drawn at
random rather than left at glorot scale, so that their place in the formula is pinned.  Tensors
only: inputs, state dicts, outputs, ``beta`` and the gradients of the inputs and of every parameter
the call uses.

The layer has two kinks, the LeakyReLU of the logits and the ReLU of the aggregated rows; a value
within rounding of one lands on either side depending on the order of a float32 sum.  A seed is
refused (the next one is tried, +1000) when a LeakyReLU argument lies within ``1e-4 * max|arg|`` of
0 or a pre-ReLU element within ``1e-4 * max|value|`` of 0; the smallest margins found are stored.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ.get('PYG_REFERENCE', '/root/reference'))
import torch_geometric  # noqa: E402
from torch_geometric.nn import HANConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

AWP = ('author', 'writes', 'paper')
ARP = ('author', 'reviews', 'paper')
PRA = ('paper', 'rev_writes', 'author')
PCP = ('paper', 'cites', 'paper')
PIV = ('paper', 'in', 'venue')
VHP = ('venue', 'hosts', 'paper')
SIZES = {'author': 20, 'paper': 30, 'venue': 6}
MARGIN = 1e-4

# name -> (in_channels, out_channels, heads, node types, metadata edge types,
#          {edge type of the call: number of edges}, node sizes)
CASES = {
    # (a) three node types, four edge types: paper is the destination of two (beta of length 2)
    'three_types': ({'author': 8, 'paper': 12, 'venue': 5}, 16, 2, ['author', 'paper', 'venue'],
                    [AWP, PRA, PCP, PIV], {AWP: 90, PRA: 70, PCP: 120, PIV: 40}, SIZES),
    # (b) two edge types with one source AND one destination type, next to a third
    'shared': ({'author': 8, 'paper': 12}, 12, 2, ['author', 'paper'], [AWP, ARP, PRA],
               {AWP: 70, ARP: 50, PRA: 60}, SIZES),
    # (c) an edge type with an empty edge_index (a block of zeros in the semantic attention) and
    # one missing from the dict (its lin_src / lin_dst take no gradient)
    'empty_missing': ({'author': 8, 'paper': 12, 'venue': 5}, 16, 2, ['author', 'paper', 'venue'],
                      [AWP, PRA, PCP, PIV], {AWP: 90, PRA: 0, PIV: 40}, SIZES),
    # (d) venue is only ever a source: it maps to None
    'source_only': ({'author': 8, 'paper': 12, 'venue': 5}, 16, 2, ['author', 'paper', 'venue'],
                    [AWP, PRA, VHP], {AWP: 90, PRA: 70, VHP: 50}, SIZES),
    # (e) one head
    'heads1': ({'author': 8, 'paper': 12}, 8, 1, ['author', 'paper'], [AWP, PRA, PCP],
               {AWP: 80, PRA: 60, PCP: 100}, SIZES),
    # (f) D = 5: no multiple of any tile
    'd5': ({'author': 8, 'paper': 12}, 15, 3, ['author', 'paper'], [AWP, PRA, PCP],
           {AWP: 80, PRA: 60, PCP: 100}, SIZES),
    # (g) venue has no rows: a [0, 16] output and None weights
    'no_venue_rows': ({'author': 8, 'paper': 12, 'venue': 5}, 16, 2, ['author', 'paper', 'venue'],
                      [AWP, PRA, PIV], {AWP: 90, PRA: 70, PIV: 0},
                      {'author': 20, 'paper': 30, 'venue': 0}),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def kink_margins(conv, x_dict, edge_index_dict):
    """(smallest |LeakyReLU argument| / max, smallest |pre-ReLU element| / max) of the call, from
    the reference's own modules; 1.0 where there is nothing to measure."""
    H, D = conv.heads, conv.out_channels // conv.heads
    args, pres = [], []
    with torch.no_grad():
        xn = {t: conv.proj[t](x).view(-1, H, D) for t, x in x_dict.items()}
        for et, ei in edge_index_dict.items():
            key = '__'.join(et)
            a_src = (xn[et[0]] * conv.lin_src[key]).sum(-1)
            a_dst = (xn[et[-1]] * conv.lin_dst[key]).sum(-1)
            args.append((a_src[ei[0]] + a_dst[ei[1]]).flatten())
            pre = conv.propagate(ei, x=(xn[et[0]], xn[et[-1]]), alpha=(a_src, a_dst))
            # rows without an incoming edge are exactly 0 on every route: no kink to land on
            deg = torch.bincount(ei[1], minlength=pre.size(0))
            pres.append(pre[deg > 0].flatten())

    def margin(parts):
        v = torch.cat(parts).abs() if parts else torch.zeros(0)
        return float(v.min() / v.max()) if v.numel() else 1.0

    return margin(args), margin(pres)


def run_case(name, spec, seed):
    in_channels, out_channels, heads, node_types, edge_types, edges, sizes = spec
    g = gen(seed)
    x_dict = {t: torch.randn(sizes[t], in_channels[t], generator=g) for t in node_types}
    edge_index_dict = {}
    for et, e in edges.items():
        n_src, n_dst = sizes[et[0]], sizes[et[-1]]
        src = torch.randint(0, max(n_src, 1), (e, ), generator=g)
        dst = (torch.rand(e, generator=g).pow(3) * n_dst).long().clamp(max=max(n_dst - 1, 0))
        edge_index_dict[et] = torch.stack([src, dst])
    torch.manual_seed(seed)
    conv = HANConv(in_channels, out_channels, (node_types, edge_types), heads=heads)
    with torch.no_grad():
        for p in list(conv.lin_src.values()) + list(conv.lin_dst.values()) + [conv.q]:
            p.copy_(torch.randn(p.shape, generator=g))
    conv.eval()
    m_leaky, m_relu = kink_margins(conv, x_dict, edge_index_dict)
    if m_leaky < MARGIN or m_relu < MARGIN:
        return None, (m_leaky, m_relu)
    xs = {t: v.clone().requires_grad_(True) for t, v in x_dict.items()}
    out, beta = conv(xs, edge_index_dict, return_semantic_attention_weights=True)
    keys = [t for t in out if out[t] is not None]
    grad_out = {t: torch.randn(out[t].shape, generator=gen(seed + 1)) for t in keys}
    names = [n for n, _ in conv.named_parameters()]
    diff = [t for t in keys if out[t].requires_grad]
    grads = torch.autograd.grad([out[t] for t in diff],
                                list(xs.values()) + [p for _, p in conv.named_parameters()],
                                [grad_out[t] for t in diff], allow_unused=True)
    g_x, g_p = grads[:len(xs)], grads[len(xs):]
    return {'kwargs': {'in_channels': in_channels, 'out_channels': out_channels,
                       'metadata': (node_types, edge_types), 'heads': heads},
            'x_dict': x_dict, 'edge_index_dict': edge_index_dict,
            'state': {k: v.detach().clone() for k, v in conv.state_dict().items()},
            'out': {t: out[t].detach() for t in keys},
            'none': [t for t in out if out[t] is None],
            'beta': {t: b.detach() for t, b in beta.items() if b is not None},
            'grad_out': grad_out,
            'grad_x': {t: g.detach() for t, g in zip(xs, g_x) if g is not None},
            'grad_params': {n: g.detach() for n, g in zip(names, g_p) if g is not None},
            'margin_leaky': torch.tensor(m_leaky), 'margin_relu': torch.tensor(m_relu),
            'seed': seed}, (m_leaky, m_relu)


def main():
    cases = {}
    for i, (name, spec) in enumerate(CASES.items()):
        seed = 5100 + i
        while True:
            case, margins = run_case(name, spec, seed)
            if case is not None:
                break
            print(f'{name}: seed {seed} refused, margins {margins[0]:.2e} / {margins[1]:.2e}')
            seed += 1000
        cases[name] = case
    path = os.path.join(HERE, 'golden_han_v1.pt')
    torch.save({'cases': cases, 'torch': str(torch.__version__),
                'reference': str(torch_geometric.__version__)}, path)
    print(path, os.path.getsize(path), 'bytes')
    for name, c in cases.items():
        print(name, 'seed', c['seed'], {t: tuple(v.shape) for t, v in c['out'].items()},
              {t: tuple(b.shape) for t, b in c['beta'].items()}, len(c['grad_params']),
              'parameter gradients, margins', f"{float(c['margin_leaky']):.2e}",
              f"{float(c['margin_relu']):.2e}")


if __name__ == '__main__':
    main()
