"""Generates tests/golden/golden_film_v1.pt by running the REAL reference (PyG) on CPU: ``FiLMConv``
(nn/conv/film_conv.py:19-165) in ten settings and one two-layer stack.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_film.py

The graph has 40 nodes, 12 input features and 200 edges with skewed destinations, empty
destinations and some self-loops, plus a 15-node destination set for the bipartite case.  Every
case draws its own edge types from its seed.  Tensors only (and each case's constructor arguments
as plain values): inputs, edge types, state dicts, outputs and the gradients of every ``x`` and of
every parameter.

ReLU flips: a float32 kernel may round a pre-activation across zero, which flips a mask and
changes a gradient by a whole entry.  For every case with a ReLU the generator therefore computes
``min |pre|`` over all slots of all relations and over the skip term (for the stack: of both
layers), advances the case's seed until it is at least 1e-4, and records the seed taken and the
minimum (``margin``).  The margin is about 100 x the error the split-arithmetic dense transforms
put on a pre-activation of unit scale.
"""
import os
import sys

import torch
from torch.nn import Linear, ReLU, Sequential, Tanh

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import FiLMConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E, F = 40, 12, 200, 16
N_PAIR_DST, PAIR = 15, (5, 7)
HIDDEN = 8
MARGIN = 1e-4

# in_channels, out_channels, num_relations, aggr, act, nn, x: 'one' | 'pair', edge types drawn below
CASES = {
    'r1_default': (K, F, 1, 'mean', 'relu', None, 'one', None),
    'r3_mean': (K, F, 3, 'mean', 'relu', None, 'one', 3),
    'r3_add': (K, F, 3, 'add', 'relu', None, 'one', 3),
    'r3_empty_relation': (K, F, 3, 'mean', 'relu', None, 'one', 'skip1'),
    'r3_out_of_range': (K, F, 3, 'mean', 'relu', None, 'one', 5),
    'pair_r2': (PAIR, F, 2, 'mean', 'relu', None, 'pair', 2),
    'act_none': (K, F, 3, 'mean', 'none', None, 'one', 3),
    'custom_nn': (K, F, 2, 'add', 'relu', HIDDEN, 'one', 2),
    'r2_max': (K, F, 2, 'max', 'relu', None, 'one', 2),
    'act_tanh': (K, F, 3, 'mean', 'tanh', None, 'one', 3),
}
ACTS = {'relu': ReLU, 'none': lambda: None, 'tanh': Tanh}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_graph(seed):
    g = gen(seed)
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    src[:8] = dst[:8]                                     # some self-loops
    pair_dst = (torch.rand(E, generator=g).pow(3) * N_PAIR_DST).long().clamp(max=N_PAIR_DST - 1)
    return {'x': torch.randn(N, K, generator=g),
            'x_pair_src': torch.randn(N, PAIR[0], generator=g),
            'x_pair_dst': torch.randn(N_PAIR_DST, PAIR[1], generator=g),
            'edge_index': torch.stack([src, dst]), 'edge_index_pair': torch.stack([src, pair_dst])}


def draw_types(kind, seed):
    if kind is None:
        return None
    g = gen(seed + 50)
    if kind == 'skip1':                                   # relation 1 has no edges
        return torch.randint(0, 2, (E, ), generator=g) * 2
    return torch.randint(0, kind, (E, ), generator=g)


def make_conv(in_channels, out_channels, R, aggr, act, hidden):
    nn = None
    if hidden is not None:
        width = in_channels if isinstance(in_channels, int) else in_channels[1]
        nn = Sequential(Linear(width, hidden), Tanh(), Linear(hidden, 2 * out_channels))
    return FiLMConv(in_channels, out_channels, num_relations=R, nn=nn, act=ACTS[act](), aggr=aggr)


def margin(conv, x_src, x_dst, ei, et):
    """min |pre-activation| over the skip term and every slot of every relation"""
    with torch.no_grad():
        Fo = conv.out_channels
        beta, gamma = conv.film_skip(x_dst).split(Fo, dim=-1)
        least = float((gamma * conv.lin_skip(x_dst) + beta).abs().min())
        for r, (lin, film) in enumerate(zip(conv.lins, conv.films)):
            beta, gamma = film(x_dst).split(Fo, dim=-1)
            sel = ei if et is None else ei[:, et == r]
            if sel.size(1) > 0:
                pre = gamma[sel[1]] * lin(x_src)[sel[0]] + beta[sel[1]]
                least = min(least, float(pre.abs().min()))
    return least


def snapshot(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def record(case, module, state, out, leaves, seed):
    go = torch.randn(out.shape, generator=gen(seed + 1))
    params = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(out, leaves + [p for _, p in params], go)
    case.update({'state': state, 'out': out.detach(), 'grad_out': go,
                 'grad_x': [g.detach() for g in grads[:len(leaves)]],
                 'grad_params': {n: g.detach() for (n, _), g in zip(params, grads[len(leaves):])}})
    return case


def run_conv(spec, graph, seed):
    in_channels, out_channels, R, aggr, act, hidden, mode, kind = spec
    torch.manual_seed(seed)
    conv = make_conv(in_channels, out_channels, R, aggr, act, hidden).train()
    if mode == 'pair':
        xs = [graph['x_pair_src'].clone().requires_grad_(True),
              graph['x_pair_dst'].clone().requires_grad_(True)]
        ei = graph['edge_index_pair']
    else:
        xs = [graph['x'].clone().requires_grad_(True)]
        ei = graph['edge_index']
    et = draw_types(kind, seed)
    case = {'in_channels': in_channels, 'out_channels': out_channels, 'num_relations': R,
            'aggr': aggr, 'act': act, 'hidden': hidden, 'mode': mode, 'seed': seed,
            'edge_type': et, 'repr': repr(conv)}
    if act == 'relu':
        case['margin'] = margin(conv, xs[0], xs[-1], ei, et)
        if case['margin'] < MARGIN:
            return None
    state = snapshot(conv)
    out = conv(xs[0] if mode == 'one' else (xs[0], xs[1]), ei, et)
    return record(case, conv, state, out, xs, seed)


def make_stack():
    return torch.nn.ModuleList([FiLMConv(K, F, num_relations=3), FiLMConv(F, 8, num_relations=3)])


def run_stack(graph, seed):
    torch.manual_seed(seed)
    layers = make_stack().train()
    x = graph['x'].clone().requires_grad_(True)
    ei, et = graph['edge_index'], draw_types(3, seed)
    mid = layers[0](x, ei, et)
    case = {'seed': seed, 'edge_type': et,
            'margin': min(margin(layers[0], x, x, ei, et), margin(layers[1], mid, mid, ei, et))}
    if case['margin'] < MARGIN:
        return None
    return record(case, layers, snapshot(layers), layers[1](mid, ei, et), [x], seed)


def first(run, seed):
    out = run(seed)
    while out is None:
        seed += 1
        out = run(seed)
    return out


graph = make_graph(3)
deg = torch.bincount(graph['edge_index'][1], minlength=N)
assert int((deg == 0).sum()) > 0 and int(deg.max()) > 20

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'N': N, 'K': K},
     **graph, 'cases': {}}
for i, (name, spec) in enumerate(CASES.items()):
    case = first(lambda s: run_conv(spec, graph, s), 7300 + 200 * i)
    G['cases'][name] = case
    print(f"{name}: seed {case['seed']}  margin {case.get('margin', float('nan')):.2e}  out "
          f"{tuple(case['out'].shape)}  |out| max {float(case['out'].abs().max()):.3f}  params "
          f"{len(case['grad_params'])}")
G['stack'] = first(lambda s: run_stack(graph, s), 9700)
print(f"stack: seed {G['stack']['seed']}  margin {G['stack']['margin']:.2e}  keys "
      f"{len(G['stack']['state'])}")
for name, case in list(G['cases'].items()) + [('stack', G['stack'])]:
    assert case.get('margin', 1.0) >= MARGIN, name
et = G['cases']['r3_empty_relation']['edge_type']
assert int((et == 1).sum()) == 0
et = G['cases']['r3_out_of_range']['edge_type']
assert int((et >= 3).sum()) > 0

out_path = os.path.join(HERE, 'golden_film_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
