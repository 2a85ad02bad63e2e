"""Generates tests/golden/golden_pna_v1.pt by running the REAL reference (PyG) on CPU: ``PNAConv``
(nn/conv/pna_conv.py:18-213) over ``DegreeScalerAggregation`` (nn/aggr/scaler.py:13-109) in twelve
settings.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_pna.py

The graph is the one of make_golden_gin.py (48 nodes, 16 features, 400 edges with skewed
destinations: empty destinations, a hub over 40, self-loops and duplicate edges, whose equal
messages tie in min and max); ``in = out = 16``.  A case with ``edge_dim = D`` draws ``edge_attr
[400, D]`` from its seed.  The std aggregator is discontinuous where ``var`` crosses 1e-5: the
messages are formed in float64 and a case's seed is advanced until no (destination, column) of
degree >= 2 has ``var`` in [5e-6, 2e-5]; the seed that was taken is recorded.  Tensors only: inputs,
the degree histogram, state dicts, outputs and the gradients of ``x``, of ``edge_attr`` and of every
parameter.
"""
import copy
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import PNAConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E = 48, 16, 400
BAND = (5e-6, 2e-5)
FOUR = ['mean', 'min', 'max', 'std']
THREE = ['identity', 'amplification', 'attenuation']

CASES = {
    'identity': dict(aggregators=FOUR, scalers=['identity']),
    'amplification': dict(aggregators=FOUR, scalers=['amplification']),
    'attenuation': dict(aggregators=FOUR, scalers=['attenuation']),
    'towers4': dict(aggregators=FOUR, scalers=THREE, towers=4),
    'towers4_divide': dict(aggregators=FOUR, scalers=THREE, towers=4, divide_input=True),
    'edge3': dict(aggregators=FOUR, scalers=THREE, towers=2, edge_dim=3),
    'edge9': dict(aggregators=FOUR, scalers=['identity', 'attenuation'], edge_dim=9),
    'train_norm': dict(aggregators=FOUR, scalers=['amplification', 'attenuation', 'linear'],
                       train_norm=True),
    'linear_scalers': dict(aggregators=['mean', 'max'], scalers=['linear', 'inverse_linear']),
    'single': dict(aggregators=['max'], scalers=['identity'], edge_dim=3),
    'deep': dict(aggregators=FOUR, scalers=THREE, towers=2, pre_layers=2, post_layers=2,
                 edge_dim=3),
    'sum_var': dict(aggregators=['sum', 'var', 'mean'], scalers=['identity', 'amplification']),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_graph(seed):
    g = gen(seed)
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    src[:12] = dst[:12]                                   # some self-loops
    torch.rand(E, generator=g)                            # (make_golden_gin.py's pair draw)
    return {'x': torch.randn(N, K, generator=g), 'edge_index': torch.stack([src, dst])}


def in_band(conv, x, ei, ea):
    """the number of (destination, column) of degree >= 2 whose float64 variance lies in BAND"""
    c64 = copy.deepcopy(conv).double()
    T, F = conv.towers, conv.F_in
    xt = x.double().view(-1, T, F) if conv.divide_input else \
        x.double().view(-1, 1, F).repeat(1, T, 1)
    with torch.no_grad():
        m = c64.message(xt[ei[1]], xt[ei[0]], None if ea is None else ea.double())
    m = m.reshape(m.size(0), -1)
    cnt = torch.bincount(ei[1], minlength=N).double().view(-1, 1)
    mean = torch.zeros(N, m.size(1), dtype=torch.float64).index_add_(0, ei[1], m) / cnt.clamp(min=1)
    var = torch.zeros(N, m.size(1), dtype=torch.float64).index_add_(
        0, ei[1], (m - mean[ei[1]]) ** 2) / cnt.clamp(min=1)
    hit = (var >= BAND[0]) & (var <= BAND[1]) & (cnt >= 2)
    return int(hit.sum())


def run_conv(kw, graph, deg, seed):
    torch.manual_seed(seed)
    conv = PNAConv(K, K, deg=deg, **kw)
    x = graph['x'].clone().requires_grad_(True)
    ei = graph['edge_index']
    ea = None
    if kw.get('edge_dim'):
        ea = torch.randn(E, kw['edge_dim'], generator=gen(seed + 100)).requires_grad_(True)
    if in_band(conv, graph['x'], ei, None if ea is None else ea.detach()) > 0:
        return None
    out = conv(x, ei, ea)
    go = torch.randn(out.shape, generator=gen(seed + 1))
    names = [n for n, _ in conv.named_parameters()]
    leaves = [x] + ([ea] if ea is not None else [])
    grads = torch.autograd.grad(out, leaves + [p for _, p in conv.named_parameters()], go)
    case = {'kwargs': dict(kw), 'seed': seed,
            'state': {k: v.detach().clone() for k, v in conv.state_dict().items()},
            'out': out.detach(), 'grad_out': go, 'grad_x': grads[0].detach(),
            'grad_params': {n: g.detach() for n, g in zip(names, grads[len(leaves):])}}
    if ea is not None:
        case['edge_attr'] = ea.detach().clone()
        case['grad_edge_attr'] = grads[1].detach()
    return case


graph = make_graph(2)
in_deg = torch.bincount(graph['edge_index'][1], minlength=N)
assert int((in_deg == 0).sum()) > 0 and int(in_deg.max()) > 40
pairs = graph['edge_index'][0] * N + graph['edge_index'][1]
assert pairs.unique().numel() < E                         # duplicate edges: ties in min / max
deg = torch.bincount(in_deg)

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'N': N, 'K': K,
              'band': BAND}, **graph, 'deg': deg, 'cases': {}}
for i, (name, kw) in enumerate(CASES.items()):
    seed = 7000 + 200 * i
    case = run_conv(kw, graph, deg, seed)
    while case is None:
        seed += 1
        case = run_conv(kw, graph, deg, seed)
    G['cases'][name] = case
    assert ('aggr_module.avg_deg_lin' in case['grad_params']) == bool(kw.get('train_norm')), name
    print(f"{name}: seed {case['seed']}  out {tuple(case['out'].shape)}  |out| max "
          f"{float(case['out'].abs().max()):.3f}  keys {len(case['state'])}")

out_path = os.path.join(HERE, 'golden_pna_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
