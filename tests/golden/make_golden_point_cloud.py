"""Generates tests/golden/golden_point_cloud_v1.pt by running the REAL reference (PyG) on CPU:
``EdgeConv`` (nn/conv/edge_conv.py) and ``PointNetConv`` (nn/conv/point_conv.py).  Build container
only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_point_cloud.py

Two clouds of 40 and 25 random normal points in 3-D.  The graph is built HERE by brute force in
float64: the 6 nearest neighbours of every point inside its cloud, the point itself included,
ordered by (distance, index); the script asserts that every query is decided, i.e. that all gaps
between consecutive distances up to rank 7 exceed ``(3 + 4) * 2^-23`` of the distance, so a float32
search finds exactly these edges.  ``edge_index`` is ``[neighbour; point]`` (source to target);
``edge_index_no_loop`` is the same without the self loops.

``EdgeConv`` runs with ``aggr`` max / add / mean on the coordinates and an MLP of two ``Linear``s —
this is also the expected result of ``DynamicEdgeConv(k=6)`` on the clouds, whose reference class
cannot be constructed without pyg-lib.  ``PointNetConv`` runs on five extra features per point over
``edge_index_no_loop``, with and without ``add_self_loops``, for the three aggregations.

Every case is evaluated twice by the reference: in float64 — the stored ``out`` and input
gradients (rounded once to float32), the parameter gradients kept in float64 — and in float32,
whose scaled error against float64, ``max |f32 - f64| / max(max |f64|, 1)``, is stored per tensor
under ``ref_err``.  The seed of a case is advanced until no input of a ReLU sits within 1e-4 of
zero.  Tensors, floats, strings and lists only."""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import EdgeConv, PointNetConv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [40, 25]
K = 6
F_POS, F_X, HIDDEN, OUT, OUT_GLOBAL = 3, 5, 16, 8, 6
MARGIN = 1e-4
TAU = (F_POS + 4) * 2.0 ** -23


def gen(seed):
    return torch.Generator().manual_seed(seed)


N = sum(SIZES)
batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
pos = torch.randn(N, F_POS, generator=gen(1))
feat = torch.randn(N, F_X, generator=gen(2))

rows, cols = [], []
base = 0
for n in SIZES:
    p = pos[base:base + n].double()
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    od, oi = torch.sort(d, dim=1, stable=True)
    gaps = od[:, 1:K + 1] - od[:, :K]
    assert bool((gaps > TAU * od[:, 1:K + 1]).all()), 'an undecided query: change the seed'
    rows.append(torch.arange(n).repeat_interleave(K) + base)
    cols.append(oi[:, :K].reshape(-1) + base)
    base += n
row, col = torch.cat(rows), torch.cat(cols)
edge_index = torch.stack([col, row])
edge_index_no_loop = edge_index[:, col != row]
assert edge_index_no_loop.size(1) == N * (K - 1)


def scaled_err(a32, a64):
    return float((a32.double() - a64).abs().max() / max(float(a64.abs().max()), 1.0))


def mlp(seed, n_in, n_out):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(n_in, HIDDEN), torch.nn.ReLU(),
                               torch.nn.Linear(HIDDEN, n_out))


def record(make, inputs, call, grad_out, **meta):
    """inputs: name -> float32 tensor (each gets a gradient)"""
    seen = []
    probe = make().double()
    for m in probe.modules():
        if isinstance(m, torch.nn.ReLU):
            m.register_forward_hook(lambda mod, a, o: seen.append(float(a[0].detach().abs().min())))
    call(probe, {k: v.double() for k, v in inputs.items()})
    if min(seen) < MARGIN:
        return None

    def evaluate(dtype):
        m = make().to(dtype)
        xs = {k: v.to(dtype).clone().requires_grad_(True) for k, v in inputs.items()}
        out = call(m, xs)
        params = list(m.named_parameters())
        grads = torch.autograd.grad(out, list(xs.values()) + [p for _, p in params],
                                    grad_out.to(dtype))
        g_in = dict(zip(xs, grads[:len(xs)]))
        return out.detach(), g_in, {n: g.detach() for (n, _), g in zip(params, grads[len(xs):])}

    o64, gi64, gp64 = evaluate(torch.float64)
    o32, gi32, gp32 = evaluate(torch.float32)
    err = {'out': scaled_err(o32, o64)}
    err.update({f'grad.{k}': scaled_err(gi32[k], v) for k, v in gi64.items()})
    err.update({f'grad_params.{n}': scaled_err(gp32[n], v) for n, v in gp64.items()})
    m = make()
    return {'state': {k: v.detach().clone() for k, v in m.state_dict().items()},
            'keys': list(m.state_dict().keys()), 'repr': repr(m), 'out': o64.float(),
            'grad': {k: v.float() for k, v in gi64.items()}, 'grad_params': gp64,
            'ref_err': err, 'margin': min(seen), **meta}


def until_safe(build):
    seed = 100
    case = build(seed)
    while case is None:
        seed += 1
        case = build(seed)
    case['seed'] = seed
    return case


G = {'meta': {'torch': str(torch.__version__), 'pyg': str(torch_geometric.__version__), 'sizes': SIZES,
              'k': K, 'hidden': HIDDEN, 'margin': MARGIN},
     'batch': batch, 'pos': pos, 'feat': feat, 'edge_index': edge_index,
     'edge_index_no_loop': edge_index_no_loop,
     'grad_out': torch.randn(N, OUT, generator=gen(3)),
     'grad_out_global': torch.randn(N, OUT_GLOBAL, generator=gen(4)), 'cases': {}}
C = G['cases']

for aggr in ('max', 'add', 'mean'):
    C[f'edge_conv_{aggr}'] = until_safe(lambda seed: record(
        lambda: EdgeConv(mlp(seed, 2 * F_POS, OUT), aggr=aggr), {'x': pos},
        lambda m, t: m(t['x'], edge_index), G['grad_out'], kind='edge_conv', aggr=aggr))
    for loops in (True, False):
        C[f'point_net_conv_{aggr}_{"loops" if loops else "plain"}'] = until_safe(
            lambda seed: record(
                lambda: PointNetConv(mlp(seed, F_X + F_POS, OUT),
                                     torch.nn.Sequential(torch.nn.Linear(OUT, OUT_GLOBAL)),
                                     add_self_loops=loops, aggr=aggr), {'x': feat, 'pos': pos},
                lambda m, t: m(t['x'], t['pos'], edge_index_no_loop), G['grad_out_global'],
                kind='point_net_conv', aggr=aggr, add_self_loops=loops))

for name, case in C.items():
    print(f"{name}: seed {case['seed']} margin {case['margin']:.1e} keys {case['keys']} ref_err "
          + ' '.join(f'{k} {v:.1e}' for k, v in case['ref_err'].items()))
out_path = os.path.join(HERE, 'golden_point_cloud_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
