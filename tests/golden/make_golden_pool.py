"""Generates tests/golden/golden_pool_v1.pt by running the REAL reference (PyG) on CPU:
``TopKPooling`` (nn/pool/topk_pool.py), ``SAGPooling`` (nn/pool/sag_pool.py) and ``topk``
(nn/pool/select/topk.py) on an unsorted batch vector.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_pool.py

One batch of nine graphs of ``[1, 2, 3, 63, 64, 65, 0, 70, 5]`` nodes (one of them empty) with
``F = 20`` features and 1,200 random edges inside the graphs, self loops and duplicates included.

Every layer case is evaluated twice by the reference: in float64 — the stored outputs, ``perm``,
``grad_x``, ``grad_edge_attr`` and parameter gradients (the float tensors rounded once to float32,
the parameter gradients kept in float64) — and in float32, whose scaled error against float64,
``max |f32 - f64| / max(max |f64|, 1)``, is stored per tensor as a plain float under ``ref_err``.
For every ``ratio`` case the seed is advanced until any two scores of one graph differ by at least
1e-4 (a float32 score may otherwise order two nodes the other way); in ``min_score`` mode, where a
threshold selects and the order is not used, until no score sits within 1e-6 of its threshold.
The generator asserts the margin, and that the float32 evaluation selects the same nodes.

Tensors, floats and constructor arguments only."""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import GCNConv, GraphConv, SAGPooling, TopKPooling  # noqa: E402
from torch_geometric.nn.pool.select.topk import topk  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
F = 20
SIZES = [1, 2, 3, 63, 64, 65, 0, 70, 5]
MARGIN = 1e-4
E = 1200
GNNS = {'GraphConv': GraphConv, 'GCNConv': GCNConv}


def gen(seed):
    return torch.Generator().manual_seed(seed)


batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
N = batch.numel()
ptr = torch.tensor([0] + torch.tensor(SIZES).cumsum(0).tolist())
x = torch.randn(N, F, generator=gen(11))
g = gen(21)
graph_of_edge = torch.multinomial(torch.tensor(SIZES, dtype=torch.float), E, replacement=True,
                                  generator=g)
lo, size = ptr[graph_of_edge], torch.tensor(SIZES)[graph_of_edge]
edge_index = torch.stack([lo + (torch.rand(E, generator=g) * size).long().clamp(max=size - 1),
                          lo + (torch.rand(E, generator=g) * size).long().clamp(max=size - 1)])
edge_index[:, 100:120] = edge_index[:, 0:20]          # duplicates
edge_index[1, 200:230] = edge_index[0, 200:230]       # self loops
# (a two-node graph joined both ways gives both nodes the SAME GCN score: keep only loops on node 1)
edge_index[:, batch[edge_index[0]] == 1] = 1
EDGE_ATTR = {None: None, 'E': torch.randn(E, generator=gen(31)),
             'E3': torch.randn(E, 3, generator=gen(32))}


def scaled_err(a32, a64):
    if a64.numel() == 0:
        return 0.0
    return float((a32.double() - a64).abs().max() / max(float(a64.abs().max()), 1.0))


def make_layer(kind, kwargs, gnn, seed):
    torch.manual_seed(seed)
    if kind == 'topk':
        return TopKPooling(F, **kwargs)
    return SAGPooling(F, GNN=GNNS[gnn], **kwargs)


def score_margin(layer, use_batch):
    """the smallest gap between two scores of one graph (and to the min_score threshold)"""
    layer = layer.double()
    b = batch if use_batch else torch.zeros(N, dtype=torch.long)
    attn = x.double()
    if isinstance(layer, SAGPooling):
        attn = layer.gnn(attn, edge_index)
    sel = layer.select
    score = (attn * sel.weight).sum(-1)
    if sel.min_score is None:
        score = sel.act(score / sel.weight.norm(p=2, dim=-1))
    else:
        from torch_geometric.utils import softmax
        score = softmax(score, b)
    gap = float('inf')
    for i in b.unique().tolist():
        s = score[b == i].detach().sort().values
        if s.numel() > 1 and sel.min_score is None:
            gap = min(gap, float((s[1:] - s[:-1]).min()))
        if sel.min_score is not None:   # (a threshold selects: the order of the scores is not used)
            thr = min(sel.min_score, float(s.max()) - 1e-7)
            gap = min(gap, float((s - thr).abs().min()) * (MARGIN / 1e-6))
    return gap


def evaluate(kind, kwargs, gnn, seed, attr, use_batch, dtype):
    layer = make_layer(kind, kwargs, gnn, seed).to(dtype)
    xx = x.to(dtype).clone().requires_grad_(True)
    ea = EDGE_ATTR[attr]
    ea = None if ea is None else ea.to(dtype).clone().requires_grad_(True)
    out, ei, eo, bo, perm, score = layer(xx, edge_index, ea, batch if use_batch else None)
    go = torch.randn(out.shape, generator=gen(41), dtype=torch.float64).to(dtype)
    gs = torch.randn(score.shape, generator=gen(42), dtype=torch.float64).to(dtype)
    loss = (out * go).sum() + (score * gs).sum()
    if eo is not None:
        ge = torch.randn(eo.shape, generator=gen(43), dtype=torch.float64).to(dtype)
        loss = loss + (eo * ge).sum()
    params = list(layer.named_parameters())
    grads = torch.autograd.grad(loss, [xx] + [p for _, p in params]
                                + ([] if ea is None else [ea]))
    res = {'out': out.detach(), 'score': score.detach(), 'grad_x': grads[0]}
    res.update({f'grad_params.{n}': v for (n, _), v in zip(params, grads[1:])})
    if ea is not None:
        res['edge_attr'] = eo.detach()
        res['grad_edge_attr'] = grads[-1]
    return res, {'edge_index': ei, 'batch': bo, 'perm': perm}


def record(kind, kwargs, gnn=None, attr=None, use_batch=True, seed=100):
    while score_margin(make_layer(kind, kwargs, gnn, seed), use_batch) < MARGIN:
        seed += 1
    assert score_margin(make_layer(kind, kwargs, gnn, seed), use_batch) >= MARGIN
    r64, i64 = evaluate(kind, kwargs, gnn, seed, attr, use_batch, torch.float64)
    r32, i32 = evaluate(kind, kwargs, gnn, seed, attr, use_batch, torch.float32)
    for key in i64:
        assert torch.equal(i64[key], i32[key]), key
    layer = make_layer(kind, kwargs, gnn, seed)
    case = {'kind': kind, 'kwargs': kwargs, 'gnn': gnn, 'attr': attr, 'use_batch': use_batch,
            'seed': seed, 'repr': repr(layer),
            'state': {k: v.detach().clone() for k, v in layer.state_dict().items()},
            'ref_err': {k: scaled_err(r32[k], v) for k, v in r64.items()}}
    case.update(i64)
    case.update({k: (v if k.startswith('grad_params.') else v.float()) for k, v in r64.items()})
    return case


G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'F': F,
              'sizes': SIZES, 'margin': MARGIN, 'grad_seeds': {'out': 41, 'score': 42,
                                                              'edge_attr': 43}},
     'batch': batch, 'x': x, 'edge_index': edge_index,
     'edge_attr': {k: v for k, v in EDGE_ATTR.items() if k is not None}, 'cases': {}}
C = G['cases']
C['topk_ratio_0.5'] = record('topk', {'ratio': 0.5})
C['topk_ratio_0.7_attr_E'] = record('topk', {'ratio': 0.7}, attr='E')
C['topk_ratio_3_attr_E3'] = record('topk', {'ratio': 3}, attr='E3')
C['topk_ratio_100'] = record('topk', {'ratio': 100})
C['topk_min_score'] = record('topk', {'min_score': 0.01}, attr='E3')
C['topk_multiplier_2'] = record('topk', {'ratio': 0.5, 'multiplier': 2.0}, attr='E')
C['topk_sigmoid'] = record('topk', {'ratio': 0.5, 'nonlinearity': 'sigmoid'})
C['topk_no_batch'] = record('topk', {'ratio': 0.5}, attr='E3', use_batch=False)
C['sag_graph_conv'] = record('sag', {'ratio': 0.5}, gnn='GraphConv', attr='E3')
C['sag_gcn_conv'] = record('sag', {'ratio': 0.7, 'multiplier': 2.0}, gnn='GCNConv')
C['sag_min_score'] = record('sag', {'min_score': 0.01}, gnn='GraphConv', attr='E')

# ---- topk on an unsorted batch vector --------------------------------------------------------------
shuffle = torch.randperm(N, generator=gen(51))
score = (torch.randperm(N, generator=gen(52)).float() / N)     # tie-free by construction
G['unsorted'] = {'batch': batch[shuffle], 'score': score,
                 'perm': {r: topk(score, r, batch[shuffle]) for r in (0.5, 0.7, 3, 100)},
                 'perm_min_score': topk(score, None, batch[shuffle], min_score=0.4)}

G['reprs'] = {'topk': repr(TopKPooling(F)), 'topk_min_score': repr(TopKPooling(F, min_score=0.1)),
              'sag': repr(SAGPooling(F)), 'sag_gcn': repr(SAGPooling(F, GNN=GCNConv)),
              'select': repr(TopKPooling(F).select), 'connect': repr(TopKPooling(F).connect)}
G['keys'] = {'topk': {k: tuple(v.shape) for k, v in TopKPooling(F).state_dict().items()},
             'sag': {k: tuple(v.shape) for k, v in SAGPooling(F).state_dict().items()},
             'sag_gcn': {k: tuple(v.shape)
                         for k, v in SAGPooling(F, GNN=GCNConv).state_dict().items()}}

for name, case in C.items():
    print(f"{name}: seed {case['seed']}  kept {case['perm'].numel()} nodes "
          f"{case['edge_index'].size(1)} edges  ref_err "
          + '  '.join(f'{k} {v:.1e}' for k, v in case['ref_err'].items()))
out_path = os.path.join(HERE, 'golden_pool_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
