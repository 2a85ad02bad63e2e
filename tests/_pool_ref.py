"""What the pooling tests share (tests/test_pool_host.py, tests/test_gpu_pool.py): the golden
(tests/golden/golden_pool_v1.pt), a plain-Python restatement of the per-graph top-k selection —
``sorted`` by ``(-score, index)`` with NaN first, nothing of the code under test — and the runner
of the golden layer cases.  Tolerances are ``tests/_norm_ref.tol_of``: ``max(2e-5, 2 x the float32
error of the reference on that tensor)``."""
import math
import os

import torch

from tests._norm_ref import scaled_err, tol_of
from tests._util import assert_close_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_G = None


def load_golden():
    global _G
    if _G is None:
        _G = torch.load(os.path.join(ROOT, 'tests', 'golden', 'golden_pool_v1.pt'),
                        map_location='cpu', weights_only=False)
    return _G


def num_kept(ratio, n: int) -> int:
    if ratio >= 1:
        return min(int(ratio), n)
    return min(int(math.ceil(float(torch.tensor(float(ratio)) * torch.tensor(float(n))))), n)


def topk_ref(score, sizes, ratio):
    """Graph by graph the best ``k`` nodes: score descending (any NaN above every number, -0.0 ==
    +0.0), then node index ascending.  ``score``: a list of Python floats."""
    perm, start = [], 0
    for n in sizes:
        ids = list(range(start, start + n))
        start += n

        def key(i):
            s = score[i]
            return (0, 0.0, i) if s != s else (1, -(s + 0.0), i)
        perm += sorted(ids, key=key)[:num_kept(ratio, n)]
    return perm


def batch_of(sizes, device='cpu', dtype=torch.int64):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(
        device=device, dtype=dtype)


class host:
    """Plain-torch restatements of the two score layers of the SAGPooling cases, with the
    reference's parameter names, for host tensors: this package's conv layers run on the device
    only, and what the host tests check is the pooling behind them."""

    class GraphConv(torch.nn.Module):
        def __init__(self, in_channels, out_channels):
            super().__init__()
            self.lin_rel = torch.nn.Linear(in_channels, out_channels)
            self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=False)

        def reset_parameters(self):
            self.lin_rel.reset_parameters()
            self.lin_root.reset_parameters()

        def forward(self, x, edge_index):
            agg = torch.zeros_like(x).index_add_(0, edge_index[1], x[edge_index[0]])
            return self.lin_rel(agg) + self.lin_root(x)

    class GCNConv(torch.nn.Module):
        def __init__(self, in_channels, out_channels):
            super().__init__()
            self.bias = torch.nn.Parameter(torch.zeros(out_channels))
            self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)

        def reset_parameters(self):
            self.lin.reset_parameters()

        def forward(self, x, edge_index):
            n = x.size(0)
            loops = torch.arange(n)
            ei = edge_index[:, edge_index[0] != edge_index[1]]
            row, col = torch.cat([ei[0], loops]), torch.cat([ei[1], loops])
            dis = torch.zeros(n, dtype=x.dtype).index_add_(
                0, col, torch.ones(col.numel(), dtype=x.dtype)).pow(-0.5)
            h = self.lin(x)
            out = torch.zeros_like(h).index_add_(0, col, (dis[row] * dis[col]).view(-1, 1) * h[row])
            return out + self.bias


def make_layer(case, nn, gnns=None):
    """``gnns``: where the SAGPooling cases take their score layer from (default: ``nn``)"""
    G = load_golden()
    if case['kind'] == 'topk':
        layer = nn.TopKPooling(G['meta']['F'], **case['kwargs'])
    else:
        layer = nn.SAGPooling(G['meta']['F'], GNN=getattr(gnns or nn, case['gnn']),
                              **case['kwargs'])
    layer.load_state_dict(case['state'])
    return layer


def _randn(shape, seed, device):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64).float().to(device)


def run_golden_case(name, device, fuse, index_dtype=torch.int64):
    """golden case ``name`` through this package's layer on ``device``: (layer, outputs)"""
    import pytorch_geometric_amd.nn as nn
    G = load_golden()
    case = G['cases'][name]
    layer = make_layer(case, nn, host if str(device) == 'cpu' else None).to(device)
    layer.fuse = fuse
    assert repr(layer) == case['repr']
    x = G['x'].to(device).clone().requires_grad_(True)
    ea = None
    if case['attr'] is not None:
        ea = G['edge_attr'][case['attr']].to(device).clone().requires_grad_(True)
    batch = G['batch'].to(device=device, dtype=index_dtype) if case['use_batch'] else None
    out, ei, eo, bo, perm, score = layer(x, G['edge_index'].to(device), ea, batch)
    seeds = G['meta']['grad_seeds']
    loss = (out * _randn(out.shape, seeds['out'], device)).sum() \
        + (score * _randn(score.shape, seeds['score'], device)).sum()
    if eo is not None:
        loss = loss + (eo * _randn(eo.shape, seeds['edge_attr'], device)).sum()
    loss.backward()
    got = {'out': out, 'score': score, 'grad_x': x.grad, 'perm': perm, 'edge_index': ei,
           'batch': bo}
    got.update({f'grad_params.{n}': p.grad for n, p in layer.named_parameters()})
    if ea is not None:
        got['edge_attr'], got['grad_edge_attr'] = eo, ea.grad
    return layer, got


def check_golden_case(name, device, fuse, index_dtype=torch.int64):
    G = load_golden()
    case = G['cases'][name]
    layer, got = run_golden_case(name, device, fuse, index_dtype)
    for key in ('perm', 'edge_index', 'batch'):   # exact
        assert got[key].dtype == torch.int64 or key == 'batch'
        assert torch.equal(got[key].cpu().long(), case[key]), f'{name} {key}'
    err = case['ref_err']
    assert set(err) == set(got) - {'perm', 'edge_index', 'batch'}
    for key in err:
        print(f'{name} {key}: err {scaled_err(got[key], case[key]):.2e} '
              f'tol {tol_of(err[key]):.2e}')
    for key in err:
        assert got[key].shape == case[key].shape, f'{name} {key}'
        assert_close_scaled(got[key].double(), case[key].double(), tol=tol_of(err[key]),
                            what=f'{name} {key}')
    return layer, got
