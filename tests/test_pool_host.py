"""TopKPooling / SAGPooling without a GPU: every golden case (the real reference's outputs, stored
in tests/golden/golden_pool_v1.pt) through the generic route on CPU tensors, an unsorted batch
vector, state dicts, the count ``k``, the tie rule against a plain-Python restatement, the exports
and the entry points' argument checks."""
import ctypes

import pytest
import torch

from tests import _pool_ref as R

G = R.load_golden()


@pytest.mark.parametrize('name', sorted(G['cases']))
@pytest.mark.parametrize('fuse', [False, True])
def test_golden_case_on_cpu(name, fuse):
    """(``fuse=True`` changes nothing for host tensors: they always take the generic route)"""
    R.check_golden_case(name, 'cpu', fuse)


def test_unsorted_batch_vector():
    from pytorch_geometric_amd.nn import topk
    U = G['unsorted']
    for ratio, want in U['perm'].items():
        got = topk(U['score'], ratio, U['batch'])
        assert torch.equal(got, want), ratio
    assert torch.equal(topk(U['score'], None, U['batch'], min_score=0.4), U['perm_min_score'])
    with pytest.raises(ValueError):
        topk(U['score'], None, U['batch'])


def test_state_dicts_and_reprs():
    import pytorch_geometric_amd.nn as nn
    F = G['meta']['F']
    made = {'topk': nn.TopKPooling(F), 'sag': nn.SAGPooling(F),
            'sag_gcn': nn.SAGPooling(F, GNN=nn.GCNConv)}
    for key, layer in made.items():
        assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == G['keys'][key]
        assert repr(layer) == G['reprs'][key]
    assert repr(nn.TopKPooling(F, min_score=0.1)) == G['reprs']['topk_min_score']
    assert repr(made['topk'].select) == G['reprs']['select']
    assert repr(made['topk'].connect) == G['reprs']['connect']
    # the reference's state loads here, and what this layer saves has the reference's keys, shapes
    # and values: it loads there
    for name, case in G['cases'].items():
        layer = R.make_layer(case, nn)
        saved = layer.state_dict()
        assert list(saved) == list(case['state'])
        for k, v in case['state'].items():
            assert torch.equal(saved[k], v) and saved[k].dtype == v.dtype
    with pytest.raises(ValueError):
        nn.TopKPooling(F, ratio=None)
    # initialisation: uniform(in_channels, weight), bound 1 / sqrt(in_channels)
    w = nn.TopKPooling(400).select.weight.detach()
    assert tuple(w.shape) == (1, 400) and float(w.abs().max()) <= 1 / 20 and float(w.std()) > 0.02


def test_fuse_attribute_and_switch():
    import pytorch_geometric_amd.nn as nn
    from pytorch_geometric_amd.nn.pool import _fuse
    assert set(_fuse.DEFAULTS) == {'TopKPooling', 'SAGPooling', 'topk', 'filter_adj'}
    layer = nn.SAGPooling(4)
    assert layer.fuse == _fuse.fuse_default('SAGPooling')
    assert nn.TopKPooling(4).fuse == _fuse.fuse_default('TopKPooling')
    layer.fuse = False
    assert layer.select.fuse is False and layer.connect.fuse is False and layer.fuse is False
    layer.fuse = True
    assert layer.select.fuse is True and layer.connect.fuse is True
    assert 'fuse' not in layer.state_dict()


def test_k_is_the_reference_expression():
    from pytorch_geometric_amd.nn.pool.select.topk import num_selected
    n = torch.arange(1, 301)
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        for ratio in [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1e-9]:
            want = (float(ratio) * n.to(dtype)).ceil().to(torch.long)     # topk.py:34
            assert torch.equal(num_selected(ratio, n, dtype), want)
            assert torch.equal(num_selected(ratio, n.int(), dtype), want)
            if dtype == torch.float32:
                assert want.tolist() == [R.num_kept(ratio, int(i)) for i in n]
    for ratio in (1, 3, 100, 1.0, 2.5):
        assert num_selected(ratio, n, torch.float32).tolist() == [int(ratio)] * 300   # topk.py:32


def test_tie_rule_against_plain_python():
    from pytorch_geometric_amd.nn import topk
    sizes = [1, 2, 3, 63, 64, 65, 0, 70, 5]
    batch = R.batch_of(sizes)
    n = batch.numel()
    g = torch.Generator().manual_seed(3)
    inf, nan = float('inf'), float('nan')
    scores = {'equal': torch.full((n, ), 0.25),
              'zeros': torch.where(torch.rand(n, generator=g) < 0.5, 0.0, -0.0),
              'few values': torch.randint(0, 4, (n, ), generator=g).float() - 1.0,
              'inf': torch.tensor([inf, -inf, 1.0, 0.0, -0.0])[torch.randint(0, 5, (n, ),
                                                                             generator=g)]}
    for where in ('first', 'last', 'middle'):
        s = torch.randn(n, generator=g)
        start = 0
        for size in sizes:
            if size > 0:
                s[start + {'first': 0, 'last': size - 1, 'middle': size // 2}[where]] = nan
            start += size
        s[140], s[141] = nan, -nan      # two NaNs in one graph: index order
        scores['nan ' + where] = s
    for what, s in scores.items():
        for ratio in (0.5, 0.7, 1e-9, 1, 3, 100):
            want = R.topk_ref(s.tolist(), sizes, ratio)
            assert topk(s, ratio, batch).tolist() == want, (what, ratio)
            assert topk(s, ratio, batch, fuse=True).tolist() == want, (what, ratio)


def test_filter_adj_on_cpu():
    from pytorch_geometric_amd.nn import filter_adj
    ei = torch.tensor([[0, 1, 1, 2, 3, 3, 3], [1, 0, 1, 3, 2, 3, 3]])
    attr = torch.arange(7.0)
    out, oa = filter_adj(ei, attr, torch.tensor([3, 1]), num_nodes=4)
    assert out.tolist() == [[1, 0, 0], [1, 0, 0]] and oa.tolist() == [2.0, 5.0, 6.0]
    out, oa = filter_adj(ei, None, torch.tensor([3, 1]), torch.tensor([5, 7]))
    assert out.tolist() == [[7, 5, 5], [7, 5, 5]] and oa is None


def test_new_symbols_are_exported():
    import pytorch_geometric_amd.nn as nn
    from pytorch_geometric_amd import _functions, _native
    from pytorch_geometric_amd.nn import pool
    from pytorch_geometric_amd.nn.pool import connect, select
    for name in ('TopKPooling', 'SAGPooling', 'topk', 'filter_adj'):
        assert name in nn.__all__ and name in pool.__all__ and getattr(nn, name) is getattr(pool, name)
    assert select.__all__ == ['Select', 'SelectOutput', 'SelectTopK', 'topk']
    assert connect.__all__ == ['Connect', 'ConnectOutput', 'FilterEdges', 'filter_adj']
    assert (_native.TOPK_WAVE_NODES, _native.TOPK_GROUP) == (64, 4)
    assert _native.TOPK_MAX_NODES >= 1024
    assert hasattr(_functions, 'GatherScaleFunction')
    with pytest.raises(ValueError):
        select.SelectOutput(torch.zeros(2, dtype=torch.long), 3, torch.zeros(3, dtype=torch.long), 3)
    with pytest.raises(ValueError):
        connect.ConnectOutput(torch.zeros(3, 2, dtype=torch.long))


def test_entry_points_validate_without_gpu():
    """Null pointers, negative sizes and F < 1 are rejected before any device work."""
    from pytorch_geometric_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    p = P(16)   # (never dereferenced: every call below is rejected or has nothing to do)
    # select
    assert lib.pygamd_topk_select(p, -1, p, 1, 2, p, p, 0, 4, p, p, None) == 1
    assert lib.pygamd_topk_select(p, 8, p, 7, 2, p, p, 4, 4, p, p, None) == 1       # idx_dtype
    assert lib.pygamd_topk_select(p, 8, None, 1, 2, p, p, 4, 4, p, p, None) == 1
    assert lib.pygamd_topk_select(p, 8, p, 1, 2, None, p, 4, 4, p, p, None) == 1
    assert lib.pygamd_topk_select(p, 8, p, 1, 2, p, None, 4, 4, p, p, None) == 1
    assert lib.pygamd_topk_select(None, 8, p, 1, 2, p, p, 4, 4, p, p, None) == 1
    assert lib.pygamd_topk_select(p, 8, p, 1, 2, p, p, 4, 4, None, p, None) == 1
    assert lib.pygamd_topk_select(p, 8, p, 1, 2, p, p, 9, 4, p, p, None) == 1       # M > N
    assert lib.pygamd_topk_select(p, 8, p, 1, -2, p, p, 4, 4, p, p, None) == 1
    assert lib.pygamd_topk_select(p, 8, p, 1, 2, p, p, 4, -4, p, p, None) == 1
    assert lib.pygamd_topk_select(p, 4000, p, 1, 2, p, p, 4, 1025, p, p, None) == 2  # envelope
    assert lib.pygamd_topk_select(p, 8, p, 1, 2, p, p, 0, 4, None, None, None) == 0  # nothing kept
    # gather-scale
    fwd, bwd = lib.pygamd_gather_scale_forward, lib.pygamd_gather_scale_backward
    assert fwd(p, 8, 4, 0, p, p, 2, 1.0, p, 8, p, None) == 1                        # F < 1
    assert fwd(p, 4, 4, 8, p, p, 2, 1.0, p, 8, p, None) == 1                        # ldx < F
    assert fwd(p, 8, 4, 8, p, p, 2, 1.0, p, 4, p, None) == 1                        # ldo < F
    assert fwd(p, 8, -4, 8, p, p, 2, 1.0, p, 8, p, None) == 1
    assert fwd(p, 8, 4, 8, p, p, -2, 1.0, p, 8, p, None) == 1
    for bad in range(4):
        args = [p, 8, 4, 8, p, p, 2, 1.0, p, 8, p, None]
        args[(0, 4, 5, 8)[bad]] = None
        assert fwd(*args) == 1
    assert fwd(None, 8, 0, 8, None, None, 0, 1.0, None, 8, None, None) == 0
    assert bwd(p, 8, 4, 0, p, p, 2, 1.0, p, 8, None, p, 8, p, None) == 1
    assert bwd(p, 8, 4, 8, p, p, 2, 1.0, p, 4, None, p, 8, p, None) == 1            # ldg < F
    assert bwd(p, 8, 4, 8, p, p, 2, 1.0, p, 8, None, p, 4, p, None) == 1            # ldgx < F
    assert bwd(p, 8, 4, 8, p, p, 2, 1.0, None, 8, None, p, 8, p, None) == 1
    assert bwd(p, 8, 4, 8, p, None, 2, 1.0, p, 8, None, p, 8, p, None) == 1
    assert bwd(p, 8, 4, 8, p, p, -1, 1.0, p, 8, None, p, 8, p, None) == 1
    assert bwd(None, 8, 0, 8, None, None, 0, 1.0, None, 8, None, None, 8, None, None) == 0
    # edge filter
    n = ctypes.c_size_t(123)
    assert lib.pygamd_filter_edges_workspace_size(-1, ctypes.byref(n)) == 1
    assert lib.pygamd_filter_edges_workspace_size(5, None) == 1
    assert lib.pygamd_filter_edges_workspace_size(0, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.pygamd_filter_edges_workspace_size(3 * 4096 + 5, ctypes.byref(n)) == 0
    assert n.value == (4 + 1) * 8
    flt = lib.pygamd_filter_edges
    ok = [p, 1, p, 1, 1, 10, p, 4, p, p, p, p, p, n.value, None]
    for i in (0, 2, 6, 8, 9, 10, 11):
        args = list(ok)
        args[i] = None
        assert flt(*args) == 1, i
    for i, v in ((1, 0), (3, 0), (4, 9), (5, -1), (7, -1)):
        args = list(ok)
        args[i] = v
        assert flt(*args) == 1, i
    assert flt(*(ok[:12] + [None, 0, None])) == 3
    assert flt(*(ok[:12] + [p, 8, None])) == 3
    assert flt(None, 1, None, 1, 1, 0, None, 0, None, None, None, None, None, 0, None) == 0
