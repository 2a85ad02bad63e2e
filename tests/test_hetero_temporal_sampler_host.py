"""Temporal heterogeneous sampling without a GPU: the plain-Python restatement
(``tests/_hetero_temporal_ref.py``) reproduces answers worked out by hand; the two C entry points
are declared, exported and in the ctypes table and reject bad arguments before any launch; and
``HeteroNeighborSampler``, ``HeteroNeighborLoader`` and the ``backend`` adapter validate the time
arguments (rules 1 and 6) before touching the device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests._hetero_temporal_ref import edge_level_loader_graph, hetero_temporal_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUYS, REV = ('u', 'buys', 'i'), ('i', 'rev', 'u')


def _lib_or_skip():
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    return _lib.load()


def _two_type_graph():
    """Users (timed: 5, 1, 3) buy items (untimed).  Item 0 is bought by u0, u1, u2, item 1 by u1;
    its time-sorted column is u1 (1), u2 (3), u0 (5).  'rev' points back: u1 <- i0, u2 <- i0, i1."""
    eid = {BUYS: torch.tensor([[0, 1, 2, 1], [0, 0, 0, 1]]),
           REV: torch.tensor([[0, 0, 1], [1, 2, 2]])}
    return eid, {'u': 3, 'i': 2}, {'u': torch.tensor([5, 1, 3])}


# ---- the restatement: known answers worked out by hand ---------------------------------------------
def test_restatement_two_types_one_timed():
    eid, nn, nt = _two_type_graph()
    fan = {BUYS: [-1, -1], REV: [-1, -1]}
    # two trees from the same item: tree 0 sees times <= 3 (u1, u2), tree 1 times <= 0 (nobody)
    node, row, col, edge, batch, n_nodes, n_edges = hetero_temporal_sample(
        eid, nn, fan, 'i', [0, 0], node_time=nt, seed_time=[3, 0])
    assert node == {'u': [1, 2], 'i': [0, 0, 1]}
    assert batch == {'u': [0, 0], 'i': [0, 1, 0]}
    assert edge[BUYS] == [1, 2] and row[BUYS] == [0, 1] and col[BUYS] == [0, 0]
    # 'rev' is untimed (items carry no time): every in-edge of u1 and u2, in edge_index order;
    # item 0 of tree 0 is the seed, item 1 of tree 0 is new
    assert edge[REV] == [0, 1, 2] and row[REV] == [0, 0, 2] and col[REV] == [0, 1, 1]
    assert n_nodes == {'u': [0, 2, 0], 'i': [2, 0, 1]}
    assert n_edges == {BUYS: [2, 0], REV: [0, 3]}
    # 'last' with k = 1: the most recent eligible buyer of every tree
    node, row, col, edge, batch, n_nodes, n_edges = hetero_temporal_sample(
        eid, nn, {BUYS: [1], REV: [0]}, 'i', [0, 0], node_time=nt, seed_time=[5, 1],
        strategy='last')
    assert edge[BUYS] == [0, 1] and node['u'] == [0, 1] and batch['u'] == [0, 1]
    assert n_edges == {BUYS: [2], REV: [0]}


def test_restatement_seed_time_default_and_refusals():
    eid, nn, nt = _two_type_graph()
    fan = {BUYS: [-1], REV: [-1]}
    # seeds of the timed type default to their own time
    node, _, _, edge, _, _, n_edges = hetero_temporal_sample(eid, nn, fan, 'u', [2, 0], node_time=nt)
    assert edge[REV] == [1, 2] and n_edges[BUYS] == [0]
    with pytest.raises(ValueError, match='needs the seed times'):
        hetero_temporal_sample(eid, nn, fan, 'i', [0], node_time=nt)
    with pytest.raises(ValueError, match='random'):
        hetero_temporal_sample(eid, nn, {BUYS: [2], REV: [2]}, 'i', [0], node_time=nt,
                               seed_time=[9])
    with pytest.raises(ValueError, match='random'):
        hetero_temporal_sample(eid, nn, {BUYS: [3], REV: [3]}, 'i', [0], node_time=nt,
                               seed_time=[9], replace=True)


def test_restatement_reference_edge_level_graph():
    """The reference's edge-level loader test: with seed time 4, every batch's edge times are
    <= 4.  By hand: seed 2 reaches 1 over edge 2 (time 2), then 0 over edge 0 and 2 over edge 3;
    seed 4's only in-edge has time 6."""
    eid, nn, et_time = edge_level_loader_graph()
    (et, ei), = eid.items()
    fan = {et: [-1, -1]}
    for seed in range(5):
        node, row, col, edge, batch, n_nodes, n_edges = hetero_temporal_sample(
            eid, nn, fan, 'A', [seed], edge_time=et_time, seed_time=[4])
        assert all(int(et_time[et][e]) <= 4 for e in edge[et])
        assert all(node['A'][r] == int(ei[0, e]) and node['A'][c] == int(ei[1, e])
                   for r, c, e in zip(row[et], col[et], edge[et]))
        if seed == 2:
            assert node['A'] == [2, 1, 0] and edge[et] == [2, 0, 3]
            assert row[et] == [1, 2, 0] and col[et] == [0, 1, 1]
            assert n_nodes['A'] == [1, 1, 1] and n_edges[et] == [1, 2]
        if seed == 4:
            assert node['A'] == [4] and n_edges[et] == [0, 0]


# ---- the C entry points ----------------------------------------------------------------------------
@pytest.mark.parametrize('sym,n_args', [('pygamd_hetero_sample_temporal_window', 17),
                                        ('pygamd_hetero_sample_neighbors_temporal', 17)])
def test_entry_points_are_declared_exported_and_typed(sym, n_args):
    from pytorch_geometric_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'pyg_amd.h')).read()
    assert re.search(r'PYGAMD_API\s+int\s+' + sym + r'\s*\(', text)
    _, args = _lib.SIGNATURES[sym]
    assert len(args) == n_args
    _lib_or_skip()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True,
                         text=True).stdout
    assert re.search(r' T ' + sym + r'\b', out)
    assert _lib.ABI_VERSION == 11


def test_entry_points_validate_without_gpu():
    from pytorch_geometric_amd import _lib
    lib = _lib_or_skip()
    fake = ctypes.c_void_p(64)  # never dereferenced: every call below is rejected before a launch
    I64 = _lib.IDX_I64

    def arr(*v):
        return (ctypes.c_int64 * len(v))(*v)

    ib, tab = arr(0, 5), arr(0, 0, 0, 3)

    def window(colptr=fake, row=fake, dt=I64, time=fake, level=0, frontier=fake, ftime=fake,
               item_begin=ib, table=tab, n_et=1, mask=1, replace=0, strategy=0, lo=fake, hi=fake,
               cnt=fake):
        return lib.pygamd_hetero_sample_temporal_window(
            colptr, row, dt, time, level, frontier, ftime, item_begin, table, n_et, mask, replace,
            strategy, lo, hi, cnt, None)

    assert window(level=2) != 0 and window(level=-1) != 0
    assert window(strategy=2) != 0 and window(strategy=-1) != 0
    assert window(table=arr(0, 0, 0, 65)) == 2            # UNSUPPORTED: fan-out above 64
    assert window(table=arr(0, 0, 0, -2)) != 0
    assert window(dt=7) != 0
    assert window(item_begin=arr(0, -1)) != 0 and window(item_begin=arr(1, 5)) != 0
    assert window(n_et=0) != 0 and window(n_et=65) != 0
    assert window(mask=2) != 0                            # a timed bit past the edge types
    for name in ('colptr', 'row', 'time', 'frontier', 'ftime', 'lo', 'hi', 'cnt'):
        assert window(**{name: None}) != 0, name
    assert window(item_begin=arr(0, 0)) == 0              # an empty work list launches nothing

    def draw(row=fake, perm=fake, dt=I64, frontier=fake, lo=fake, hi=fake, offsets=fake,
             item_begin=ib, table=tab, n_et=1, src=fake, col=fake, edge=fake):
        return lib.pygamd_hetero_sample_neighbors_temporal(
            row, perm, dt, frontier, lo, hi, offsets, item_begin, table, n_et, 0, 0, src, col,
            edge, None, None)

    assert draw(table=arr(0, 0, 0, 65)) == 2
    assert draw(dt=7) != 0
    assert draw(item_begin=arr(0, 3, 2), table=arr(0, 0, 0, 3, 0, 0, 0, 3), n_et=2) != 0
    assert draw(n_et=0) != 0
    for name in ('row', 'perm', 'frontier', 'lo', 'hi', 'offsets', 'src', 'col', 'edge'):
        assert draw(**{name: None}) != 0, name
    assert draw(item_begin=arr(0, 0)) == 0


# ---- the sampler validates before any device work --------------------------------------------------
def _construct(**kw):
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler
    eid, nn, _ = _two_type_graph()
    return HeteroNeighborSampler(eid, nn, kw.pop('num_neighbors', [2, 2]), **kw)


L = torch.long


@pytest.mark.parametrize('kw,match', [
    (dict(node_time={'u': torch.zeros(3, dtype=L)}, edge_time={BUYS: torch.zeros(4, dtype=L)}),
     "either 'node_time' or 'edge_time'"),
    (dict(node_time={'x': torch.zeros(3, dtype=L)}), 'not a node type'),
    (dict(edge_time={('u', 'sells', 'i'): torch.zeros(4, dtype=L)}), 'not an edge type'),
    (dict(node_time={'u': torch.zeros(4, dtype=L)}), '1-D tensor with 3 entries'),
    (dict(edge_time={BUYS: torch.zeros(3, dtype=L)}), '1-D tensor with 4 entries'),
    (dict(edge_time={'i__rev__u': torch.zeros(4, dtype=L)}), '1-D tensor with 3 entries'),
    (dict(node_time={'u': torch.zeros(3)}), 'integer tensor'),
    (dict(edge_time={BUYS: torch.zeros(4, dtype=torch.bool)}), 'integer tensor'),
    (dict(node_time={'u': torch.zeros(3, dtype=torch.complex64)}), 'integer tensor'),
    (dict(node_time={'u': [0, 0, 0]}), '1-D tensor'),
    (dict(node_time=torch.zeros(3, dtype=L)), 'temporal heterogeneous'),
    (dict(node_time={'u': torch.zeros(3, dtype=L)}, temporal_strategy='first'),
     'unknown temporal_strategy'),
    (dict(node_time={'u': torch.zeros(3, dtype=L)}, edge_weight=torch.ones(4)),
     'weighted heterogeneous'),
    (dict(node_time={'u': torch.zeros(3, dtype=L)}, subgraph_type='induced'),
     "'directional' only"),
])
def test_sampler_refuses_bad_times_before_device_work(kw, match):
    _lib_or_skip()
    with pytest.raises(ValueError, match=match):
        _construct(**kw)


def test_valid_times_reach_the_device_check():
    """Valid dicts (string and pair keys normalised, types missing) pass the time rules: host
    tensors are then refused as such."""
    _lib_or_skip()
    for kw in (dict(node_time={'u': torch.zeros(3, dtype=torch.int32)}),
               dict(node_time={}),
               dict(edge_time={'u__buys__i': torch.zeros(4, dtype=L)}),
               dict(edge_time={BUYS: torch.zeros(4, dtype=L), REV: torch.zeros(3, dtype=L)})):
        with pytest.raises(ValueError, match='HIP device'):
            _construct(**kw)


def _bare(**attrs):
    """A sampler made with ``__new__``: the seed-time rules read host-side facts only."""
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler
    smp = HeteroNeighborSampler.__new__(HeteroNeighborSampler)
    smp.node_types = ['u', 'i']
    smp._type_index = {'u': 0, 'i': 1}
    smp.num_nodes = {'u': 3, 'i': 2}
    smp.node_base = [0, 3, 5]
    for k, v in attrs.items():
        setattr(smp, k, v)
    return smp


def test_missing_seed_times_are_refused():
    seeds = torch.tensor([0, 1])
    edge_level = _bare(is_temporal=True, edge_level=True, timed_node_types=set())
    with pytest.raises(ValueError, match='needs the seed times'):
        edge_level.seed_time('u', seeds)
    with pytest.raises(ValueError, match='needs the seed times'):
        edge_level.sample_from_nodes(('u', seeds))
    node_level = _bare(is_temporal=True, edge_level=False, timed_node_types={'u'})
    with pytest.raises(ValueError, match='needs the seed times'):
        node_level.seed_time('i', seeds)
    with pytest.raises(ValueError, match='one entry per seed'):
        node_level.seed_time('i', seeds, torch.zeros(3, dtype=L))
    with pytest.raises(ValueError, match='integer tensor'):
        node_level.seed_time('i', seeds, torch.zeros(2))
    plain = _bare(is_temporal=False)
    with pytest.raises(ValueError, match='temporal'):
        plain.sample_from_nodes(('u', seeds), time=torch.zeros(2, dtype=L))
    with pytest.raises(ValueError, match='temporal'):
        plain.seed_time('u', seeds)


def test_loader_refuses_input_time_without_times():
    from pytorch_geometric_amd.loader import HeteroBatch, HeteroNeighborLoader
    eid, nn, _ = _two_type_graph()
    x = {t: torch.zeros(n, 2) for t, n in nn.items()}
    with pytest.raises(ValueError, match="conflicting 'input_time' and 'time_attr'"):
        HeteroNeighborLoader(x, eid, [1], input_nodes='u', input_time=torch.zeros(3, dtype=L))
    # the time rules come before the device check in the loader too
    with pytest.raises(ValueError, match='integer tensor'):
        HeteroNeighborLoader(x, eid, [1], input_nodes='u', node_time={'u': torch.zeros(3)})
    assert HeteroBatch.__dataclass_fields__['seed_time'].default is None


def test_adapter_collects_time_attr():
    try:
        from oracle import make_ref
        make_ref.import_reference()
        from torch_geometric.data import HeteroData
    except ImportError:
        pytest.skip('torch_geometric cannot be imported')
    _lib_or_skip()
    from pytorch_geometric_amd import backend
    eid, nn, nt = _two_type_graph()
    data = HeteroData()
    for t, n in nn.items():
        data[t].num_nodes = n
    for et, ei in eid.items():
        data[et].edge_index = ei
    with pytest.raises(ValueError, match='neither a node-level or edge-level.*heterogeneous'):
        backend.neighbor_sampler(data, [1], time_attr='t')
    with pytest.raises(ValueError, match='weighted heterogeneous'):
        backend.neighbor_sampler(data, [1], weight_attr='w')
    data['u'].t = nt['u']
    data[BUYS].t = torch.zeros(4, dtype=L)
    with pytest.raises(ValueError, match='both node-level and edge-level'):
        backend.neighbor_sampler(data, [1], time_attr='t')
    del data[BUYS].t               # node level alone: collected, then the device check
    with pytest.raises(ValueError, match='HIP device'):
        backend.neighbor_sampler(data, [1], time_attr='t')
