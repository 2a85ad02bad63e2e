"""Heterogeneous sampling without a GPU: the three C entry points are declared, exported and in
the ctypes table and reject bad arguments before any launch; ``HeteroNeighborSampler`` validates
its arguments (the reference's ``NumNeighbors`` rules and wording, the refused options) before
touching the device; and the plain-Python restatement of the hop loop reproduces the reference's
known answer (test/loader/test_neighbor_loader.py:756-793)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests._hetero_ref import (SAMPLED_INFO_EDGES, SAMPLED_INFO_NODES, hetero_sample,
                               sampled_info_graph)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP, PA, AP = ('paper', 'to', 'paper'), ('paper', 'to', 'author'), ('author', 'to', 'paper')


def _lib_or_skip():
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    return _lib.load()


def _graph(dtype=torch.int64):
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]], dtype=dtype)
    return {PP: ei, PA: ei.clone(), AP: ei.clone()}, {'paper': 3, 'author': 3}


@pytest.mark.parametrize('sym,n_args', [('pygamd_hetero_sample_counts', 9),
                                        ('pygamd_hetero_sample_neighbors', 16),
                                        ('pygamd_hetero_split', 20)])
def test_hetero_entry_points_are_declared_exported_and_typed(sym, n_args):
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


def test_hetero_entry_points_validate_without_gpu():
    from pytorch_geometric_amd import _lib
    lib = _lib_or_skip()
    fake = ctypes.c_void_p(64)  # never dereferenced: every call below is rejected before a launch
    I64 = _lib.IDX_I64

    def arr(*v):
        return (ctypes.c_int64 * len(v))(*v)

    ib, tab = arr(0, 5), arr(0, 0, 0, 3)
    assert lib.pygamd_hetero_sample_counts(fake, I64, fake, ib, tab, 0, 0, fake, None) != 0
    assert lib.pygamd_hetero_sample_counts(fake, I64, fake, ib, tab, 65, 0, fake, None) != 0
    assert lib.pygamd_hetero_sample_counts(fake, I64, fake, arr(1, 5), tab, 1, 0, fake,
                                           None) != 0
    assert lib.pygamd_hetero_sample_counts(fake, I64, fake, arr(0, -1), tab, 1, 0, fake,
                                           None) != 0
    assert lib.pygamd_hetero_sample_counts(fake, I64, fake, ib, arr(0, 0, 0, 65), 1, 0, fake,
                                           None) == 2  # UNSUPPORTED: fan-out above 64
    assert lib.pygamd_hetero_sample_counts(fake, I64, fake, ib, arr(0, 0, 0, -2), 1, 0, fake,
                                           None) != 0
    assert lib.pygamd_hetero_sample_counts(fake, I64, None, ib, tab, 1, 0, fake, None) != 0
    assert lib.pygamd_hetero_sample_counts(fake, 7, fake, ib, tab, 1, 0, fake, None) != 0
    # an empty work list launches nothing
    assert lib.pygamd_hetero_sample_counts(fake, I64, fake, arr(0, 0), tab, 1, 0, fake, None) == 0
    assert lib.pygamd_hetero_sample_neighbors(fake, fake, None, I64, fake, fake, ib, tab, 1, 0, 0,
                                              fake, fake, fake, None, None) != 0
    assert lib.pygamd_hetero_sample_neighbors(fake, fake, fake, I64, fake, fake, ib, tab, 0, 0, 0,
                                              fake, fake, fake, None, None) != 0
    nb, cp = arr(0, 3, 6), arr(0, 0)
    assert lib.pygamd_hetero_split(2, fake, I64, 4, fake, nb, cp, 2, fake, fake, ib, 1, None,
                                   None, None, fake, fake, None, fake, None) != 0
    assert lib.pygamd_hetero_split(0, fake, I64, 4, fake, nb, cp, 0, fake, fake, ib, 1, None,
                                   None, None, fake, fake, None, fake, None) != 0
    assert lib.pygamd_hetero_split(1, fake, I64, 4, fake, nb, cp, 2, fake, fake, ib, 1, fake,
                                   None, None, fake, fake, None, fake, None) != 0  # aux, no out
    assert lib.pygamd_hetero_split(1, fake, I64, 4, fake, nb, None, 2, fake, fake, ib, 1, None,
                                   None, None, fake, fake, None, fake, None) != 0
    assert lib.pygamd_hetero_split(1, fake, I64, 0, fake, nb, cp, 2, fake, fake, ib, 1, None,
                                   None, None, fake, fake, None, fake, None) == 0  # m = 0


# ---- num_neighbors: the reference's NumNeighbors rules and error texts ----------------------------
def test_num_neighbors_rules():
    from pytorch_geometric_amd.sampler import hetero_num_neighbors
    ets = [PP, PA, AP]
    assert hetero_num_neighbors([3, 2], ets) == {et: [3, 2] for et in ets}
    got = hetero_num_neighbors({PP: [1], 'paper__to__author': [2], ('author', 'paper'): [-1]}, ets)
    assert got == {PP: [1], PA: [2], AP: [-1]}
    assert hetero_num_neighbors(({PP: [4, 4]}, [0, -1]), ets) == {PP: [4, 4], PA: [0, -1],
                                                                   AP: [0, -1]}
    with pytest.raises(ValueError, match='hops must be the same across all'):
        hetero_num_neighbors({PP: [-1], PA: [-1, -1], AP: [-1, -1]}, ets)
    with pytest.raises(ValueError, match="Not all edge types specified in 'num_neighbors' exist"):
        hetero_num_neighbors({PP: [1], ('author', 'to', 'author'): [1]}, ets)
    with pytest.raises(ValueError, match='Missing number of neighbors for edge type'):
        hetero_num_neighbors({PP: [1], PA: [1]}, ets)
    with pytest.raises(ValueError, match="'default' must be set to 'None'"):
        hetero_num_neighbors(type('NN', (), {'values': [1], 'default': [2]})(), ets)
    with pytest.raises(ValueError, match='integers >= -1'):
        hetero_num_neighbors([-2], ets)


def test_num_neighbors_reference_object():
    """The reference's ``NumNeighbors`` object is read through ``values`` / ``default``."""
    from types import SimpleNamespace
    from pytorch_geometric_amd.sampler import hetero_num_neighbors
    nn = SimpleNamespace(values={'paper__to__paper': [5]}, default=[1])
    assert hetero_num_neighbors(nn, [PP, AP]) == {PP: [5], AP: [1]}


# ---- the sampler validates before any device work --------------------------------------------------
def _construct(**kw):
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler
    eid, nn = kw.pop('graph', None) or _graph()
    return HeteroNeighborSampler(eid, nn, kw.pop('num_neighbors', [2, 2]), **kw)


@pytest.mark.parametrize('kw,match', [
    (dict(edge_weight=torch.ones(3)), 'weighted heterogeneous'),
    (dict(node_time=torch.zeros(3, dtype=torch.long)), 'temporal heterogeneous'),
    (dict(edge_time=torch.zeros(3, dtype=torch.long)), 'temporal heterogeneous'),
    (dict(subgraph_type='induced'), "'directional' only"),
    (dict(subgraph_type='bidirectional'), "'directional' only"),
    (dict(subgraph_type='both'), 'unknown subgraph_type'),
    (dict(num_neighbors={PP: [1], PA: [1, 1], AP: [1]}), 'hops must be the same'),
    (dict(num_neighbors=[65]), 'above 64'),
])
def test_sampler_refuses_before_device_work(kw, match):
    _lib_or_skip()
    with pytest.raises(ValueError, match=match):
        _construct(**kw)


def test_sampler_refuses_mixed_index_dtypes_and_bad_types():
    _lib_or_skip()
    eid, nn = _graph()
    eid[PA] = eid[PA].to(torch.int32)
    with pytest.raises(ValueError, match='one index dtype'):
        _construct(graph=(eid, nn))
    eid, nn = _graph()
    eid[('venue', 'to', 'paper')] = eid[PP]
    with pytest.raises(ValueError, match="missing from 'num_nodes_dict'"):
        _construct(graph=(eid, nn))
    eid, nn = _graph(torch.int32)
    nn['paper'] = 2 ** 31
    with pytest.raises(ValueError, match='does not fit in int32'):
        _construct(graph=(eid, nn))
    eid, nn = _graph()   # host tensors: refused as such once the arguments are valid
    with pytest.raises(ValueError, match='HIP device'):
        _construct(graph=(eid, nn))


def test_out_of_scope_entry_points_are_refused():
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler
    smp = HeteroNeighborSampler.__new__(HeteroNeighborSampler)
    with pytest.raises(NotImplementedError, match='link-level'):
        smp.sample_from_edges(torch.zeros(2, 1, dtype=torch.long))
    with pytest.raises(NotImplementedError, match='static-shape'):
        smp.sample_padded(torch.zeros(1, dtype=torch.long))


def test_homogeneous_sampler_still_refuses_input_type():
    from types import SimpleNamespace
    from pytorch_geometric_amd.sampler import NeighborSampler
    smp = NeighborSampler.__new__(NeighborSampler)
    inp = SimpleNamespace(node=torch.zeros(1, dtype=torch.long), input_id=None, time=None,
                          input_type='paper')
    with pytest.raises(NotImplementedError, match='heterogeneous'):
        smp.sample_from_nodes(inp)


# ---- the restatement -----------------------------------------------------------------------------
def test_restatement_known_answer():
    eid, nn = sampled_info_graph()
    fan = {et: [1, 2, 4] for et in eid}
    node, row, col, edge, batch, n_nodes, n_edges = hetero_sample(eid, nn, fan, 'paper', [0, 1])
    assert n_nodes == SAMPLED_INFO_NODES
    assert n_edges == SAMPLED_INFO_EDGES
    assert node['paper'] == [0, 1, 2, 3, 4, 7, 5, 10, 11, 12, 13]
    assert node['author'] == [2, 3, 4, 7, 5, 10, 11, 12, 13]
    assert batch is None
    for et in eid:
        s_t, _, d_t = et
        ei = eid[et]
        for r, c, e in zip(row[et], col[et], edge[et]):
            assert node[s_t][r] == int(ei[0, e]) and node[d_t][c] == int(ei[1, e])
    # disjoint: paper 7 is reached from both seeds, so it is two batch nodes (one per tree)
    node, row, col, edge, batch, n_nodes, n_edges = hetero_sample(eid, nn, fan, 'paper', [0, 1],
                                                                  disjoint=True)
    assert n_nodes == {'paper': [2, 2, 4, 8], 'author': [0, 2, 4, 8]}
    assert n_edges == {PP: [2, 4, 8], PA: [0, 4, 8], AP: [2, 4, 8]}
    assert batch['paper'][:2] == [0, 1]
    assert node['paper'][2:6] == [2, 3, 4, 7] and batch['paper'][2:6] == [0, 1, 0, 0]
    for et in eid:
        s_t, _, d_t = et
        assert all(batch[s_t][r] == batch[d_t][c] for r, c in zip(row[et], col[et]))


def test_restatement_refuses_random_draws():
    eid, nn = sampled_info_graph()
    with pytest.raises(ValueError, match='random'):
        hetero_sample(eid, nn, {et: [1, 1, 1] for et in eid}, 'paper', [0, 1])
