"""Temporal neighbour sampling without a GPU: the two C entry points are declared, exported and in
the ctypes table and reject bad arguments before any launch; the constructor, the loader and the
reference-facing adapter (``backend.neighbor_sampler(..., time_attr=...)``) validate their time
arguments before touching the device."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = 'pygamd_sample_temporal_window'
DRAW = 'pygamd_sample_neighbors_temporal'


def _lib_or_skip():
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    return _lib.load()


@pytest.mark.parametrize('sym,n_args', [(WINDOW, 16), (DRAW, 15)])
def test_temporal_entry_points_are_declared_exported_and_typed(sym, n_args):
    from pytorch_geometric_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'pyg_amd.h')).read()
    assert re.search(r'PYGAMD_API\s+int\s+' + sym + r'\s*\(', text)
    assert sym in _lib.SIGNATURES
    _, args = _lib.SIGNATURES[sym]
    assert len(args) == n_args
    _lib_or_skip()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True,
                         text=True).stdout
    assert re.search(r' T ' + sym + r'\b', out)


def test_window_entry_point_validates_without_gpu():
    lib = _lib_or_skip()
    fake = 64  # never dereferenced: every call below is rejected before a launch
    args = dict(colptr=fake, row=fake, idx_dtype=1, time=fake, level=0, frontier=fake,
                ftime=fake, n=1, k=5, replace=0, strategy=0, n_valid=None, lo=fake, hi=fake,
                cnt=fake, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return getattr(lib, WINDOW)(a['colptr'], a['row'], a['idx_dtype'], a['time'], a['level'],
                                    a['frontier'], a['ftime'], a['n'], a['k'], a['replace'],
                                    a['strategy'], a['n_valid'], a['lo'], a['hi'], a['cnt'],
                                    a['stream'])

    assert call(time=None) == 1                           # PYGAMD_ERR_INVALID_ARG
    assert call(time=None, n=0) == 1
    assert call(ftime=None) == 1
    assert call(level=2) == 1 and call(level=-1, n=0) == 1
    assert call(strategy=2) == 1 and call(strategy=-1, n=0) == 1
    assert call(k=65) == 2                                # PYGAMD_ERR_UNSUPPORTED
    assert call(k=65, n=0) == 2
    assert call(replace=1, k=-1) == 1                     # replacement needs a bounded fan-out
    assert call(n=-1) == 1
    for name in ('colptr', 'row', 'frontier', 'lo', 'hi', 'cnt'):
        assert call(**{name: None}) == 1, name
    assert call(idx_dtype=7) == 1
    assert call(n=0) == 0                                 # nothing to do
    assert call(n=0, level=1, strategy=1, replace=1, k=3) == 0


def test_draw_entry_point_validates_without_gpu():
    lib = _lib_or_skip()
    fake = 64
    args = dict(row=fake, idx_dtype=1, frontier=fake, n=1, lo=fake, hi=fake, offsets=fake, k=5,
                seed=0, flags=0, seed_dev=None, src=fake, dst=fake, slot=fake, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return getattr(lib, DRAW)(a['row'], a['idx_dtype'], a['frontier'], a['n'], a['lo'],
                                  a['hi'], a['offsets'], a['k'], a['seed'], a['flags'],
                                  a['seed_dev'], a['src'], a['dst'], a['slot'], a['stream'])

    assert call(lo=None) == 1 and call(hi=None, n=0) == 1
    assert call(k=65) == 2 and call(k=65, n=0) == 2
    assert call(flags=1, k=0) == 1
    assert call(n=-1) == 1
    for name in ('row', 'frontier', 'offsets', 'src', 'dst', 'slot'):
        assert call(**{name: None}) == 1, name
    assert call(idx_dtype=7) == 1
    assert call(n=0) == 0


# ---- constructor / loader validation: every case below raises before any device work -----------
def _ei():
    return torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]])


@pytest.mark.parametrize('kw,match', [
    (dict(node_time=torch.zeros(5)), 'integer'),
    (dict(edge_time=torch.zeros(4, dtype=torch.float64)), 'integer'),
    (dict(node_time=torch.zeros(4, dtype=torch.long)), '5 entries'),
    (dict(edge_time=torch.zeros(5, dtype=torch.long)), '4 entries'),
    (dict(node_time=torch.zeros(5, dtype=torch.long), edge_time=torch.zeros(4, dtype=torch.long)),
     'not both'),
    (dict(node_time=torch.zeros(5, dtype=torch.long), temporal_strategy='recent'),
     'temporal_strategy'),
    (dict(node_time=torch.zeros(5, dtype=torch.long), subgraph_type='induced'), 'induced'),
    (dict(node_time=torch.zeros(5, dtype=torch.long), edge_weight=torch.ones(4)), 'weighted'),
])
def test_constructor_refuses_bad_time_arguments(kw, match):
    from pytorch_geometric_amd.sampler import NeighborSampler
    with pytest.raises(ValueError, match=match):
        NeighborSampler(_ei(), 5, [2, 2], **kw)


def test_loader_refuses_input_time_without_a_time_attribute():
    from pytorch_geometric_amd.loader import NeighborLoader
    with pytest.raises(ValueError, match="'input_time' is set while 'time_attr' is not set"):
        NeighborLoader(torch.zeros(5, 3), _ei(), [2], input_time=torch.zeros(5, dtype=torch.long))


class _StubTemporal:
    """Stands in for the sampler's constructor (no device): ``seed_time`` and ``sample_padded``
    run the real code paths on an object with the attributes they read."""
    def __init__(self, edge_level):
        from pytorch_geometric_amd.sampler import NeighborSampler
        self.is_temporal, self.edge_level = True, edge_level
        self.time = torch.arange(5)
        self.row = torch.zeros(4, dtype=torch.long)
        self.num_neighbors = [2]
        self.seed_time = NeighborSampler.seed_time.__get__(self)
        self.sample_padded = NeighborSampler.sample_padded.__get__(self)


def test_edge_level_time_needs_seed_times_and_padded_is_refused():
    s = _StubTemporal(edge_level=True)
    with pytest.raises(ValueError, match='needs the seed times'):
        s.seed_time(torch.tensor([1, 2]))
    with pytest.raises(ValueError, match='integer'):
        s.seed_time(torch.tensor([1, 2]), torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match='one entry per seed'):
        s.seed_time(torch.tensor([1, 2]), torch.tensor([1]))
    assert s.seed_time(torch.tensor([1, 2]), torch.tensor([7, 8], dtype=torch.int32)).tolist() \
        == [7, 8]
    n = _StubTemporal(edge_level=False)
    assert n.seed_time(torch.tensor([3, 1])).tolist() == [3, 1]
    with pytest.raises(ValueError, match='temporal'):
        n.sample_padded(torch.tensor([1]))


# ---- the reference-facing adapter ------------------------------------------------------------
class _StubSampler:
    calls = []

    def __init__(self, edge_index, num_nodes, num_neighbors, **kw):
        _StubSampler.calls.append(kw)
        self.replace, self.disjoint = kw.get('replace', False), kw.get('disjoint', False)
        self.subgraph_type = kw.get('subgraph_type', 'directional')
        self.edge_weight = kw.get('edge_weight')


def test_backend_detects_node_and_edge_time_attrs(monkeypatch):
    from oracle import make_ref
    try:
        make_ref.import_reference()
        from torch_geometric.data import Data
    except ImportError:
        pytest.skip('no reference available')
    from pytorch_geometric_amd import backend, sampler

    class OnDevice(torch.Tensor):  # a CPU tensor that passes the adapter's device check
        @property
        def is_cuda(self):
            return True

    monkeypatch.setattr(sampler, 'NeighborSampler', _StubSampler)
    monkeypatch.setattr(backend, '_sampler_cls', None)
    _StubSampler.calls.clear()
    ei = torch.Tensor._make_subclass(OnDevice, torch.tensor([[1, 3, 0], [2, 2, 1]]))
    nt = torch.tensor([5, 4, 3, 2, 1])
    et = torch.tensor([10, 20, 30])
    data = Data(edge_index=ei, num_nodes=5, t=nt, et=et)
    smp = backend.neighbor_sampler(data, [1, 1], time_attr='t', temporal_strategy='last')
    kw = _StubSampler.calls[-1]
    assert kw['node_time'] is data['t'] and kw['edge_time'] is None
    assert kw['temporal_strategy'] == 'last'
    assert smp.is_temporal and smp.time_attr == 't' and smp.temporal_strategy == 'last'
    smp = backend.neighbor_sampler(data, [1, 1], time_attr='et')
    kw = _StubSampler.calls[-1]
    assert kw['edge_time'] is data['et'] and kw['node_time'] is None
    assert kw['temporal_strategy'] == 'uniform' and smp.is_temporal
    smp = backend.neighbor_sampler(data, [1, 1])
    kw = _StubSampler.calls[-1]
    assert kw['node_time'] is None and kw['edge_time'] is None and not smp.is_temporal
    with pytest.raises(ValueError, match="neither a node-level or edge-level attribute"):
        backend.neighbor_sampler(Data(edge_index=ei, num_nodes=5, odd=torch.zeros(7)), [1],
                                 time_attr='odd')
    with pytest.raises(ValueError):
        backend.neighbor_sampler((ei, 5), [1, 1], time_attr='t')
    monkeypatch.setattr(backend, '_sampler_cls', None)  # do not leak the stubbed class
