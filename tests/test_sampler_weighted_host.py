"""Weighted neighbour sampling without a GPU: the C entry point is declared, exported and in the
ctypes table, rejects bad arguments before any launch, and the reference-facing adapter
(``backend.neighbor_sampler(..., weight_attr=...)``) hands ``data[weight_attr]`` to the sampler."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = 'pygamd_sample_neighbors_weighted'


def _lib_or_skip():
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    return _lib.load()


def test_weighted_entry_point_is_declared_exported_and_typed():
    from pytorch_geometric_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'pyg_amd.h')).read()
    assert re.search(r'PYGAMD_API\s+int\s+' + SYM + r'\s*\(', text)
    assert SYM in _lib.SIGNATURES
    restype, args = _lib.SIGNATURES[SYM]
    assert len(args) == 15
    _lib_or_skip()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True,
                         text=True).stdout
    assert re.search(r' T ' + SYM + r'\b', out)


def test_weighted_entry_point_validates_without_gpu():
    lib = _lib_or_skip()
    fake = 64  # never dereferenced: every call below is rejected before a launch
    args = dict(colptr=fake, row=fake, idx_dtype=1, weight=fake, frontier=fake, n=1,
                offsets=fake, k=5, seed=0, flags=0, seed_dev=None, src=fake, dst=fake,
                slot=fake, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return getattr(lib, SYM)(a['colptr'], a['row'], a['idx_dtype'], a['weight'],
                                 a['frontier'], a['n'], a['offsets'], a['k'], a['seed'],
                                 a['flags'], a['seed_dev'], a['src'], a['dst'], a['slot'],
                                 a['stream'])

    assert lib.pygamd_status_string(1) and lib.pygamd_status_string(2)
    assert call(weight=None) == 1                         # PYGAMD_ERR_INVALID_ARG
    assert call(weight=None, n=0) == 1
    assert call(k=65) == 2                                # PYGAMD_ERR_UNSUPPORTED
    assert call(k=65, n=0) == 2
    assert call(n=-1) == 1
    assert call(row=None) == 1
    assert call(flags=1, k=0) == 1                        # replacement needs a bounded fan-out
    assert call(idx_dtype=7) == 1
    assert call(n=0) == 0                                 # nothing to do


class _StubSampler:
    calls = []

    def __init__(self, edge_index, num_nodes, num_neighbors, **kw):
        _StubSampler.calls.append(kw)
        self.replace, self.disjoint = kw.get('replace', False), kw.get('disjoint', False)
        self.subgraph_type = kw.get('subgraph_type', 'directional')
        self.edge_weight = kw.get('edge_weight')


def test_backend_passes_weight_attr_through(monkeypatch):
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
    ei = torch.Tensor._make_subclass(OnDevice, torch.tensor([[1, 3, 0, 4], [2, 2, 1, 3]]))
    w = torch.tensor([0.0, 1.0, 0.0, 1.0])
    data = Data(edge_index=ei, num_nodes=5, edge_weight=w)
    smp = backend.neighbor_sampler(data, [1, 1], weight_attr='edge_weight')
    assert _StubSampler.calls[-1]['edge_weight'] is data['edge_weight']
    assert smp.weight_attr == 'edge_weight' and smp.edge_weight is w
    backend.neighbor_sampler(data, [1, 1])
    assert _StubSampler.calls[-1]['edge_weight'] is None
    with pytest.raises(ValueError):
        backend.neighbor_sampler((ei, 5), [1, 1], weight_attr='edge_weight')
    with pytest.raises(KeyError):
        backend.neighbor_sampler(data, [1, 1], weight_attr='no_such_attr')
    monkeypatch.setattr(backend, '_sampler_cls', None)  # do not leak the stubbed class
