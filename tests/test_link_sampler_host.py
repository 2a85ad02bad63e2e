"""Link-level sampling without a GPU: the two C entry points are declared, exported and in the
ctypes table and reject bad arguments before any launch; ``NegativeSampling`` and
``LinkNeighborLoader`` give the reference's validation errors before touching the device."""
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = 'pygamd_sample_negatives'
UNIQ = 'pygamd_unique_inverse'


def _lib_or_skip():
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    return _lib.load()


@pytest.mark.parametrize('sym,n_args', [(NEG, 12), (UNIQ, 11)])
def test_link_entry_points_are_declared_exported_and_typed(sym, n_args):
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


def test_negatives_entry_point_validates_without_gpu():
    lib = _lib_or_skip()
    fake = 64  # never dereferenced: every call below is rejected before a launch
    args = dict(n=4, N=10, seed=1, seed_dev=None, cdf=None, node_time=None, bound=None,
                n_bound=0, fallback=0, dtype=1, out=fake, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return getattr(lib, NEG)(a['n'], a['N'], a['seed'], a['seed_dev'], a['cdf'],
                                 a['node_time'], a['bound'], a['n_bound'], a['fallback'],
                                 a['dtype'], a['out'], a['stream'])

    assert call(n=-1) == 1                                # PYGAMD_ERR_INVALID_ARG
    assert call(dtype=2) == 1 and call(dtype=-1, n=0) == 1
    assert call(dtype=0, N=2 ** 31) == 1                  # int32 ids cannot hold the nodes
    assert call(N=0) == 1 and call(N=-3) == 1
    assert call(out=None) == 1
    assert call(bound=fake, n_bound=4) == 1               # a bound without node times
    t = dict(node_time=fake, bound=fake, n_bound=4, fallback=0)
    assert call(**dict(t, bound=None)) == 1
    assert call(**dict(t, n_bound=0)) == 1
    assert call(**dict(t, fallback=10)) == 1 and call(**dict(t, fallback=-1)) == 1
    assert call(**dict(t, fallback=10, n=0)) == 1
    assert call(n=0) == 0                                 # nothing to do
    assert call(n=0, N=0, out=None) == 0


def test_unique_entry_point_validates_without_gpu():
    lib = _lib_or_skip()
    fake = 64
    args = dict(keys=fake, perm=fake, dtype=1, n=5, rank=fake, ws=fake, ws_bytes=1 << 20,
                uniq=fake, inv=fake, nu=fake, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return getattr(lib, UNIQ)(a['keys'], a['perm'], a['dtype'], a['n'], a['rank'], a['ws'],
                                  a['ws_bytes'], a['uniq'], a['inv'], a['nu'], a['stream'])

    assert call(n=-1) == 1
    assert call(dtype=7) == 1 and call(dtype=7, n=0) == 1
    for name in ('keys', 'perm', 'rank', 'ws', 'uniq', 'inv', 'nu'):
        assert call(**{name: None}) == 1, name
    assert call(ws_bytes=0) == 3                          # PYGAMD_ERR_WORKSPACE
    assert call(n=0) == 0 and call(n=0, keys=None) == 0


def test_native_wrappers_refuse_host_tensors():
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd._lib import PygAmdError
    with pytest.raises(PygAmdError):
        _native.unique_inverse(torch.tensor([3, 1, 3]))
    with pytest.raises(PygAmdError):
        _native.sample_negatives(4, 10, 0, torch.device('cpu'))
    with pytest.raises(ValueError, match='int32 or int64'):
        _native.sample_negatives(4, 10, 0, torch.device('cpu'), dtype=torch.float32)
    with pytest.raises(ValueError, match='non-negative'):
        _native.sample_negatives(-1, 10, 0, torch.device('cpu'))
    with pytest.raises(ValueError, match='at least one node'):
        _native.sample_negatives(3, 0, 0, torch.device('cpu'))
    with pytest.raises(ValueError, match='go together'):
        _native.sample_negatives(3, 5, 0, torch.device('cpu'), node_time=torch.zeros(5).long())


def test_negative_sampling_validation_and_cast():
    from pytorch_geometric_amd.sampler import NegativeSampling
    with pytest.raises(ValueError, match="'amount' needs to be positive"):
        NegativeSampling('binary', 0)
    with pytest.raises(ValueError, match="'amount' needs to be positive"):
        NegativeSampling('triplet', -1)
    with pytest.raises(ValueError, match="needs to be an integer"):
        NegativeSampling('triplet', 1.5)
    with pytest.raises(ValueError, match='not a valid NegativeSamplingMode'):
        NegativeSampling('ternary')
    ns = NegativeSampling('triplet', 2.0)
    assert ns.is_triplet() and ns.amount == 2 and isinstance(ns.amount, int)
    assert NegativeSampling('binary', 0.5).amount == 0.5
    assert NegativeSampling.cast(None) is None
    assert NegativeSampling.cast(ns) is ns
    assert NegativeSampling.cast('binary').is_binary()
    d = NegativeSampling.cast(dict(mode='triplet', amount=3))
    assert d.is_triplet() and d.amount == 3
    w = torch.ones(7)
    ref_like = SimpleNamespace(mode=SimpleNamespace(value='binary'), amount=2.5, src_weight=w,
                               dst_weight=None)  # the reference's object: an enum mode
    c = NegativeSampling.cast(ref_like)
    assert c.is_binary() and c.amount == 2.5 and c.src_weight is w and c.dst_weight is None
    c.check(7)
    with pytest.raises(ValueError, match='needs to match the number of nodes 8'):
        c.check(8)
    with pytest.raises(ValueError):
        NegativeSampling.cast(3.0)


def test_link_loader_validates_before_touching_the_device():
    """Every error below is raised before the sampler is built: the tensors are on the host, and
    no GPU is needed."""
    from pytorch_geometric_amd.loader import LinkNeighborLoader
    x = torch.zeros(10, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(ValueError, match="conflicting 'edge_label_time' and 'time_attr'"):
        LinkNeighborLoader(x, ei, [2], edge_label_time=torch.arange(3))
    with pytest.raises(ValueError, match="'edge_label_time' is not set while 'time_attr' is set"):
        LinkNeighborLoader(x, ei, [2], node_time=torch.arange(10))
    with pytest.raises(ValueError, match="'edge_label' needs to be undefined for 'triplet'"):
        LinkNeighborLoader(x, ei, [2], edge_label=torch.ones(3), neg_sampling='triplet')
    with pytest.raises(ValueError, match="needs to be an integer"):
        LinkNeighborLoader(x, ei, [2], neg_sampling=dict(mode='triplet', amount=0.5))
    with pytest.raises(ValueError, match="'amount' needs to be positive"):
        LinkNeighborLoader(x, ei, [2], neg_sampling_ratio=-1.0)
    with pytest.raises(ValueError, match='needs to match the number of nodes 10'):
        LinkNeighborLoader(x, ei, [2], neg_sampling=dict(mode='binary', dst_weight=torch.ones(9)))
    with pytest.raises(ValueError, match=r"\[2, L\]"):
        LinkNeighborLoader(x, ei, [2], edge_label_index=torch.zeros(3, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="one entry per link"):
        LinkNeighborLoader(x, ei, [2], edge_label=torch.ones(4))
