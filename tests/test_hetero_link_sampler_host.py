"""Heterogeneous link-level sampling without a GPU: the C entry point is declared, exported, typed
and rejects bad arguments before any launch; ``HeteroNeighborSampler.sample_from_edges`` and
``HeteroLinkNeighborLoader`` refuse bad input before any device work; the restatement
(``tests/_hetero_link_ref.py``) gives known answers and, where ``torch_geometric`` imports, the
seeds, ``batch % P`` and metadata of the reference's own ``edge_sample``."""
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from tests._hetero_link_ref import hetero_link_sample, hetero_sample_multi, link_seed_block
from tests._hetero_ref import hetero_sample, sampled_info_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = 'pygamd_hetero_link_seeds'
RATES = ('user', 'rates', 'item')
REV = ('item', 'rev', 'user')
FOLLOWS = ('user', 'follows', 'user')


def _lib_or_skip():
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    return _lib.load()


def _graph():
    """4 users, 3 items; 'rates' user -> item, 'rev' item -> user, 'follows' user -> user."""
    eid = {RATES: torch.tensor([[0, 1, 1, 2, 3], [0, 0, 1, 2, 2]]),
           REV: torch.tensor([[0, 0, 1, 2], [0, 1, 1, 3]]),
           FOLLOWS: torch.tensor([[1, 2, 3, 0], [0, 0, 1, 3]])}
    return eid, {'user': 4, 'item': 3}


# ---- the C entry point -----------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_typed():
    from pytorch_geometric_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'pyg_amd.h')).read()
    assert re.search(r'PYGAMD_API\s+int\s+' + SYM + r'\s*\(', text)
    assert SYM in _lib.SIGNATURES and len(_lib.SIGNATURES[SYM][1]) == 16
    _lib_or_skip()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True,
                         text=True).stdout
    assert re.search(r' T ' + SYM + r'\b', out)


def test_entry_point_validates_without_gpu():
    import ctypes
    lib = _lib_or_skip()
    fake = 64  # never dereferenced: every call below is rejected before a launch (or has n = 0)

    def table(*rows):
        return (ctypes.c_int64 * 6)(*[v for r in rows for v in r])

    ok = table((10, 0, 0), (20, 10, 0))
    args = dict(src=fake, dst=fake, dtype=1, P=4, num_neg=4, mode=1, link_time=None, table=ok,
                src_cdf=None, dst_cdf=None, src_time=None, dst_time=None, seed=1, out=fake,
                time_out=None, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return getattr(lib, SYM)(a['src'], a['dst'], a['dtype'], a['P'], a['num_neg'], a['mode'],
                                 a['link_time'], a['table'], a['src_cdf'], a['dst_cdf'],
                                 a['src_time'], a['dst_time'], a['seed'], a['out'],
                                 a['time_out'], a['stream'])

    bad = 1                                                   # PYGAMD_ERR_INVALID_ARG
    assert call(mode=3) == bad and call(mode=-1) == bad
    assert call(P=-1) == bad and call(num_neg=-1) == bad
    assert call(mode=0) == bad                                # negatives without a mode
    assert call(table=None) == bad
    assert call(dtype=2) == bad and call(dtype=7, P=0, num_neg=0) == bad
    assert call(table=table((-1, 0, 0), (20, 10, 0))) == bad
    assert call(table=table((10, -1, 0), (20, 10, 0))) == bad
    big = table((10, 0, 0), (2 ** 31 - 10, 10, 0))
    assert call(dtype=0, table=big) == bad                    # int32 ids cannot hold the type
    assert call(dtype=1, table=big, P=0, num_neg=0) == 0
    for name in ('src', 'dst', 'out'):
        assert call(**{name: None}) == bad, name
    # node times need the link times, and a fallback inside their type
    assert call(dst_time=fake) == bad and call(src_time=fake) == bad
    t = dict(link_time=fake, time_out=fake)
    assert call(**dict(t, time_out=None)) == bad              # link times without their output
    assert call(**dict(t, dst_time=fake, table=table((10, 0, 0), (20, 10, 20)))) == bad
    assert call(**dict(t, dst_time=fake, table=table((10, 0, 0), (20, 10, -1)))) == bad
    assert call(**dict(t, src_time=fake, table=table((10, 0, 10), (20, 10, 0)))) == bad
    # draws from a type without nodes: binary for either endpoint, triplet for the destination
    assert call(table=table((0, 0, 0), (20, 0, 0))) == bad
    assert call(mode=2, table=table((10, 0, 0), (0, 10, 0))) == bad
    assert call(P=0) == bad                                   # negatives without positives
    # nothing to do
    assert call(P=0, num_neg=0) == 0
    assert call(P=0, num_neg=0, mode=0, src=None, dst=None, out=None) == 0


def test_native_wrapper_refuses_before_any_device_work():
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd._lib import PygAmdError
    src, dst = torch.tensor([0, 1]), torch.tensor([2, 0])
    ends = [dict(num_nodes=4, node_base=0), dict(num_nodes=3, node_base=4)]
    f = _native.hetero_link_seeds
    with pytest.raises(ValueError, match="None, 'binary' or 'triplet'"):
        f(src, dst, 2, 'ternary', 0, ends)
    with pytest.raises(ValueError, match='one length and one dtype'):
        f(src, dst[:1], 0, None, 0, ends)
    with pytest.raises(ValueError, match='one length and one dtype'):
        f(src, dst.int(), 0, None, 0, ends)
    with pytest.raises(ValueError, match='int32 or int64'):
        f(src.float(), dst.float(), 0, None, 0, ends)
    with pytest.raises(ValueError, match="'num_neg' must be non-negative"):
        f(src, dst, 2, None, 0, ends)
    with pytest.raises(ValueError, match="'num_neg' must be non-negative"):
        f(src, dst, -1, 'binary', 0, ends)
    with pytest.raises(ValueError, match='source and the destination'):
        f(src, dst, 0, None, 0, ends[:1])
    with pytest.raises(ValueError, match="'link_time' must be"):
        f(src, dst, 0, None, 0, ends, link_time=torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError, match="'link_time' must be"):
        f(src, dst, 0, None, 0, ends, link_time=torch.zeros(2))
    with pytest.raises(ValueError, match='at least one node'):
        f(src, dst, 2, 'triplet', 0, [ends[0], dict(num_nodes=0, node_base=4)])
    with pytest.raises(ValueError, match='do not fit'):
        f(src.int(), dst.int(), 0, None, 0, [ends[0], dict(num_nodes=3, node_base=2 ** 31 - 2)])
    with pytest.raises(ValueError, match="'cdf' must be"):
        f(src, dst, 2, 'binary', 0, [dict(ends[0], cdf=torch.ones(4)), ends[1]])
    nt = torch.zeros(3, dtype=torch.long)
    with pytest.raises(ValueError, match="'link_time', which is missing"):
        f(src, dst, 2, 'binary', 0, [ends[0], dict(ends[1], node_time=nt)])
    lt = torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="'node_time' must be contiguous int64 with 3"):
        f(src, dst, 2, 'binary', 0, [ends[0], dict(ends[1], node_time=nt[:2])], link_time=lt)
    with pytest.raises(ValueError, match="'fallback' must be a node id"):
        f(src, dst, 2, 'binary', 0, [ends[0], dict(ends[1], node_time=nt, fallback=3)],
          link_time=lt)
    with pytest.raises(PygAmdError):                          # host tensors: no CPU fallback
        f(src, dst, 2, 'binary', 0, ends)
    with pytest.raises(PygAmdError):
        _native.unique_inverse(torch.tensor([3, 1, 3]), count_on_device=True)


# ---- the sampler's refusals ------------------------------------------------------------------------
def _host_sampler(temporal=False):
    """A sampler made with ``__new__``, carrying only the host-side facts the checks read: any
    step past them would need the device members and fail with an AttributeError."""
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler
    smp = HeteroNeighborSampler.__new__(HeteroNeighborSampler)
    eid, nn = _graph()
    smp.node_types, smp.num_nodes = list(nn), dict(nn)
    smp.edge_types = list(eid)
    smp._type_index = {t: i for i, t in enumerate(nn)}
    smp.is_temporal = temporal
    return smp


def test_sampler_needs_the_edge_type():
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler
    smp = HeteroNeighborSampler.__new__(HeteroNeighborSampler)   # no attribute may be touched
    with pytest.raises(NotImplementedError, match='link-level.*needs the edge type of the seed '
                                                  'links'):
        smp.sample_from_edges(torch.zeros(2, 1, dtype=torch.long))
    inp = SimpleNamespace(row=torch.tensor([0]), col=torch.tensor([0]), input_type=None)
    with pytest.raises(NotImplementedError, match='link-level.*needs the edge type of the seed '
                                                  'links'):
        smp.sample_from_edges(inp)


def test_sampler_refuses_before_any_device_work():
    smp = _host_sampler()
    pos = torch.tensor([[0, 1], [2, 0]])
    with pytest.raises(ValueError, match=r"must be \(edge_type, \[2, B\] tensor\)"):
        smp.sample_from_edges((RATES, pos, 3))
    with pytest.raises(ValueError, match=r'must be a \[2, B\] tensor'):
        smp.sample_from_edges((RATES, torch.zeros(3, 2, dtype=torch.long)))
    with pytest.raises(ValueError, match=r'must be a \[2, B\] tensor'):
        smp.sample_from_edges((RATES, None))
    with pytest.raises(ValueError, match='not an edge type of the graph'):
        smp.sample_from_edges((('user', 'buys', 'item'), pos))
    with pytest.raises(ValueError, match='not an edge type of the graph'):
        smp.sample_from_edges(('user__rates__user', pos))
    with pytest.raises(ValueError, match='is not an edge type'):
        smp.sample_from_edges((('user', ), pos))
    inp = SimpleNamespace(row=pos[0], col=pos[1][:1], input_type=RATES)
    with pytest.raises(ValueError, match='1-D tensors of one length'):
        smp.sample_from_edges(inp)
    with pytest.raises(ValueError, match='at least one positive edge'):
        smp.sample_from_edges((RATES, pos[:, :0]))
    inp = SimpleNamespace(row=pos[0], col=pos[1], input_type=RATES, time=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match='is given but the sampler is not temporal'):
        smp.sample_from_edges(inp)
    with pytest.raises(ValueError, match="needs the seed-link times"):
        _host_sampler(temporal=True).sample_from_edges((RATES, pos))
    # the weights are per endpoint type: 4 users, 3 items
    with pytest.raises(ValueError, match="number of nodes 4 of node type 'user' \\(got 3\\)"):
        smp.sample_from_edges((RATES, pos), dict(mode='binary', src_weight=torch.ones(3)))
    with pytest.raises(ValueError, match="number of nodes 3 of node type 'item' \\(got 4\\)"):
        smp.sample_from_edges((RATES, pos), dict(mode='triplet', dst_weight=torch.ones(4)))
    inp = SimpleNamespace(row=pos[0], col=pos[1], input_type=RATES, label=torch.ones(2))
    with pytest.raises(ValueError, match="undefined for 'triplet'"):
        smp.sample_from_edges(inp, 'triplet')
    inp.label = torch.ones(3)
    with pytest.raises(ValueError, match='one entry per positive edge'):
        smp.sample_from_edges(inp, 'binary')
    with pytest.raises(ValueError, match="'amount' needs to be positive"):
        smp.sample_from_edges((RATES, pos), dict(mode='binary', amount=0))
    # both endpoints against their OWN type: item 3 does not exist, user 3 does
    with pytest.raises(ValueError, match=r"\[0, 3\) for node type 'item'"):
        smp.sample_from_edges((RATES, torch.tensor([[3], [3]])))
    with pytest.raises(ValueError, match=r"\[0, 4\) for node type 'user'"):
        smp.sample_from_edges((RATES, torch.tensor([[4], [0]])))
    with pytest.raises(ValueError, match=r"\[0, 3\) for node type 'item'"):
        smp.sample_from_edges((REV, torch.tensor([[3], [3]])))
    with pytest.raises(ValueError, match='int32 or int64'):
        smp.sample_from_edges((RATES, pos.float()))
    # past every check the host-only object has nothing to run on
    with pytest.raises(AttributeError):
        smp.sample_from_edges((RATES, pos))


def test_homogeneous_sampler_keeps_refusing_an_input_type():
    from pytorch_geometric_amd.sampler import NeighborSampler
    smp = NeighborSampler.__new__(NeighborSampler)
    inp = SimpleNamespace(row=torch.tensor([0]), col=torch.tensor([0]), input_type=RATES)
    with pytest.raises(NotImplementedError):
        smp.sample_from_edges(inp)


def test_loader_validates_before_touching_the_device():
    """Every error below is raised before the sampler is built: the tensors are on the host."""
    from pytorch_geometric_amd.loader import HeteroLinkNeighborLoader as L
    eid, nn = _graph()
    x = {'user': torch.zeros(4, 2), 'item': torch.zeros(3, 2)}
    eli = (RATES, eid[RATES][:, :3])
    with pytest.raises(ValueError, match="conflicting 'edge_label_time' and 'time_attr'"):
        L(x, eid, [2], eli, edge_label_time=torch.arange(3))
    with pytest.raises(ValueError, match="'edge_label_time' is not set while 'time_attr' is set"):
        L(x, eid, [2], eli, node_time={'user': torch.arange(4)})
    with pytest.raises(ValueError, match="'edge_label_time' is not set while 'time_attr' is set"):
        L(x, eid, [2], eli, edge_time={RATES: torch.arange(5)})
    with pytest.raises(ValueError, match="'edge_label' needs to be undefined for 'triplet'"):
        L(x, eid, [2], eli, edge_label=torch.ones(3), neg_sampling='triplet')
    with pytest.raises(ValueError, match='needs to be an integer'):
        L(x, eid, [2], eli, neg_sampling=dict(mode='triplet', amount=0.5))
    with pytest.raises(ValueError, match="'amount' needs to be positive"):
        L(x, eid, [2], eli, neg_sampling_ratio=-1.0)
    with pytest.raises(ValueError, match='needs the edge type of the seed links'):
        L(x, eid, [2], eid[RATES])
    with pytest.raises(ValueError, match='needs the edge type of the seed links'):
        L(x, eid, [2], (eid[RATES], RATES))
    with pytest.raises(ValueError, match='not an edge type of the graph'):
        L(x, eid, [2], (('user', 'buys', 'item'), eid[RATES]))
    with pytest.raises(ValueError, match="'item' of the seed links has no entry in 'x_dict'"):
        L({'user': x['user']}, eid, [2], eli)
    with pytest.raises(ValueError, match=r"\[2, L\]"):
        L(x, eid, [2], (RATES, torch.zeros(3, 4, dtype=torch.long)))
    with pytest.raises(ValueError, match='one entry per link'):
        L(x, eid, [2], eli, edge_label=torch.ones(4))
    with pytest.raises(ValueError, match="number of nodes 3 of node type 'item' \\(got 4\\)"):
        L(x, eid, [2], eli, neg_sampling=dict(mode='binary', dst_weight=torch.ones(4)))
    with pytest.raises(ValueError, match="number of nodes 4 of node type 'user' \\(got 3\\)"):
        L(x, eid, [2], (RATES, None), neg_sampling=dict(mode='binary', src_weight=torch.ones(3)))


# ---- the restatement ----------------------------------------------------------------------------------
def test_multi_seed_restatement_with_one_type_is_the_single_type_one():
    eid, nn = sampled_info_graph()
    fan = {et: [1, 2, 4] for et in eid}
    for disjoint in (False, True):
        assert hetero_sample_multi(eid, nn, fan, {'paper': [0, 1]}, disjoint=disjoint) == \
            hetero_sample(eid, nn, fan, 'paper', [0, 1], disjoint=disjoint)
    with pytest.raises(ValueError, match='random'):
        hetero_sample_multi(eid, nn, {et: [1] for et in eid}, {'paper': [2], 'author': [7]})


def test_restatement_known_answer_two_types():
    eid, nn = _graph()
    fan = {et: [-1] for et in eid}
    # links u1 -> i0 and u2 -> i2 twice: not disjoint, each endpoint made unique on its own
    (node, row, col, edge, batch, n_nodes, n_edges), blk = hetero_link_sample(
        eid, nn, fan, RATES, [2, 1, 2], [2, 0, 2])
    assert blk['seed_dict'] == {'user': [1, 2], 'item': [0, 2]}
    assert blk['index'] == [[1, 0, 1], [1, 0, 1]] and blk['label'] is None
    # rates into i0: u0, u1, into i2: u2, u3; rev into u1: i0, i1; follows into u1: u3
    assert node == {'user': [1, 2, 0, 3], 'item': [0, 2, 1]}
    assert edge == {RATES: [0, 1, 3, 4], REV: [1, 2], FOLLOWS: [2]}
    assert row[RATES] == [2, 0, 1, 3] and col[RATES] == [0, 0, 1, 1]
    assert row[REV] == [0, 2] and col[REV] == [0, 0]
    assert n_nodes == {'user': [2, 2], 'item': [2, 1]} and batch is None
    # disjoint, binary negatives: trees run through the sources, then the destinations
    (node, _, _, _, batch, n_nodes, _), blk = hetero_link_sample(
        eid, nn, fan, RATES, [2, 1], [2, 0], disjoint=True, mode='binary', amount=0.5,
        src_neg=[3], dst_neg=[1], time=[7, 9])
    assert blk['seed_dict'] == {'user': [2, 1, 3], 'item': [2, 0, 1]}
    assert blk['seed_time'] == [7, 9, 7, 7, 9, 7] and blk['src_time'] == [7, 9, 7]
    assert blk['index'] == [[0, 1, 2], [0, 1, 2]] and blk['label'] == [1.0, 1.0, 0]
    assert node['user'][:3] == [2, 1, 3] and node['item'][:3] == [2, 0, 1]
    # tree ids 0, 1, 2 (sources) and 3, 4, 5 (destinations), folded by % P = 2
    assert batch['user'][:3] == [0, 1, 0] and batch['item'][:3] == [1, 0, 1]
    assert n_nodes['user'][0] == 3 and n_nodes['item'][0] == 3


def test_restatement_known_answer_one_type_and_triplet():
    blk = link_seed_block(FOLLOWS, [1, 2], [0, 0], mode='triplet', amount=2,
                          dst_neg=[3, 1, 2, 3])
    assert blk['seed_dict'] == {'user': [0, 1, 2, 3]}
    assert blk['index'] == ([1, 2], [0, 0], [[3, 1], [2, 3]])
    blk = link_seed_block(FOLLOWS, [1, 2], [0, 0], mode='triplet', amount=2,
                          dst_neg=[3, 1, 2, 3], disjoint=True, time=[4, 5])
    assert blk['seed_dict'] == {'user': [1, 2, 0, 0, 3, 1, 2, 3]}
    assert blk['index'] == ([0, 1], [2, 3], [[4, 6], [5, 7]])
    assert blk['src_time'] == [4, 5] and blk['seed_time'] == [4, 5] + [4, 5] * 3
    blk = link_seed_block(RATES, [1, 2], [0, 0], mode='triplet', amount=1, dst_neg=[2, 1],
                          disjoint=True)
    assert blk['seed_dict'] == {'user': [1, 2], 'item': [0, 0, 2, 1]}
    assert blk['index'] == ([0, 1], [0, 1], [2, 3])
    blk = link_seed_block(RATES, [1, 2], [0, 0], mode='triplet', amount=2, dst_neg=[2, 1, 1, 0])
    assert blk['seed_dict'] == {'user': [1, 2], 'item': [0, 1, 2]}
    assert blk['index'] == ([0, 1], [0, 0], [[2, 1], [1, 0]])


@pytest.mark.parametrize('disjoint', [False, True])
@pytest.mark.parametrize('input_type', [RATES, REV, FOLLOWS])
def test_restatement_equals_the_reference_edge_sample(input_type, disjoint):
    """The reference's own ``edge_sample`` (no negatives) driven with the restatement's multi-seed
    sampler as ``sample_fn``: the seed dict it hands over, ``batch % P`` and the metadata are the
    restatement's.  This pins the layout to the real reference without ``pyg-lib``."""
    try:
        from oracle import make_ref
        make_ref.import_reference()
        from torch_geometric.sampler import EdgeSamplerInput, HeteroSamplerOutput
        from torch_geometric.sampler.neighbor_sampler import edge_sample
    except ImportError:
        pytest.skip('torch_geometric cannot be imported')
    eid, nn = _graph()
    fan = {et: [-1, -1] for et in eid}
    src, dst = eid[input_type][0], eid[input_type][1]
    src, dst = torch.cat([src, src[:2]]), torch.cat([dst, dst[:2]])      # repeated links
    P = src.numel()
    label = torch.arange(P) % 3
    time = torch.arange(P) + 10 if disjoint else None
    seen = {}

    def sample_fn(seed_dict, seed_time_dict):
        seen['seeds'] = {t: v.tolist() for t, v in seed_dict.items()}
        seen['time'] = None if seed_time_dict is None else \
            [t for v in seed_time_dict.values() for t in v.tolist()]
        node, row, col, edge, batch, n_nodes, n_edges = hetero_sample_multi(
            eid, nn, fan, seen['seeds'], disjoint=disjoint)
        ten = torch.tensor
        return HeteroSamplerOutput(
            node={t: ten(v) for t, v in node.items()}, row={k: ten(v) for k, v in row.items()},
            col={k: ten(v) for k, v in col.items()}, edge={k: ten(v) for k, v in edge.items()},
            batch=None if batch is None else {t: ten(v) for t, v in batch.items()},
            num_sampled_nodes=n_nodes, num_sampled_edges=n_edges)

    inp = EdgeSamplerInput(torch.arange(P), src, dst, label=label, time=time,
                           input_type=input_type)
    ref = edge_sample(inp, sample_fn, nn, disjoint)
    want, blk = hetero_link_sample(eid, nn, fan, input_type, src.tolist(), dst.tolist(),
                                   disjoint=disjoint, label=label.tolist(),
                                   time=None if time is None else time.tolist())
    assert seen['seeds'] == blk['seed_dict'] and list(seen['seeds']) == list(blk['seed_dict'])
    assert seen['time'] == blk['seed_time']
    assert {t: v.tolist() for t, v in ref.node.items()} == want[0]
    if disjoint:
        assert {t: v.tolist() for t, v in ref.batch.items()} == want[4]
    input_id, eli, lab, src_time = ref.metadata
    assert input_id.tolist() == list(range(P))
    assert eli.tolist() == blk['index']
    assert lab.tolist() == blk['label']
    assert (None if src_time is None else src_time.tolist()) == blk['src_time']
