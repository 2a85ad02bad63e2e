"""Heterogeneous link-level sampling on the GPU: ``HeteroNeighborSampler.sample_from_edges``,
``pygamd_hetero_link_seeds``, ``HeteroLinkNeighborLoader`` and ``backend.neighbor_sampler(
hetero_data)`` under the reference's ``LinkLoader`` (the heterogeneous branch of ``edge_sample``,
sampler/neighbor_sampler.py:852-998; loader/link_loader.py:280-334).  Deterministic draws are pinned
to the plain-Python restatement in ``tests/_hetero_link_ref.py`` (fed with the negatives the batch
contains), order included; one node type and one edge type must give
``NeighborSampler.sample_from_edges`` bit for bit; the seed-block kernel must give
``pygamd_sample_negatives``' draws.  The RNG is counter-based: every statistical check below is
deterministic for its fixed seeds."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests._hetero_link_ref import hetero_link_sample
from tests._util import gen

pytestmark = pytest.mark.gpu

DTYPES = [torch.int64, torch.int32]
RATES = ('user', 'rates', 'item')
REV = ('item', 'rev', 'user')        # source type after destination type in the node-type order
FOLLOWS = ('user', 'follows', 'user')
NN = {'user': 50, 'item': 30}


def _rand_ei(n_src, n_dst, m, seed, dtype=torch.int64):
    g = gen(seed)
    return torch.stack([torch.randint(0, n_src, (m, ), generator=g),
                        torch.randint(0, n_dst, (m, ), generator=g)]).to(dtype)


def _graph(dtype=torch.int64):
    eid = {RATES: _rand_ei(50, 30, 120, 1, dtype), REV: _rand_ei(30, 50, 100, 2, dtype),
           FOLLOWS: _rand_ei(50, 50, 90, 3, dtype)}
    return eid, dict(NN)


def _sampler(eid, nn, fan, dev, **kw):
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler
    kw = {k: ({a: b.to(dev) for a, b in v.items()} if isinstance(v, dict) else v)
          for k, v in kw.items()}
    return HeteroNeighborSampler({k: v.to(dev) for k, v in eid.items()}, nn, fan, **kw)


def _lists(out):
    f = (lambda d: {k: v.long().tolist() for k, v in d.items()})
    return (f(out.node), f(out.row), f(out.col), f(out.edge),
            None if out.batch is None else f(out.batch), out.num_sampled_nodes,
            out.num_sampled_edges)


def _positives(eid, et, B, seed):
    """``B`` links of the edge type, some of them twice (so that ``unique`` has work to do)."""
    ei = eid[et].long()
    pos = ei[:, torch.randperm(ei.size(1), generator=gen(seed))[:B - 3]]
    return torch.cat([pos, pos[:, :3]], 1)


def _assert_hops(out, want, what=''):
    for g, w, name in zip(_lists(out), want, ('node', 'row', 'col', 'edge', 'batch', 'n_nodes',
                                              'n_edges')):
        assert g == w, (what, name)


def _assert_metadata(out, blk, mode, dev):
    md = out.metadata
    for t in md[1:4 if mode == 'triplet' else 2]:
        assert t.dtype == torch.int64 and t.device.type == dev.type
    if mode == 'triplet':
        assert len(md) == 5
        assert md[1].tolist() == blk['index'][0] and md[2].tolist() == blk['index'][1]
        assert md[3].tolist() == blk['index'][2]
    else:
        assert len(md) == 4
        assert md[1].tolist() == blk['index']
        assert (None if md[2] is None else md[2].tolist()) == blk['label']
    assert (None if md[-1] is None else md[-1].tolist()) == blk['src_time']


# ---- 1. full fan-out, no negatives: the restatement exactly ----------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('disjoint', [False, True])
@pytest.mark.parametrize('et', [RATES, REV, FOLLOWS])
def test_full_fanout_equals_restatement(dev, dtype, disjoint, et):
    eid, nn = _graph(dtype)
    fan = {k: [-1, -1] for k in eid}
    smp = _sampler(eid, nn, [-1, -1], dev, disjoint=disjoint, seed=3)
    pos = _positives(eid, et, 12, 5)
    label = torch.arange(12) % 3
    inp = SimpleNamespace(row=pos[0], col=pos[1], label=label, time=None,
                          input_id=torch.arange(12), input_type=et)
    want, blk = hetero_link_sample(eid, nn, fan, et, pos[0].tolist(), pos[1].tolist(),
                                   disjoint=disjoint, label=label.tolist())
    out = smp.sample_from_edges(inp, seed=9)
    assert all(v.dtype == dtype for v in out.node.values())
    assert all(v.dtype == dtype for v in out.row.values())
    _assert_hops(out, want, 'first')
    _assert_metadata(out, blk, None, dev)
    assert torch.equal(out.metadata[0], torch.arange(12))
    # the tuple form; and a second identical call gives the same batch (the id map is clean)
    again = smp.sample_from_edges((et, pos.to(dev)), seed=9)
    _assert_hops(again, want, 'second')
    assert again.metadata[0] is None and again.metadata[2] is None
    assert again.metadata[1].tolist() == blk['index']
    # and so does sample_from_nodes after it
    nodes = smp.sample_from_nodes((et[0], pos[0][:4]), seed=9)
    assert nodes.node[et[0]][:nodes.num_sampled_nodes[et[0]][0]].tolist() == pos[0][:4].tolist()


# ---- 2. with negatives ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('disjoint', [False, True])
@pytest.mark.parametrize('et', [RATES, REV, FOLLOWS])
@pytest.mark.parametrize('mode,amount', [('binary', 1), ('binary', 0.5), ('binary', 2.5),
                                         ('triplet', 1), ('triplet', 3)])
def test_negatives_layout_and_hops(dev, dtype, disjoint, et, mode, amount):
    from pytorch_geometric_amd.sampler import NegativeSampling
    eid, nn = _graph(dtype)
    fan = {k: [-1, -1] for k in eid}
    s_t, d_t = et[0], et[2]
    B = 10
    num_neg = math.ceil(B * amount)
    smp = _sampler(eid, nn, [-1, -1], dev, disjoint=disjoint, seed=1)
    pos = _positives(eid, et, B, 7)
    out = smp.sample_from_edges((et, pos), NegativeSampling(mode, amount), seed=21)
    n_s, n_d = out.node[s_t].long().cpu(), out.node[d_t].long().cpu()
    n_src = B + (num_neg if mode == 'binary' else 0)
    n_dst = B + num_neg
    if mode == 'binary':
        _, eli, label, src_time = out.metadata
        eli = eli.cpu()
        assert eli.shape == (2, B + num_neg) and src_time is None
        src_all, dst_all = n_s[eli[0]], n_d[eli[1]]
        assert torch.equal(label.cpu(), torch.cat([torch.ones(B), torch.zeros(num_neg)]))
        assert label.dtype == torch.float32
        if disjoint:
            ar = torch.arange(B + num_neg)
            assert torch.equal(eli[0], ar)
            assert torch.equal(eli[1], ar + (n_src if s_t == d_t else 0))
    else:
        _, src_index, dst_pos_index, dst_neg_index, src_time = out.metadata
        assert src_time is None
        assert dst_neg_index.shape == ((B, ) if amount == 1 else (B, amount))
        src_index, dst_pos_index = src_index.cpu(), dst_pos_index.cpu()
        dst_neg_index = dst_neg_index.cpu()
        off = n_src if s_t == d_t else 0
        if disjoint:
            assert torch.equal(src_index, torch.arange(B))
            assert torch.equal(dst_pos_index, torch.arange(B) + off)
            flat = torch.arange(B, n_dst) + off               # the slots in draw order
            assert int(dst_neg_index.min()) == B + off
            assert torch.equal(dst_neg_index, flat.view(-1, B).t().reshape(B, -1).squeeze(-1))
        else:
            flat = dst_neg_index.reshape(-1)                  # row-major: draw j at [j // amount]
        src_all = n_s[src_index]
        dst_all = torch.cat([n_d[dst_pos_index], n_d[flat]])
    # node[S][row 0] / node[D][row 1] reproduce cat([positives, negatives])
    assert torch.equal(src_all[:B], pos[0]) and torch.equal(dst_all[:B], pos[1])
    src_neg, dst_neg = src_all[B:], dst_all[B:]
    assert src_neg.numel() == n_src - B and dst_neg.numel() == num_neg
    assert bool((src_neg >= 0).all() and (src_neg < nn[s_t]).all())
    assert bool((dst_neg >= 0).all() and (dst_neg < nn[d_t]).all())
    # then everything equals the restatement fed with those negatives
    want, blk = hetero_link_sample(eid, nn, fan, et, pos[0].tolist(), pos[1].tolist(),
                                   disjoint=disjoint, mode=mode, amount=amount,
                                   src_neg=src_neg.tolist(), dst_neg=dst_neg.tolist())
    _assert_hops(out, want)
    _assert_metadata(out, blk, mode, dev)
    if disjoint:
        assert all(int(b.max()) < B for b in out.batch.values() if b.numel())
    # the same seed gives the same negatives, another seed others
    again = smp.sample_from_edges((et, pos), NegativeSampling(mode, amount), seed=21)
    assert _lists(again) == _lists(out)
    other = smp.sample_from_edges((et, pos), NegativeSampling(mode, amount), seed=22)
    assert _lists(other)[0] != _lists(out)[0]


# ---- 3. one node type, one edge type: NeighborSampler.sample_from_edges bit for bit ------------------
def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind,disjoint', [('uniform', False), ('uniform', True),
                                           ('weighted', False), ('weighted', True),
                                           ('temporal', True), ('edge_temporal', True)])
def test_one_type_equals_the_homogeneous_sampler(dev, dtype, kind, disjoint):
    from pytorch_geometric_amd.sampler import NegativeSampling, NeighborSampler
    N, B = 300, 24
    et = ('v', 'to', 'v')
    ei = _rand_ei(N, N, 3000, 11, dtype)
    g = gen(12)
    kw_homo, kw_het, weights, time = {}, {}, {}, None
    pos = ei[:, torch.randperm(ei.size(1), generator=g)[:B]].long()
    if kind == 'weighted':
        w = torch.rand(N, generator=g)
        w[::5] = 0
        weights = dict(src_weight=w.to(dev), dst_weight=w.flip(0).contiguous().to(dev))
    if kind == 'temporal':
        node_time = torch.randint(0, 50, (N, ), generator=g)
        node_time[[17, 40]] = -3                              # the earliest: 17 is the fallback
        kw_homo, kw_het = dict(node_time=node_time.to(dev)), dict(node_time={'v': node_time})
        time = torch.randint(0, 30, (B, ), generator=g)
        time[:3] = -5                                         # nothing is eligible there
    if kind == 'edge_temporal':
        edge_time = torch.randint(0, 50, (ei.size(1), ), generator=g)
        kw_homo, kw_het = dict(edge_time=edge_time.to(dev)), dict(edge_time={et: edge_time})
        time = torch.randint(0, 60, (B, ), generator=g)
    homo = NeighborSampler(ei.to(dev), N, [3, 2], disjoint=disjoint, seed=5, **kw_homo)
    het = _sampler({et: ei}, {'v': N}, [3, 2], dev, disjoint=disjoint, seed=5, **kw_het)
    label = torch.arange(B) % 4
    for neg in (None, NegativeSampling('binary', 1.5, **weights),
                NegativeSampling('triplet', 2, **weights)):
        triplet = neg is not None and neg.is_triplet()
        inp = SimpleNamespace(row=pos[0], col=pos[1], label=None if triplet else label,
                              time=time, input_id=torch.arange(B), input_type=None)
        ref = homo.sample_from_edges(inp, neg, seed=31)
        inp.input_type = et
        out = het.sample_from_edges(inp, neg, seed=31)
        assert _same(out.node['v'], ref.node)
        assert _same(out.row[et], ref.row) and _same(out.col[et], ref.col)
        assert _same(out.edge[et], ref.edge)
        assert _same(None if out.batch is None else out.batch['v'], ref.batch)
        assert out.num_sampled_nodes['v'] == ref.num_sampled_nodes
        assert out.num_sampled_edges[et] == ref.num_sampled_edges
        assert len(out.metadata) == len(ref.metadata) == (5 if triplet else 4)
        for a, b in zip(out.metadata, ref.metadata):
            assert _same(a, b)


# ---- 4. the kernel alone -------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('with_cdf', [False, True])
@pytest.mark.parametrize('with_time', [False, True])
def test_seed_block_kernel_equals_two_negative_draws(dev, dtype, with_cdf, with_time):
    from pytorch_geometric_amd import _native
    g = gen(40)
    n_s, n_d, base_s, base_d, P = 70, 45, 45, 0, 33         # the source type sits after the other
    src = torch.randint(0, n_s, (P, ), generator=g).to(dtype).to(dev)
    dst = torch.randint(0, n_d, (P, ), generator=g).to(dtype).to(dev)
    ends = [dict(num_nodes=n_s, node_base=base_s), dict(num_nodes=n_d, node_base=base_d)]
    kw = [dict(), dict()]
    link_time = None
    if with_cdf:
        for e, n in enumerate((n_s, n_d)):
            w = torch.rand(n, generator=g).double()
            w[::4] = 0
            kw[e]['cdf'] = torch.cumsum(w, 0).to(dev)
    if with_time:                                             # the destination type only
        nt = torch.randint(0, 100, (n_d, ), generator=g)
        link_time = torch.randint(0, 60, (P, ), generator=g).to(dev)
        kw[1].update(node_time=nt.to(dev), fallback=int(nt.argmin()))
    for e in range(2):
        ends[e].update(kw[e])
    for mode, num_neg in (('binary', 50), ('binary', 17), ('triplet', 66), (None, 0)):
        seed = 1234 + num_neg
        seeds, seed_time = _native.hetero_link_seeds(src, dst, num_neg, mode, seed, ends,
                                                     link_time=link_time)
        assert seeds.dtype == dtype
        want, want_t = [], []
        for e, (p, n, base) in enumerate(((src, n_s, base_s), (dst, n_d, base_d))):
            block = [p]
            if mode == 'binary' or (mode == 'triplet' and e == 1):
                block.append(_native.sample_negatives(
                    num_neg, n, seed * 2 + e, dev, dtype, cdf=kw[e].get('cdf'),
                    node_time=kw[e].get('node_time'),
                    bound=link_time if 'node_time' in kw[e] else None,
                    fallback=kw[e].get('fallback', 0)))
            block = torch.cat(block) + base
            want.append(block)
            if link_time is not None:
                want_t.append(link_time[torch.arange(block.numel(), device=dev) % P])
        assert torch.equal(seeds, torch.cat(want)), (mode, num_neg)
        if link_time is None:
            assert seed_time is None
        else:
            assert seed_time.dtype == torch.int64 and torch.equal(seed_time, torch.cat(want_t))
    # refusals with device tensors, before any launch
    with pytest.raises(ValueError, match="'num_neg' must be non-negative"):
        _native.hetero_link_seeds(src, dst, 5, None, 0, ends, link_time=link_time)
    with pytest.raises(ValueError, match="'cdf' must be"):
        _native.hetero_link_seeds(src, dst, 5, 'binary', 0,
                                  [dict(ends[0], cdf=torch.ones(n_s, device=dev)), ends[1]],
                                  link_time=link_time)
    with pytest.raises(ValueError, match='one length and one dtype'):
        _native.hetero_link_seeds(src, dst[:-1], 5, 'binary', 0, ends, link_time=link_time)
    bare = [dict(num_nodes=n_s, node_base=base_s), dict(num_nodes=n_d, node_base=base_d)]
    empty, _ = _native.hetero_link_seeds(src[:0], dst[:0], 0, 'binary', 0, bare)
    assert empty.numel() == 0


# ---- 5. the negatives' statistics per endpoint type --------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_negatives_marginals_per_endpoint(dev, dtype):
    from pytorch_geometric_amd import _native
    n_s, n_d, n, P = 97, 61, 200_000, 8
    z = torch.zeros(P, dtype=dtype, device=dev)
    ends = [dict(num_nodes=n_s, node_base=n_d), dict(num_nodes=n_d, node_base=0)]
    seeds, _ = _native.hetero_link_seeds(z, z, n, 'binary', 123, ends)
    blocks = seeds.long().cpu().view(2, P + n)[:, P:]
    for out, N, base in ((blocks[0], n_s, n_d), (blocks[1], n_d, 0)):
        assert int(out.min()) >= base and int(out.max()) < base + N
        c = torch.bincount(out - base, minlength=N)
        assert c.numel() == N
        p = 1 / N
        sigma = math.sqrt(n * p * (1 - p))
        assert float((c - n * p).abs().max()) <= 5 * sigma


@pytest.mark.parametrize('dtype', DTYPES)
def test_weighted_negatives_are_proportional_per_endpoint(dev, dtype):
    from pytorch_geometric_amd import _native
    n_s, n_d, n, P = 60, 43, 300_000, 8
    ws = (torch.arange(n_s) % 7).double()     # every 7th node has weight 0, node 0 included
    ws[n_s - 1] = 0.0                         # the last one as well
    wd = (torch.arange(n_d) % 5).double()
    wd[n_d - 1] = 0.0
    z = torch.zeros(P, dtype=dtype, device=dev)
    ends = [dict(num_nodes=n_s, node_base=0, cdf=torch.cumsum(ws, 0).to(dev)),
            dict(num_nodes=n_d, node_base=n_s, cdf=torch.cumsum(wd, 0).to(dev))]
    seeds, _ = _native.hetero_link_seeds(z, z, n, 'binary', 9, ends)
    blocks = seeds.long().cpu().view(2, P + n)[:, P:]
    for out, w, base in ((blocks[0], ws, 0), (blocks[1], wd, n_s)):
        N = w.numel()
        assert int(out.min()) >= base and int(out.max()) < base + N
        c = torch.bincount(out - base, minlength=N)
        assert int(c[w == 0].sum()) == 0
        p = w / w.sum()
        sigma = (n * p * (1 - p)).sqrt()
        assert bool(((c - n * p).abs() <= 5 * sigma + 1e-9).all())


# ---- 6. temporal -----------------------------------------------------------------------------------------
def _temporal_inputs():
    """Users are timed, items are not.  ``item_clock`` is NOT given to the sampler: it is what an
    item bound would test, and every entry lies above every link time, so a bounded item draw
    could only ever give the fallback (item 0, its earliest)."""
    g = gen(60)
    user_time = torch.randint(5, 80, (NN['user'], ), generator=g)
    user_time[[9, 20]] = 1                                    # the earliest: 9 is the fallback
    item_clock = 1000 + torch.arange(NN['item'])
    link_time = torch.randint(1, 60, (16, ), generator=g)
    link_time[:3] = 0                                         # no user is eligible there
    return user_time, item_clock, link_time


def test_temporal_inputs_show_what_they_should():
    """(No device work.)  The chosen inputs make the untimed endpoint's check certain: every item
    exceeds every bound; and some users are eligible for some links, none for the first three."""
    user_time, item_clock, link_time = _temporal_inputs()
    assert int(item_clock.min()) > int(link_time.max())
    assert int(item_clock.argmin()) == 0
    assert int(user_time.argmin()) == 9 and int(user_time.min()) > int(link_time[:3].max())
    assert bool((user_time[None, :] <= link_time[3:, None]).any(1).all())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('et,mode', [(RATES, 'binary'), (REV, 'binary'), (REV, 'triplet'),
                                     (FOLLOWS, 'binary')])
def test_temporal_node_level(dev, dtype, et, mode):
    eid, nn = _graph(dtype)
    user_time, item_clock, link_time = _temporal_inputs()
    B = link_time.numel()
    amount = 2
    smp = _sampler(eid, nn, [3, 2], dev, node_time={'user': user_time}, seed=2)
    assert smp.disjoint
    pos = _positives(eid, et, B, 8)
    inp = SimpleNamespace(row=pos[0], col=pos[1], time=link_time, input_id=None, label=None,
                          input_type=et)
    out = smp.sample_from_edges(inp, dict(mode=mode, amount=amount), seed=4)
    s_t, d_t = et[0], et[2]
    num_neg = B * amount
    n_src = B + (num_neg if mode == 'binary' else 0)
    src_time = out.metadata[-1].cpu()
    assert torch.equal(src_time, link_time.repeat(1 + amount)[:n_src])
    # every sampled (non-seed) user of tree i is no later than the tree's seed time
    users, trees = out.node['user'].long().cpu(), out.batch['user'].long().cpu()
    n0 = out.num_sampled_nodes['user'][0]
    assert int(trees.max()) < B
    assert bool((user_time[users[n0:]] <= link_time[trees[n0:]]).all())
    assert users.numel() > n0
    # the seed blocks, in seed-dict order inside node[t]
    src_all = out.node[s_t].long().cpu()[:n_src]
    off = n_src if s_t == d_t else 0
    dst_all = out.node[d_t].long().cpu()[off:off + B + num_neg]
    assert torch.equal(src_all[:B], pos[0]) and torch.equal(dst_all[:B], pos[1])
    j = torch.arange(num_neg)
    for neg, t in ((src_all[B:], s_t), (dst_all[B:], d_t)):
        if neg.numel() == 0:
            continue
        if t == 'user':     # timed: the bound, or the fallback
            ok = (user_time[neg] <= link_time[j % B]) | (neg == 9)
            assert bool(ok.all())
            assert bool((neg[j % B < 3] == 9).all())
            assert int((neg != 9).sum()) > 0
        else:               # untimed: never bounded.  A bounded draw would be item 0 everywhere
            assert bool((item_clock[neg] > link_time[j % B]).all())
            assert neg.unique().numel() > 5


@pytest.mark.parametrize('dtype', DTYPES)
def test_temporal_edge_level(dev, dtype):
    eid, nn = _graph(dtype)
    g = gen(61)
    edge_time = {RATES: torch.randint(0, 50, (eid[RATES].size(1), ), generator=g),
                 FOLLOWS: torch.randint(0, 50, (eid[FOLLOWS].size(1), ), generator=g)}
    B = 12
    link_time = torch.randint(0, 40, (B, ), generator=g)
    smp = _sampler(eid, nn, [-1, -1], dev, edge_time=edge_time, seed=2)
    pos = _positives(eid, RATES, B, 8)
    inp = SimpleNamespace(row=pos[0], col=pos[1], time=link_time, input_id=None, label=None,
                          input_type=RATES)
    out = smp.sample_from_edges(inp, 'binary', seed=4)
    for et, times in edge_time.items():
        e, c = out.edge[et].long().cpu(), out.col[et].long().cpu()
        tree = out.batch[et[2]].long().cpu()[c]
        assert e.numel() > 0
        assert bool((times[e] <= link_time[tree]).all())
    # edge-level time never bounds the negatives: both endpoints draw freely
    assert out.node['user'][B:2 * B].unique().numel() > 3
    assert out.node['item'][B:2 * B].unique().numel() > 3
    with pytest.raises(ValueError, match='needs the seed-link times'):
        smp.sample_from_edges((RATES, pos))


# ---- 7. the loader ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('et', [RATES, REV, FOLLOWS])
def test_loader(dev, dtype, et):
    from pytorch_geometric_amd.loader import HeteroLinkBatch, HeteroLinkNeighborLoader
    eid, nn = _graph(dtype)
    eid = {k: v.to(dev) for k, v in eid.items()}
    x = {t: (torch.arange(n, dtype=torch.float32).view(-1, 1) + (1000 if t == 'item' else 0)
             ).repeat(1, 3).to(dev) for t, n in nn.items()}
    s_t, d_t = et[0], et[2]
    links = eid[et].long()
    L = links.size(1)

    def batches(prefetch, **kw):
        loader = HeteroLinkNeighborLoader(x, eid, [3, 2], (et, None), batch_size=16,
                                          shuffle=True, seed=5, prefetch=prefetch, **kw)
        assert len(loader) == -(-L // 16)
        return list(loader)

    got = batches(0, neg_sampling_ratio=1.0)
    assert len(got) == -(-L // 16)
    seen = []
    for b in got:
        assert isinstance(b, HeteroLinkBatch) and b.input_type == et
        B = b.batch_size
        assert B == b.input_id.numel() and b.edge_label_index.shape == (2, 2 * B)
        for t in nn:
            assert torch.equal(b.x_dict[t], x[t][b.n_id[t].long()])
        sel = links[:, b.input_id]
        assert torch.equal(b.n_id[s_t].long()[b.edge_label_index[0, :B]], sel[0])
        assert torch.equal(b.n_id[d_t].long()[b.edge_label_index[1, :B]], sel[1])
        assert bool((b.edge_label[:B] == 1).all()) and bool((b.edge_label[B:] == 0).all())
        for k, ei in b.edge_index_dict.items():
            e = b.e_id[k].long()
            assert torch.equal(b.n_id[k[0]].long()[ei[0].long()], eid[k].long()[0, e])
            assert torch.equal(b.n_id[k[2]].long()[ei[1].long()], eid[k].long()[1, e])
        seen.append(b.input_id)
    assert sorted(torch.cat(seen).tolist()) == list(range(L))
    ahead = batches(2, neg_sampling_ratio=1.0)
    assert len(ahead) == len(got)
    for a, b in zip(ahead, got):
        assert torch.equal(a.input_id, b.input_id)
        assert torch.equal(a.edge_label_index, b.edge_label_index)
        for t in nn:
            assert torch.equal(a.n_id[t], b.n_id[t]) and torch.equal(a.x_dict[t], b.x_dict[t])
        for k in eid:
            assert torch.equal(a.edge_index_dict[k], b.edge_index_dict[k])
            assert torch.equal(a.e_id[k], b.e_id[k])
    # triplet fields, labels, drop_last
    lab = torch.arange(L, device=dev) % 2
    loader = HeteroLinkNeighborLoader(x, eid, [2], (et, links[:, :40]), edge_label=lab[:40],
                                      neg_sampling='binary', batch_size=16, drop_last=True)
    assert len(loader) == 2
    for b in loader:
        assert torch.equal(b.edge_label[:16], lab[b.input_id] + 1)   # 0 now denotes "negative"
    loader = HeteroLinkNeighborLoader(x, eid, [2], (et, links[:, :40]), batch_size=8,
                                      neg_sampling=dict(mode='triplet', amount=2), disjoint=True)
    for b in loader:
        assert b.edge_label_index is None and b.dst_neg_index.shape == (8, 2)
        assert torch.equal(b.n_id[s_t].long()[b.src_index], links[0, b.input_id])
        assert torch.equal(b.n_id[d_t].long()[b.dst_pos_index], links[1, b.input_id])
        assert all(int(v.max()) < 8 for v in b.batch.values() if v.numel())
    with pytest.raises(ValueError, match=r"\[0, \d+\) for node type"):
        HeteroLinkNeighborLoader(x, eid, [2], (et, torch.full((2, 3), 50, device=dev)))


# ---- 8. through the reference's LinkLoader ---------------------------------------------------------------
def _reference_data(dev, temporal=False):
    try:
        from oracle import make_ref
        make_ref.import_reference()
        from torch_geometric.data import HeteroData
    except ImportError:
        pytest.skip('torch_geometric cannot be imported')
    data = HeteroData()
    data['paper'].x = torch.arange(100)
    data['author'].x = torch.arange(100, 300)
    data['paper', 'to', 'paper'].edge_index = _rand_ei(100, 100, 400, 71)
    data['paper', 'to', 'author'].edge_index = _rand_ei(100, 200, 1000, 72)
    data['author', 'to', 'paper'].edge_index = _rand_ei(200, 100, 1000, 73)
    if temporal:
        data['paper'].time = torch.arange(100)
        data['author'].time = torch.arange(200)
    return data.to(dev)


def _pairs(ei):
    return set(map(tuple, ei.t().tolist()))


@pytest.mark.parametrize('neg_sampling_ratio', [None, 1.0])
def test_reference_link_loader_basic(dev, neg_sampling_ratio):
    """test_hetero_link_neighbor_loader_basic / _loop, 'directional'."""
    data = _reference_data(dev)
    from torch_geometric.data import HeteroData
    from torch_geometric.loader import LinkLoader
    from torch_geometric.sampler import NegativeSampling
    from pytorch_geometric_amd import backend
    smp = backend.neighbor_sampler(data, [-1] * 2, seed=3)
    neg = None if neg_sampling_ratio is None else NegativeSampling('binary', neg_sampling_ratio)
    for et in (('paper', 'to', 'author'), ('paper', 'to', 'paper')):
        eli = data[et].edge_index
        loader = LinkLoader(data, link_sampler=smp, edge_label_index=(et, eli), batch_size=20,
                            neg_sampling=neg, shuffle=True)
        assert len(loader) == eli.size(1) / 20
        for i, batch in enumerate(loader):
            assert isinstance(batch, HeteroData) and batch.input_type == et
            store = batch[et]
            assert batch['paper'].x.min() >= 0 and batch['paper'].x.max() < 100
            assert torch.equal(batch['paper'].x, data['paper'].x[batch['paper'].n_id])
            glob = torch.stack([batch[et[0]].n_id[store.edge_label_index[0, :20]],
                                batch[et[2]].n_id[store.edge_label_index[1, :20]]])
            assert torch.equal(glob, eli[:, store.input_id])
            if neg is None:
                # the positives are edges of the sampled subgraph (first hop, every in-edge)
                assert store.edge_label_index.size(1) == 20
                assert _pairs(store.edge_label_index.cpu()) <= _pairs(store.edge_index.cpu())
            else:
                assert store.edge_label_index.size(1) == 40
                assert bool((store.edge_label[:20] == 1).all())
                assert bool((store.edge_label[20:] == 0).all())
            if i == 4:
                break


@pytest.mark.parametrize('disjoint', [False, True])
@pytest.mark.parametrize('temporal', [False, True])
@pytest.mark.parametrize('amount', [1, 2])
def test_reference_link_loader_triplet(dev, disjoint, temporal, amount):
    """test_hetero_link_neighbor_loader_triplet."""
    if not disjoint and temporal:
        return
    data = _reference_data(dev, temporal)
    from torch_geometric.loader import LinkLoader
    from torch_geometric.sampler import NegativeSampling
    from pytorch_geometric_amd import backend
    et = ('paper', 'to', 'paper')
    eli = _rand_ei(100, 100, 500, 74).to(dev)
    edge_label_time = None
    if temporal:
        edge_label_time = torch.max(data['paper'].time[eli[0]], data['paper'].time[eli[1]]) + 50
    weight = None if temporal else torch.rand(100, generator=gen(75)).to(dev)
    bs = 20
    smp = backend.neighbor_sampler(data, [-1] * 2, disjoint=disjoint,
                                   time_attr='time' if temporal else None)
    loader = LinkLoader(data, link_sampler=smp, edge_label_index=(et, eli),
                        edge_label_time=edge_label_time, batch_size=bs, shuffle=True,
                        neg_sampling=NegativeSampling('triplet', amount, src_weight=weight,
                                                      dst_weight=weight))
    assert len(loader) == 500 / bs
    for i, batch in enumerate(loader):
        node, edge = batch['paper'], batch[et]
        assert torch.equal(node.x[node.src_index], eli[0, edge.input_id])
        assert torch.equal(node.x[node.dst_pos_index], eli[1, edge.input_id])
        assert node.dst_neg_index.size() == ((bs, ) if amount == 1 else (bs, amount))
        assert node.dst_neg_index.min() >= 0 and node.dst_neg_index.max() < node.num_nodes
        if disjoint:
            assert node.src_index.min() == 0 and node.src_index.max() == bs - 1
            assert node.dst_pos_index.min() == bs and node.dst_pos_index.max() == 2 * bs - 1
            assert node.dst_neg_index.min() == 2 * bs
            max_seed_nodes = 2 * bs + bs * amount
            assert node.dst_neg_index.max() == max_seed_nodes - 1
            assert node.batch.min() == 0 and node.batch.max() == bs - 1
            for lo in range(0, max_seed_nodes, bs):
                assert torch.equal(node.batch[lo:lo + bs].long(), torch.arange(bs, device=dev))
        if temporal:
            for t in range(bs):
                assert node.time[node.batch == t].max() <= node.seed_time[t]
                a = batch['author']
                if bool((a.batch == t).any()):
                    assert a.time[a.batch == t].max() <= node.seed_time[t]
        if i == 4:
            break


def test_reference_link_loader_two_types_disjoint_and_temporal(dev):
    """The triplet index layout for ``S != D`` in disjoint mode, and test_temporal_hetero_link_
    neighbor_loader's bounds, with seed links between two node types."""
    data = _reference_data(dev, temporal=True)
    from torch_geometric.loader import LinkLoader
    from torch_geometric.sampler import NegativeSampling
    from pytorch_geometric_amd import backend
    et = ('paper', 'to', 'author')
    eli = data[et].edge_index[:, :200]
    bs, amount = 20, 2
    smp = backend.neighbor_sampler(data, [-1] * 2, disjoint=True)
    loader = LinkLoader(data, link_sampler=smp, edge_label_index=(et, eli), batch_size=bs,
                        neg_sampling=NegativeSampling('triplet', amount))
    for batch in loader:
        p, a = batch['paper'], batch['author']
        assert torch.equal(p.src_index, torch.arange(bs, device=dev))
        assert torch.equal(a.dst_pos_index, torch.arange(bs, device=dev))
        assert a.dst_neg_index.size() == (bs, amount) and a.dst_neg_index.min() == bs
        assert a.dst_neg_index.max() == bs + bs * amount - 1
        assert torch.equal(p.x[p.src_index], eli[0, batch[et].input_id])
        assert torch.equal(a.x[a.dst_pos_index] - 100, eli[1, batch[et].input_id])
        assert torch.equal(p.batch[:bs].long(), torch.arange(bs, device=dev))
        for lo in range(0, bs + bs * amount, bs):
            assert torch.equal(a.batch[lo:lo + bs].long(), torch.arange(bs, device=dev))
    smp = backend.neighbor_sampler(data, [-1] * 2, time_attr='time')
    time = torch.max(data['paper'].time[eli[0]], data['author'].time[eli[1]])
    # (an integer ratio: the reference's `batch % P` names a tree's positive link, and so its seed
    # time, only when the number of source seeds is a multiple of P)
    loader = LinkLoader(data, link_sampler=smp, edge_label_index=(et, eli), edge_label_time=time,
                        batch_size=bs, neg_sampling=NegativeSampling('binary', 1.0))
    for batch in loader:
        store = batch[et]
        assert store.edge_label_index.size(1) == 2 * bs
        assert torch.equal(store.edge_label_time[:bs], time[store.input_id])
        assert torch.equal(store.edge_label_time[bs:], time[store.input_id])
        assert int(batch['paper'].batch.max()) + 1 == bs
        for t in ('paper', 'author'):
            node = batch[t]
            n0 = 2 * bs                                        # the seeds of either type
            assert bool((node.time[n0:] <= store.edge_label_time[node.batch[n0:].long()]).all())
            assert node.time.numel() > n0
