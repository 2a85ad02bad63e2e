"""Weighted neighbour sampling on the GPU: the reference's ``NeighborLoader(..., weight_attr=...)``
(loader/neighbor_loader.py:168-174 -> sampler/neighbor_sampler.py:110-114, 559-571).  pyg-lib's
weighted draws cannot run here and are implementation-defined anyway, so what is pinned is the
known answer of the reference's own weighted-loader test, the exact successive-sampling inclusion
probabilities, the proportional draws with replacement and the structural contract.  The RNG is
counter-based: every statistical check below is deterministic for its fixed seeds."""
import itertools
import math

import pytest
import torch

from tests._util import gen, random_graph
from tests.test_gpu_sampler import _check_contract

pytestmark = pytest.mark.gpu

DTYPES = [torch.int64, torch.int32]


def _sampler(ei, n, fan, w, dev, dtype=torch.int64, **kw):
    from pytorch_geometric_amd.sampler import NeighborSampler
    return NeighborSampler(ei.to(dtype).to(dev), n, fan, edge_weight=w.to(dev), **kw)


def _star_batch(w_rows, n_dst, seed=0):
    """``n_dst`` destinations with the same ``len(w_rows)`` in-edges each (sources shared), in a
    shuffled edge order; returns (edge_index, weights, slot label of every edge, N)."""
    d = len(w_rows)
    dst = torch.arange(n_dst).repeat_interleave(d)
    slot = torch.arange(d).repeat(n_dst)
    src = n_dst + slot
    order = torch.randperm(dst.numel(), generator=gen(seed))
    ei = torch.stack([src, dst])[:, order]
    w = torch.tensor(w_rows, dtype=torch.float64).repeat(n_dst)[order]
    return ei, w, slot[order], n_dst + d


def _successive_inclusion(w, k):
    """P(slot j in the sample) for successive sampling of k slots in proportion to w."""
    d = len(w)
    p = [0.0] * d
    for seq in itertools.permutations(range(d), k):
        pr, left = 1.0, float(sum(w))
        for j in seq:
            if left <= 0 or w[j] == 0:
                pr = 0.0
                break
            pr *= w[j] / left
            left -= w[j]
        for j in seq:
            p[j] += pr
    return p


def _within_sigmas(count, n, p, sig=5.0):
    sd = math.sqrt(max(p * (1 - p), 1e-12) / n)
    return abs(count / n - p) <= sig * sd + 1e-12


@pytest.mark.parametrize('dtype', DTYPES)
def test_weighted_known_answer_of_the_reference_loader_test(dev, dtype):
    """test/loader/test_neighbor_loader.py:822-846 (test_weighted_homo_neighbor_loader): the
    zero-weight edges are never drawn, whatever the seed."""
    ei = torch.tensor([[1, 3, 0, 4], [2, 2, 1, 3]])
    w = torch.tensor([0.0, 1.0, 0.0, 1.0])
    for replace in (False, True):
        s = _sampler(ei, 5, [1, 1], w, dev, dtype, replace=replace)
        for rng in range(20):
            out = s.sample_from_nodes(torch.tensor([2], device=dev), seed=rng)
            assert out.node.cpu().tolist() == [2, 3, 4]
            assert ei[:, out.edge.cpu()].tolist() == [[3, 4], [2, 3]]
            assert out.num_sampled_nodes == [1, 1, 1] and out.num_sampled_edges == [1, 1]


@pytest.mark.parametrize('dtype', DTYPES)
def test_weighted_without_replacement_matches_successive_sampling(dev, dtype):
    w_rows = [1.0, 2.0, 3.0, 4.0, 0.0, 10.0]
    n_dst, k = 4096, 2
    ei, w, slot, N = _star_batch(w_rows, n_dst, seed=1)
    s = _sampler(ei, N, [k], w, dev, dtype)
    out = s.sample_from_nodes(torch.arange(n_dst, device=dev), seed=3)
    edge = out.edge.cpu()
    assert edge.numel() == n_dst * k and edge.unique().numel() == edge.numel()
    assert torch.equal(torch.bincount(out.col.cpu(), minlength=n_dst),
                       torch.full((n_dst, ), k))
    hits = torch.bincount(slot[edge], minlength=len(w_rows))
    assert int(hits[4]) == 0                                  # the zero-weight slot never
    want = _successive_inclusion(w_rows, k)
    for j, p in enumerate(want):
        assert _within_sigmas(int(hits[j]), n_dst, p), (j, int(hits[j]) / n_dst, p)
    # only 2 positive weights, k = 3: both always, the third place uniform over the zero slots
    w_rows = [5.0, 0.0, 0.0, 7.0, 0.0, 0.0]
    ei, w, slot, N = _star_batch(w_rows, n_dst, seed=2)
    s = _sampler(ei, N, [3], w, dev, dtype)
    out = s.sample_from_nodes(torch.arange(n_dst, device=dev), seed=4)
    hits = torch.bincount(slot[out.edge.cpu()], minlength=6)
    assert int(hits[0]) == int(hits[3]) == n_dst
    for j in (1, 2, 4, 5):
        assert _within_sigmas(int(hits[j]), n_dst, 0.25), (j, int(hits[j]))


@pytest.mark.parametrize('dtype', DTYPES)
def test_weighted_with_replacement_is_proportional(dev, dtype):
    w_rows = [1.0, 2.0, 3.0, 4.0, 0.0, 10.0]
    n_dst, n_zero, k = 4096, 1024, 8
    ei, w, slot, N = _star_batch(w_rows, n_dst, seed=5)
    # n_zero more destinations whose weights are all zero: uniform draws
    dst_z = torch.arange(N, N + n_zero).repeat_interleave(6)
    ei_z = torch.stack([n_dst + torch.arange(6).repeat(n_zero), dst_z])
    ei = torch.cat([ei, ei_z], 1)
    w = torch.cat([w, torch.zeros(6 * n_zero, dtype=w.dtype)])
    slot = torch.cat([slot, torch.arange(6).repeat(n_zero)])
    s = _sampler(ei, N + n_zero, [k], w, dev, dtype, replace=True)
    seeds = torch.cat([torch.arange(n_dst), torch.arange(N, N + n_zero)]).to(dev)
    out = s.sample_from_nodes(seeds, seed=6)
    edge, col = out.edge.cpu(), out.col.cpu()
    assert torch.equal(torch.bincount(col, minlength=seeds.numel()),
                       torch.full((seeds.numel(), ), k))
    weighted = col < n_dst
    hits = torch.bincount(slot[edge[weighted]], minlength=6)
    assert int(hits[4]) == 0
    total = sum(w_rows)
    for j, wj in enumerate(w_rows):
        assert _within_sigmas(int(hits[j]), n_dst * k, wj / total), (j, int(hits[j]))
    hits = torch.bincount(slot[edge[~weighted]], minlength=6)
    for j in range(6):
        assert _within_sigmas(int(hits[j]), n_zero * k, 1 / 6), (j, int(hits[j]))


def test_weighted_hubs(dev):
    """In-degree 100 000: many chunks, most of them skipped after the first few."""
    deg, k = 100_000, 10
    ei = torch.stack([torch.arange(1, deg + 1), torch.zeros(deg, dtype=torch.long)])
    w = torch.ones(deg)
    heavy = 31_337
    w[heavy] = 1e6
    for replace in (False, True):
        s = _sampler(ei, deg + 1, [k], w, dev, replace=replace)
        for rng in range(8):
            e = s.sample_from_nodes(torch.tensor([0], device=dev), seed=rng).edge.cpu()
            assert e.numel() == k and bool((e == heavy).any()), (replace, rng)
            if not replace:
                assert e.unique().numel() == k
    # 64 hubs sharing one random weight vector (6.4 M edges)
    hubs = 64
    wv = torch.rand(deg, generator=gen(7)) + 1e-3
    src = torch.arange(hubs, hubs + deg).repeat(hubs)
    dst = torch.arange(hubs).repeat_interleave(deg)
    ei = torch.stack([src, dst])
    s = _sampler(ei, hubs + deg, [k], wv.repeat(hubs), dev, dtype=torch.int32)
    hits = torch.zeros(deg)
    for rng in range(10):
        out = s.sample_from_nodes(torch.arange(hubs, device=dev), seed=rng)
        e = out.edge.cpu().long()
        assert e.numel() == hubs * k
        assert torch.equal(torch.bincount(out.col.cpu().long(), minlength=hubs),
                           torch.full((hubs, ), k))
        hits += torch.bincount(e % deg, minlength=deg).float()
    order = wv.argsort()
    dec = hits[order].view(10, -1).sum(1)
    assert float(dec[-1]) >= 3 * float(dec[0]), dec
    assert float(dec[0]) < float(dec[4]) < float(dec[-1]), dec


@pytest.mark.parametrize('dtype', DTYPES)
def test_weighted_structural_contract(dev, dtype):
    n = 3000
    ei = random_graph(n, n, 40_000, seed=1, skew=True)
    w = torch.rand(ei.size(1), generator=gen(4)) + 0.01
    seeds = torch.randperm(n, generator=gen(2))[:200]
    for fanouts in ([15, 10, 5], [3, -1], [64]):
        s = _sampler(ei, n, fanouts, w, dev, dtype, seed=7)
        out = s.sample_from_nodes(seeds.to(dev))
        _check_contract(out, ei, seeds, fanouts)
        assert int((s._local != s._unset).sum()) == 0             # map reset for the next batch
        a = s.sample_from_nodes(seeds.to(dev), seed=7)
        b = s.sample_from_nodes(seeds.to(dev), seed=7)
        for f in ('node', 'row', 'col', 'edge'):
            assert torch.equal(getattr(a, f), getattr(b, f)), f
        c = s._hops_synced(seeds.to(dev).to(dtype), 7)               # synced == sync-free
        for f in ('node', 'row', 'col', 'edge'):
            assert torch.equal(getattr(a, f), getattr(c, f)), f
        assert a.num_sampled_nodes == c.num_sampled_nodes
        assert a.num_sampled_edges == c.num_sampled_edges
        assert int((s._local != s._unset).sum()) == 0
    # the weights change the draws (the uniform sampler gives another batch for the same seed)
    from pytorch_geometric_amd.sampler import NeighborSampler
    u = NeighborSampler(ei.to(dtype).to(dev), n, [15, 10, 5]).sample_from_nodes(seeds.to(dev),
                                                                                 seed=7)
    wt = _sampler(ei, n, [15, 10, 5], w, dev, dtype).sample_from_nodes(seeds.to(dev), seed=7)
    assert not torch.equal(u.edge, wt.edge)


def test_equal_weights_give_uniform_marginals(dev):
    """20 in-neighbours of equal weight, k = 5: every neighbour ~25 % of the time."""
    n_dst = 4096
    ei, w, slot, N = _star_batch([2.5] * 20, n_dst, seed=8)
    s = _sampler(ei, N, [5], w, dev)
    out = s.sample_from_nodes(torch.arange(n_dst, device=dev), seed=9)
    hits = torch.bincount(slot[out.edge.cpu()], minlength=20)
    assert int(hits.sum()) == 5 * n_dst
    for j in range(20):
        assert _within_sigmas(int(hits[j]), n_dst, 0.25), (j, int(hits[j]))


def test_weighted_options(dev):
    """disjoint, 'bidirectional' and 'induced' with weights."""
    ei = torch.tensor([[1, 3, 0, 4], [2, 2, 1, 3]])
    w = torch.tensor([0.0, 1.0, 0.0, 1.0])
    for replace in (False, True):
        s = _sampler(ei, 5, [1, 1], w, dev, disjoint=True, replace=replace)
        for rng in range(5):
            out = s.sample_from_nodes(torch.tensor([2, 2], device=dev), seed=rng)
            assert out.node.cpu().tolist() == [2, 2, 3, 3, 4, 4]
            assert out.batch.cpu().tolist() == [0, 1, 0, 1, 0, 1]
            assert sorted(out.edge.cpu().tolist()) == [1, 1, 3, 3]
    n = 800
    ei = random_graph(n, n, 6000, seed=2, skew=True)
    w = torch.rand(ei.size(1), generator=gen(3))
    w[::3] = 0
    seeds = torch.randperm(n, generator=gen(8))[:60].to(dev)
    d = _sampler(ei, n, [4, 3], w, dev, seed=5).sample_from_nodes(seeds, seed=5)
    for st in ('bidirectional', 'induced'):
        b = _sampler(ei, n, [4, 3], w, dev, seed=5, subgraph_type=st).sample_from_nodes(seeds,
                                                                                        seed=5)
        assert torch.equal(b.node, d.node), st
    # disjoint keeps the weighted contract: no zero-weight edge where a positive one was left
    s = _sampler(ei, n, [2], w, dev, disjoint=True)
    out = s.sample_from_nodes(seeds, seed=1)
    e = out.edge.cpu()
    wz = w[e] == 0
    if bool(wz.any()):
        pos = torch.zeros(n, dtype=torch.long).index_add_(0, ei[1], (w > 0).long())
        dst_nodes = out.node.cpu()[out.col.cpu()[wz]]
        assert bool((pos[dst_nodes] < 2).all())


def test_weighted_padded_sampling_is_hipgraph_capturable(dev):
    """sample_padded with weights: captured once, replayed with a bumped seed word, equals the
    eager call for the same word."""
    g = gen(92)
    N = 2000
    ei = torch.randint(0, N, (2, 30000), generator=g)
    ei[1, :3000] = 5                                        # a hub: several chunks
    w = torch.rand(ei.size(1), generator=g)
    s = _sampler(ei, N, [5, 3], w, dev, seed=3)
    static_seeds = torch.cat([torch.tensor([5]), torch.randperm(N, generator=g)[:31]]).to(dev)
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    s.sample_padded(static_seeds, seed=9, seed_dev=word)   # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p = s.sample_padded(static_seeds, seed=9, seed_dev=word)
    prev = None
    for bump in (1, 2):
        word.fill_(bump)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in p.new_nodes + p.rows + p.cols + p.edges + p.n_nodes
               + p.n_edges]
        q = s.sample_padded(static_seeds, seed=9,
                            seed_dev=torch.full((1, ), bump, dtype=torch.int64, device=dev))
        want = q.new_nodes + q.rows + q.cols + q.edges + q.n_nodes + q.n_edges
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        if prev is not None:
            assert not all(torch.equal(a, b) for a, b in zip(got, prev))
        prev = got
    assert int((s._local != s._unset).sum()) == 0


def test_weighted_loader(dev):
    from pytorch_geometric_amd.loader import NeighborLoader
    from pytorch_geometric_amd.sampler import NeighborSampler
    n = 2000
    ei = random_graph(n, n, 20_000, seed=6, skew=True).to(dev)
    w = (torch.rand(ei.size(1), generator=gen(6)) * 3).to(dev)
    x = torch.randn(n, 8, generator=gen(7)).to(dev)
    loader = NeighborLoader(x, ei, [5, 3], batch_size=256, seed=5, edge_weight=w,
                            input_nodes=torch.arange(1024, device=dev))
    ref = NeighborSampler(ei, n, [5, 3], edge_weight=w)
    for b, batch in enumerate(loader):
        want = ref.sample_from_nodes(batch.n_id[:batch.batch_size], seed=5 + b)
        assert torch.equal(batch.n_id, want.node) and torch.equal(batch.e_id, want.edge)
        assert torch.equal(batch.x, x[want.node])
    with pytest.raises(NotImplementedError):
        loader.collate_slots(torch.arange(256, device=dev),
                             torch.ones(1, dtype=torch.int64, device=dev))
    assert loader._slots is None


def test_weight_validation(dev):
    from pytorch_geometric_amd.sampler import NeighborSampler
    ei = torch.tensor([[1, 3, 0, 4], [2, 2, 1, 3]]).to(dev)
    bad = [torch.tensor([1.0, -1.0, 0.0, 1.0]), torch.tensor([1.0, float('nan'), 0.0, 1.0]),
           torch.tensor([1.0, float('inf'), 0.0, 1.0]), torch.ones(3), torch.ones(5),
           torch.ones(4, dtype=torch.int64), torch.ones(2, 2), torch.tensor([1e300, 1, 1, 1],
                                                                            dtype=torch.float64)]
    for w in bad:
        with pytest.raises(ValueError):
            NeighborSampler(ei, 5, [1], edge_weight=w.to(dev))
    s = NeighborSampler(ei, 5, [1], edge_weight=torch.tensor([0, 1, 0, 1], dtype=torch.float64,
                                                             device=dev))
    assert s.edge_weight.dtype == torch.float32 and s.edge_weight.is_contiguous()
    assert torch.equal(s.edge_weight.cpu(), torch.tensor([0.0, 0.0, 1.0, 1.0]))  # CSC order
