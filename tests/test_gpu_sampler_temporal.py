"""Temporal neighbour sampling on the GPU: the reference's ``NeighborLoader(..., time_attr=...,
input_time=..., temporal_strategy=...)`` (loader/neighbor_loader.py:150-165, 223-226 ->
sampler/neighbor_sampler.py:79-108, 386-395, 550-571, sampler/utils.py:24-42).  pyg-lib cannot run
here, so the rules are restated below as a pure-Python per-tree BFS: the deterministic draws
(``'last'`` without replacement, and every ``-1`` hop) must equal it exactly; bounded
``'uniform'`` draws keep the contract on the eligible window, with marginal frequencies checked
against ``k / window``, and equal the disjoint sampler bit for bit when every edge is eligible.
The RNG is counter-based: every statistical check below is deterministic for its fixed seeds."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests._util import gen

pytestmark = pytest.mark.gpu

DTYPES = [torch.int64, torch.int32]


def _sampler(ei, n, fan, dev, dtype=torch.int64, node_time=None, edge_time=None, **kw):
    from pytorch_geometric_amd.sampler import NeighborSampler
    mv = (lambda t: None if t is None else t.to(dev))
    return NeighborSampler(ei.to(dtype).to(dev), n, fan, node_time=mv(node_time),
                           edge_time=mv(edge_time), **kw)


def _oracle(ei, n, seeds, fan, node_time=None, edge_time=None, seed_time=None):
    """Rules 1-8 of temporal sampling with 'last' (or -1 hops), one tree per seed: slots of a
    destination sorted by (time, edge position), the eligible prefix (time <= the root's seed
    time), its last k slots; nodes as (tree, node) pairs in order of first appearance per hop,
    edges by frontier position then slot order."""
    src, dst = ei[0].tolist(), ei[1].tolist()
    key = edge_time.tolist() if edge_time is not None else [int(node_time[u]) for u in src]
    col_slots = [[] for _ in range(n)]
    for e in range(len(src)):
        col_slots[dst[e]].append(e)
    for v in range(n):
        col_slots[v].sort(key=lambda e: (key[e], e))
    seeds = seeds.tolist()
    st = seed_time.tolist() if seed_time is not None else [int(node_time[s]) for s in seeds]
    nodes = [(i, s) for i, s in enumerate(seeds)]
    pos = {p: i for i, p in enumerate(nodes)}
    rows, cols, edges = [], [], []
    nsn, nse = [len(seeds)], []
    frontier = list(range(len(seeds)))
    for k in fan:
        new, ne = [], 0
        for fp in frontier:
            t, v = nodes[fp]
            elig = [e for e in col_slots[v] if key[e] <= st[t]]
            take = elig if k < 0 else elig[max(0, len(elig) - k):]
            for e in take:
                p = (t, src[e])
                if p not in pos:
                    pos[p] = len(nodes)
                    nodes.append(p)
                    new.append(pos[p])
                rows.append(pos[p])
                cols.append(fp)
                edges.append(e)
                ne += 1
        nsn.append(len(new))
        nse.append(ne)
        frontier = new
    return dict(node=[v for _, v in nodes], batch=[t for t, _ in nodes], row=rows, col=cols,
                edge=edges, num_sampled_nodes=nsn, num_sampled_edges=nse)


def _as_dict(out):
    return dict(node=out.node.cpu().tolist(), batch=out.batch.cpu().tolist(),
                row=out.row.cpu().tolist(), col=out.col.cpu().tolist(),
                edge=out.edge.cpu().tolist(), num_sampled_nodes=list(out.num_sampled_nodes),
                num_sampled_edges=list(out.num_sampled_edges))


def _tied_graph(seed, n=40, m=260, n_times=5):
    g = gen(seed)
    ei = torch.stack([torch.randint(0, n, (m, ), generator=g),
                      torch.randint(0, n, (m, ), generator=g)])
    node_time = torch.randint(0, n_times, (n, ), generator=g)
    edge_time = torch.randint(0, n_times, (m, ), generator=g)
    seeds = torch.randint(0, n, (12, ), generator=g)
    # below all, equal to some, above all neighbour times
    seed_time = torch.tensor([-3, 0, 1, 2, 3, 4, 99, 2, 0, 4, -1, 1])
    return ei, n, node_time, edge_time, seeds, seed_time


FANS = [[3, -1], [2, 2, 2], [-1, 1], [1, -1, 2], [0, 3]]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('level', ['node', 'edge'])
def test_last_without_replacement_equals_the_oracle(dev, dtype, level):
    for gseed in range(4):
        ei, n, nt, et, seeds, st = _tied_graph(gseed)
        for fan in FANS:
            if level == 'node':
                s = _sampler(ei, n, fan, dev, dtype, node_time=nt, temporal_strategy='last')
                cases = [(None, _oracle(ei, n, seeds, fan, node_time=nt)),
                         (st, _oracle(ei, n, seeds, fan, node_time=nt, seed_time=st))]
            else:
                s = _sampler(ei, n, fan, dev, dtype, edge_time=et, temporal_strategy='last')
                cases = [(st, _oracle(ei, n, seeds, fan, edge_time=et, seed_time=st))]
            for time, want in cases:
                inp = SimpleNamespace(node=seeds, input_id=torch.arange(seeds.numel()),
                                      time=None if time is None else time.to(dev))
                out = s.sample_from_nodes(inp, seed=gseed)
                assert _as_dict(out) == want, (gseed, fan, level, time is None)
                assert out.metadata[1] is inp.time
                assert out.node.dtype == dtype


@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_all_neighbours_equals_the_oracle(dev, dtype):
    for gseed in range(3):
        ei, n, nt, et, seeds, st = _tied_graph(gseed + 10)
        for fan in ([-1], [-1, -1], [-1, -1, -1]):
            s = _sampler(ei, n, fan, dev, dtype, node_time=nt)
            assert _as_dict(s.sample_from_nodes(seeds, time=st.to(dev), seed=3)) == \
                _oracle(ei, n, seeds, fan, node_time=nt, seed_time=st)
            s = _sampler(ei, n, fan, dev, dtype, edge_time=et, replace=True)  # -1: no replacement
            assert _as_dict(s.sample_from_nodes(seeds, time=st.to(dev), seed=3)) == \
                _oracle(ei, n, seeds, fan, edge_time=et, seed_time=st)


def _windows(ei, n, node_time, edge_time, out, seed_time):
    """Per sampled edge: is it eligible for its tree; per (hop, frontier position): the window."""
    src = ei[0]
    key = edge_time if edge_time is not None else node_time[src]
    node, batch = out.node.cpu(), out.batch.cpu()
    row, col, edge = out.row.cpu(), out.col.cpu(), out.edge.cpu()
    t_of_edge = seed_time[batch[col]]
    return key, node, batch, row, col, edge, t_of_edge


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('replace', [False, True])
@pytest.mark.parametrize('level', ['node', 'edge'])
def test_bounded_uniform_keeps_the_contract(dev, dtype, replace, level):
    fan = [4, 3]
    for gseed in range(3):
        ei, n, nt, et, seeds, st = _tied_graph(gseed + 20, n=60, m=900, n_times=8)
        kw = dict(node_time=nt) if level == 'node' else dict(edge_time=et)
        s = _sampler(ei, n, fan, dev, dtype, replace=replace, **kw)
        out = s.sample_from_nodes(seeds, time=st.to(dev), seed=gseed)
        nt_, et_ = (nt, None) if level == 'node' else (None, et)
        key, node, batch, row, col, edge, t_e = _windows(ei, n, nt_, et_, out, st)
        assert torch.equal(node[row], ei[0, edge]) and torch.equal(node[col], ei[1, edge])
        assert torch.equal(batch[row], batch[col])
        assert bool((key[edge] <= t_e).all())                   # every sampled edge eligible
        assert torch.equal(node[:seeds.numel()], seeds)
        assert torch.equal(batch[:seeds.numel()], torch.arange(seeds.numel()))
        # per destination: the count rule on the window, no duplicates without replacement
        e0 = 0
        f_lo = 0
        for hop, k in enumerate(fan):
            ne = out.num_sampled_edges[hop]
            n_front = out.num_sampled_nodes[hop]
            c_h, e_h = col[e0:e0 + ne], edge[e0:e0 + ne]
            for fp in range(f_lo, f_lo + n_front):
                v, t = int(node[fp]), int(st[int(batch[fp])])
                w = int(((ei[1] == v) & (key <= t)).sum())
                mine = e_h[c_h == fp]
                want = (k if w > 0 else 0) if replace else min(w, k)
                assert mine.numel() == want, (hop, fp, w)
                if not replace:
                    assert mine.unique().numel() == mine.numel()
            e0 += ne
            f_lo += n_front


def _star(d, n_seeds):
    """Destination 0 with in-edges from 1..d (source u has node time u - 1)."""
    ei = torch.stack([torch.arange(1, d + 1), torch.zeros(d, dtype=torch.long)])
    node_time = torch.cat([torch.zeros(1, dtype=torch.long), torch.arange(d)])
    return ei, d + 1, node_time, torch.zeros(n_seeds, dtype=torch.long)


def _within_sigmas(count, n, p, sig=5.0):
    sd = math.sqrt(max(p * (1 - p), 1e-12) / n)
    return abs(count / n - p) <= sig * sd + 1e-12


@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_marginals_on_the_window(dev, dtype):
    d, B, k, t = 40, 4000, 5, 24          # window = times 0..24 = sources 1..25
    ei, n, nt, seeds = _star(d, B)
    w = t + 1
    st = torch.full((B, ), t, dtype=torch.long, device=dev)
    for replace in (False, True):
        s = _sampler(ei, n, [k], dev, dtype, node_time=nt, replace=replace)
        out = s.sample_from_nodes(seeds, time=st, seed=5)
        srcs = ei[0, out.edge.cpu()]
        assert out.num_sampled_edges == [B * k]
        cnt = torch.bincount(srcs, minlength=n)
        assert int(cnt[w + 1:].sum()) == 0                    # ineligible slots never drawn
        for u in range(1, w + 1):
            if replace:
                assert _within_sigmas(int(cnt[u]), B * k, 1 / w), (u, int(cnt[u]))
            else:
                assert _within_sigmas(int(cnt[u]), B, k / w), (u, int(cnt[u]))
    # 'last' with replacement: k draws among the last k eligible slots only
    s = _sampler(ei, n, [k], dev, dtype, node_time=nt, replace=True, temporal_strategy='last')
    out = s.sample_from_nodes(seeds, time=st, seed=6)
    cnt = torch.bincount(ei[0, out.edge.cpu()], minlength=n)
    assert out.num_sampled_edges == [B * k]
    assert int(cnt[:w - k + 1].sum()) == 0 and int(cnt[w + 1:].sum()) == 0
    for u in range(w - k + 1, w + 1):
        assert _within_sigmas(int(cnt[u]), B * k, 1 / k), (u, int(cnt[u]))
    # 'last' without replacement: exactly the k most recent, every time
    s = _sampler(ei, n, [k], dev, dtype, node_time=nt, temporal_strategy='last')
    out = s.sample_from_nodes(seeds, time=st, seed=7)
    got = ei[0, out.edge.cpu()].view(B, k)
    assert bool((got == torch.arange(w - k + 1, w + 1)).all())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('replace', [False, True])
def test_all_eligible_equals_the_disjoint_sampler_bit_for_bit(dev, dtype, replace):
    from pytorch_geometric_amd.sampler import NeighborSampler
    g = gen(31)
    n, m = 300, 6000
    ei = torch.stack([torch.randint(0, n, (m, ), generator=g),
                      (torch.rand(m, generator=g).pow(3) * n).long()])
    seeds = torch.randint(0, n, (64, ), generator=g)
    fan = [6, 4, -1] if not replace else [6, 4, 2]
    plain = NeighborSampler(ei.to(dtype).to(dev), n, fan, disjoint=True, replace=replace)
    zeros = torch.zeros(n, dtype=torch.long)
    tn = _sampler(ei, n, fan, dev, dtype, node_time=zeros, replace=replace)
    for rng in range(3):
        a = _as_dict(plain.sample_from_nodes(seeds, seed=rng))
        b = _as_dict(tn.sample_from_nodes(seeds, seed=rng))
        assert a == b
    # node-level time and the matching edge-level time give the same batches
    nt = torch.randint(0, 6, (n, ), generator=g)
    et = nt[ei[0]]
    st = torch.randint(-1, 7, (seeds.numel(), ), generator=g).to(dev)
    for strategy in ('uniform', 'last'):
        sn = _sampler(ei, n, fan, dev, dtype, node_time=nt, replace=replace,
                      temporal_strategy=strategy)
        se = _sampler(ei, n, fan, dev, dtype, edge_time=et, replace=replace,
                      temporal_strategy=strategy)
        for rng in range(2):
            assert _as_dict(sn.sample_from_nodes(seeds, time=st, seed=rng)) == \
                _as_dict(se.sample_from_nodes(seeds, time=st, seed=rng))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('level', ['node', 'edge'])
def test_window_search_at_a_hub(dev, dtype, level):
    from pytorch_geometric_amd import _native
    g = gen(41)
    D, n = 200_003, 5000
    # node 0: D in-edges; node 1: 3 in-edges; node 2: none.  Runs of 37 equal times straddle the
    # 64-slot probe boundaries.
    src = torch.cat([torch.randint(3, n, (D, ), generator=g), torch.tensor([4, 5, 6])])
    dst = torch.cat([torch.zeros(D, dtype=torch.long), torch.ones(3, dtype=torch.long)])
    order = torch.randperm(src.numel(), generator=g)
    ei = torch.stack([src, dst])[:, order]
    if level == 'edge':
        et = torch.cat([torch.arange(D) // 37, torch.tensor([2, 0, 5])])[order]
        s = _sampler(ei, n, [-1], dev, dtype, edge_time=et)
        key = et
    else:
        nt = torch.arange(n) // 3
        s = _sampler(ei, n, [-1], dev, dtype, node_time=nt)
        key = nt[ei[0]]
    vals = torch.unique(key)
    probe = torch.unique(torch.cat([vals, vals - 1, vals.min() - 5 + torch.zeros(1).long(),
                                    vals.max() + 5 + torch.zeros(1).long()]))
    P = probe.numel()
    frontier = torch.cat([torch.zeros(P), torch.ones(P), torch.full((P, ), 2)]).to(dtype).to(dev)
    ft = probe.repeat(3).to(dev)
    colptr = s.colptr.cpu().long()
    for strategy, k, replace in (('uniform', -1, False), ('last', 7, False), ('last', 7, True),
                                 ('uniform', 64, False)):
        lo, hi, cnt = _native.sample_temporal_window(
            s.colptr, s.row, s.time, frontier, ft, k, edge_level=level == 'edge',
            replace=replace, last=strategy == 'last')
        lo, hi, cnt = lo.cpu().long(), hi.cpu().long(), cnt.cpu().long()
        for v in range(3):
            a, b = int(colptr[v]), int(colptr[v + 1])
            times = key[(ei[1] == v)].sort().values
            want_hi = a + torch.searchsorted(times, probe, right=True)
            sl = slice(v * P, (v + 1) * P)
            assert torch.equal(hi[sl], want_hi), (v, strategy)
            want_lo = torch.clamp(want_hi - k, min=a) if (strategy == 'last' and k >= 0) \
                else torch.full_like(want_hi, a)
            assert torch.equal(lo[sl], want_lo)
            w = want_hi - want_lo
            want_cnt = torch.where(w > 0, k, 0) if replace else \
                (w if k < 0 else torch.clamp(w, max=k))
            assert torch.equal(cnt[sl], want_cnt)
    # the slots really are time-sorted inside every column (ties in edge_index order)
    perm = s.perm.cpu().long()
    k0 = key[perm[:int(colptr[1])]]
    assert bool((k0[1:] >= k0[:-1]).all())
    same = k0[1:] == k0[:-1]
    assert bool((perm[1:int(colptr[1])][same] > perm[:int(colptr[1]) - 1][same]).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_edge_level_temporal_loader(dev, dtype):
    """test/loader/test_neighbor_loader.py:886-906, restated homogeneously."""
    from pytorch_geometric_amd.loader import NeighborLoader
    ei = torch.tensor([[0, 1, 1, 2, 2, 3, 3, 4], [1, 0, 2, 1, 3, 2, 4, 3]])
    edge_time = torch.arange(ei.size(1))
    x = torch.zeros(5, 2, device=dev)
    loader = NeighborLoader(x, ei.to(dtype).to(dev), [-1, -1], batch_size=1,
                            edge_time=edge_time.to(dev),
                            input_time=torch.tensor([4, 4, 4, 4, 4], device=dev))
    n_batches = 0
    for batch in loader:
        n_batches += 1
        et = edge_time[batch.e_id.cpu()]
        assert et.numel() == batch.edge_index.size(1)
        if et.numel() > 0:
            assert int(et.max()) <= 4
        assert batch.seed_time.cpu().tolist() == [4]
        assert batch.batch is not None
    assert n_batches == 5


@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_karate_invariant(dev, dtype):
    """test/loader/test_neighbor_loader.py:407-420 on a synthetic graph: with descending node
    times, every batch's seed time is >= every sampled node's time."""
    from pytorch_geometric_amd.loader import NeighborLoader
    g = gen(51)
    n = 34
    ei = torch.randint(0, n, (2, 156), generator=g)
    t = torch.arange(n, 0, -1)
    x = torch.zeros(n, 2, device=dev)
    loader = NeighborLoader(x, ei.to(dtype).to(dev), [-1, -1], batch_size=1,
                            node_time=t.to(dev))
    for batch in loader:
        nt = t[batch.n_id.cpu()]
        assert bool((nt[0] >= nt[1:]).all())
        assert int(batch.seed_time) == int(nt[0])


@pytest.mark.parametrize('dtype', DTYPES)
def test_loader_shuffles_input_time_with_the_seeds(dev, dtype):
    from pytorch_geometric_amd.loader import NeighborLoader
    g = gen(61)
    n = 200
    ei = torch.randint(0, n, (2, 3000), generator=g)
    nt = torch.randint(0, 50, (n, ), generator=g)
    input_nodes = torch.randperm(n, generator=g)[:90]
    input_time = torch.randint(0, 60, (90, ), generator=g)
    x = torch.arange(n, dtype=torch.float32, device=dev).unsqueeze(1)
    for prefetch in (0, 2):
        loader = NeighborLoader(x, ei.to(dtype).to(dev), [5, 3], batch_size=16, shuffle=True,
                                input_nodes=input_nodes.to(dev), node_time=nt.to(dev),
                                input_time=input_time.to(dev), seed=3, prefetch=prefetch,
                                temporal_strategy='last')
        seen = []
        for batch in loader:
            bs = batch.batch_size
            ids = batch.input_id.cpu()
            assert torch.equal(batch.n_id[:bs].cpu(), input_nodes[ids].to(batch.n_id.dtype))
            assert torch.equal(batch.seed_time.cpu(), input_time[ids])
            b = batch.batch.cpu().long()
            assert torch.equal(b[:bs], torch.arange(bs))
            # every non-seed node is reached by an edge eligible for its tree's seed time
            e = batch.e_id.cpu()
            src_t = nt[ei[0, e]]
            tree = b[batch.edge_index[1].cpu().long()]
            assert bool((src_t <= input_time[ids][tree]).all())
            seen.append(ids)
        seen = torch.cat(seen)
        assert torch.equal(seen.sort().values, torch.arange(90))
        assert not torch.equal(seen, torch.arange(90))  # shuffled
