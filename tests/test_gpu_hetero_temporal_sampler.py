"""Temporal heterogeneous neighbour sampling on the GPU: ``HeteroNeighborSampler(node_time= /
edge_time=)``, ``HeteroNeighborLoader(..., input_time=)`` and ``backend.neighbor_sampler(
hetero_data, time_attr=...)`` (the reference's ``NeighborLoader(hetero_data, time_attr=...,
input_time=..., temporal_strategy=...)``, sampler/utils.py:114-137, neighbor_sampler.py:438-471).
The deterministic draws (``'last'`` without replacement, ``-1``) are pinned to the plain-Python
restatement in ``tests/_hetero_temporal_ref.py``, order included; bounded draws keep the contract on
the eligible window at scale and are uniform on it; one node type and one edge type give
``NeighborSampler``'s temporal batch bit for bit, constant times the non-temporal disjoint batch.
The RNG is counter-based: every statistical check below is deterministic for its fixed seeds."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests._hetero_temporal_ref import edge_level_loader_graph, hetero_temporal_sample
from tests._util import gen

pytestmark = pytest.mark.gpu

DTYPES = [torch.int64, torch.int32]


def _rand_ei(n_src, n_dst, m, seed, dtype=torch.int64):
    g = gen(seed)
    return torch.stack([torch.randint(0, n_src, (m, ), generator=g),
                        torch.randint(0, n_dst, (m, ), generator=g)]).to(dtype)


def _small_graph(dtype):
    """3 node types that are reached and one empty one, 5 edge types (one without edges); the
    'cites' stack comes first, so every other type's columns start past slot 0."""
    nn = {'paper': 40, 'author': 30, 'venue': 5, 'field': 0}
    eid = {('paper', 'cites', 'paper'): _rand_ei(40, 40, 90, 1, dtype),
           ('author', 'writes', 'paper'): _rand_ei(30, 40, 70, 2, dtype),
           ('paper', 'rev_writes', 'author'): _rand_ei(40, 30, 70, 3, dtype),
           ('venue', 'hosts', 'author'): torch.empty(2, 0, dtype=dtype),
           ('paper', 'in', 'venue'): _rand_ei(40, 5, 20, 4, dtype)}
    return eid, nn


def _scale_graph(dtype):
    """The shape of ``test_gpu_hetero_sampler._scale_graph``: paper 0 is cited 60,000 times."""
    nn = {'paper': 60000, 'author': 80000, 'inst': 2000, 'field': 5000}
    g = gen(21)
    eid = {}
    spec = [('author', 'writes', 'paper', 400000), ('paper', 'rev_writes', 'author', 400000),
            ('paper', 'cites', 'paper', 300000), ('author', 'affil', 'inst', 100000),
            ('field', 'rev_topic', 'paper', 250000), ('paper', 'topic', 'field', 250000)]
    for s, r, d, m in spec:
        src = torch.randint(0, nn[s], (m, ), generator=g)
        dst = torch.randint(0, nn[d], (m, ), generator=g)
        eid[(s, r, d)] = torch.stack([src, dst])
    hub = torch.stack([torch.randint(0, nn['paper'], (60000, ), generator=g),
                       torch.zeros(60000, dtype=torch.long)])
    eid[('paper', 'cites', 'paper')] = torch.cat([eid[('paper', 'cites', 'paper')], hub], 1)
    return {k: v.to(dtype) for k, v in eid.items()}, nn


def _sampler(eid, nn, fan, dev, node_time=None, edge_time=None, **kw):
    from pytorch_geometric_amd.sampler import HeteroNeighborSampler
    mv = (lambda d: None if d is None else {k: v.to(dev) for k, v in d.items()})
    return HeteroNeighborSampler({k: v.to(dev) for k, v in eid.items()}, nn, fan,
                                 node_time=mv(node_time), edge_time=mv(edge_time), **kw)


def _lists(out):
    f = (lambda d: {k: v.long().tolist() for k, v in d.items()})
    return (f(out.node), f(out.row), f(out.col), f(out.edge), f(out.batch),
            out.num_sampled_nodes, out.num_sampled_edges)


WHAT = ('node', 'row', 'col', 'edge', 'batch', 'n_nodes', 'n_edges')


def _assert_equal(out, want, tag=None):
    for g, w, what in zip(_lists(out), want, WHAT):
        assert g == w, (what, tag)


def _max_in_degree(eid):
    return int(max(torch.bincount(v[1].long()).max() if v.numel() else 0 for v in eid.values()))


def _times(eid, nn, seed, n_times=5):
    """Tied times: few distinct values over many nodes / edges."""
    g = gen(seed)
    node_time = {t: torch.randint(0, n_times, (n, ), generator=g) for t, n in nn.items()}
    edge_time = {et: torch.randint(0, n_times, (ei.size(1), ), generator=g)
                 for et, ei in eid.items()}
    return node_time, edge_time


# ---- 1. 'last' without replacement is exact ---------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('level', ['node', 'edge'])
def test_last_without_replacement_equals_restatement(dev, dtype, level):
    eid, nn = _small_graph(dtype)
    ets = list(eid)
    big = _max_in_degree(eid)
    all_nt, all_et = _times(eid, nn, 50)
    if level == 'node':   # authors carry no time: 'writes' is untimed; 'field' is an empty type
        kw = dict(node_time={t: all_nt[t] for t in ('paper', 'venue', 'field')})
        untimed = [ets[1]]
    else:                 # 'rev_writes' and the empty 'hosts' carry no time
        kw = dict(edge_time={et: all_et[et] for et in (ets[0], ets[1], ets[4])})
        untimed = [ets[2], ets[3]]
    fans = [{ets[0]: [2, 1, 3], ets[1]: [1, 2, 0], ets[2]: [1, 3, 2], ets[3]: [2, 2, 2],
             ets[4]: [0, -1, 1]},
            {ets[0]: [-1, 2, 1], ets[1]: [3, 0, -1], ets[2]: [3, -1, 1], ets[3]: [0, 1, -1],
             ets[4]: [1, 1, 0]}]
    # an untimed type draws at random above its fan-out: keep those deterministic (-1, 0, >= deg)
    for fan in fans:
        for et in untimed:
            fan[et] = [k if k <= 0 else big for k in fan[et]]
    seeds = torch.tensor([3, 17, 5, 29, 0, 11, 3])
    st = torch.tensor([-2, 0, 1, 2, 3, 4, 99])   # below all, equal to some, above all times
    for fan in fans:
        smp = _sampler(eid, nn, fan, dev, temporal_strategy='last', seed=3, **kw)
        assert smp.disjoint and smp.is_temporal
        cases = [('paper', seeds, st), ('author', seeds, st), ('venue', torch.tensor([0, 4, 4]),
                                                              torch.tensor([2, 0, 7]))]
        if level == 'node':
            cases.append(('paper', seeds, None))            # node_time['paper'][seeds]
        for input_type, sd, time in cases:
            inp = SimpleNamespace(node=sd, input_id=torch.arange(sd.numel()), input_type=input_type,
                                  time=None if time is None else time.to(dev))
            out = smp.sample_from_nodes(inp)
            want = hetero_temporal_sample(eid, nn, fan, input_type, sd.tolist(), seed_time=time,
                                          strategy='last', **kw)
            _assert_equal(out, want, (input_type, time is None))
            assert all(v.dtype == dtype for v in out.node.values())
            assert all(v.dtype == dtype for v in out.batch.values())
            assert out.metadata[1] is inp.time and torch.equal(out.metadata[0], inp.input_id)
            assert out.node['field'].numel() == 0
            assert out.num_sampled_edges[ets[3]] == [0, 0, 0]
    # a second batch leaves nothing behind
    again = smp.sample_from_nodes(('paper', seeds), time=st)
    _assert_equal(again, hetero_temporal_sample(eid, nn, fan, 'paper', seeds.tolist(),
                                                seed_time=st, strategy='last', **kw))


# ---- 2. 'uniform' with every neighbour is exact -----------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('level', ['node', 'edge'])
def test_uniform_all_neighbours_equals_restatement(dev, dtype, level):
    eid, nn = _small_graph(dtype)
    ets = list(eid)
    all_nt, all_et = _times(eid, nn, 60)
    kw = (dict(node_time={t: all_nt[t] for t in ('paper', 'venue')}) if level == 'node'
          else dict(edge_time={et: all_et[et] for et in ets[:3]}))
    fan = {et: [-1, -1] for et in ets}
    seeds = torch.tensor([3, 17, 5, 29, 0, 11])
    st = torch.tensor([-1, 0, 1, 2, 4, 9])
    for replace in (False, True):      # -1: no replacement either way
        smp = _sampler(eid, nn, [-1, -1], dev, replace=replace, **kw)
        out = smp.sample_from_nodes(('paper', seeds), time=st.to(dev))
        _assert_equal(out, hetero_temporal_sample(eid, nn, fan, 'paper', seeds.tolist(),
                                                  seed_time=st, **kw), replace)
    # bounded fan-outs at least the largest in-degree: every window <= k
    big = _max_in_degree(eid)
    smp = _sampler(eid, nn, [big, big], dev, **kw)
    out = smp.sample_from_nodes(('author', seeds), time=st)
    _assert_equal(out, hetero_temporal_sample(eid, nn, {et: [big, big] for et in ets}, 'author',
                                              seeds.tolist(), seed_time=st, **kw))


# ---- 3. the contract at scale -----------------------------------------------------------------------
def _window_counter(ei, key, n_dst):
    """``f(v, t)`` = number of in-edges of v with key <= t, vectorised: the edges sorted by
    (destination, key), one ``searchsorted`` per query."""
    BIG = 1 << 20
    assert int(key.min()) >= 0 and int(key.max()) < BIG - 2
    comp = (ei[1].long() * BIG + key + 1).sort().values
    start = torch.searchsorted(comp, torch.arange(n_dst) * BIG)

    def count(v, t):
        q = v * BIG + (t + 1).clamp(0, BIG - 1)
        return torch.searchsorted(comp, q, right=True) - start[v]
    return count


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('replace', [False, True])
@pytest.mark.parametrize('level', ['node', 'edge'])
def test_contract_at_scale(dev, dtype, replace, level):
    eid, nn = _scale_graph(dtype)
    ets = list(eid)
    g = gen(70)
    if level == 'node':   # authors and institutions carry no time
        nt = {t: torch.randint(0, 1000, (nn[t], ), generator=g) for t in ('paper', 'field')}
        kw = dict(node_time=nt)
        key = {et: nt[et[0]][eid[et][0].long()] for et in ets if et[0] in nt}
    else:
        key = {et: torch.randint(0, 1000, (eid[et].size(1), ), generator=g)
               for et in (ets[0], ets[1], ets[2], ets[4])}
        kw = dict(edge_time=key)
    assert 0 < len(key) < len(ets)
    fan = {ets[0]: [10, 5], ets[1]: [7, 3], ets[2]: [12, 4], ets[3]: [3, 2], ets[4]: [5, 2],
           ets[5]: [0, 6]}
    smp = _sampler(eid, nn, fan, dev, replace=replace, seed=9, **kw)
    B = 1024
    seeds = torch.cat([torch.tensor([0]), torch.randperm(nn['paper'], generator=gen(3))[:B - 1]])
    st = torch.randint(-5, 1100, (B, ), generator=g)
    out = smp.sample_from_nodes(('paper', seeds), time=st.to(dev))
    node = {t: v.long().cpu() for t, v in out.node.items()}
    batch = {t: v.long().cpu() for t, v in out.batch.items()}
    for t, v in node.items():
        assert sum(out.num_sampled_nodes[t]) == v.numel() == batch[t].numel()
        pairs = batch[t] * 10 ** 6 + v
        assert pairs.unique().numel() == pairs.numel(), t     # unique per (tree, node)
    assert torch.equal(node['paper'][:B], seeds)
    assert torch.equal(batch['paper'][:B], torch.arange(B))
    bounds = {t: [0] + torch.tensor(out.num_sampled_nodes[t]).cumsum(0).tolist() for t in node}
    deg = {et: torch.bincount(eid[et][1].long(), minlength=nn[et[2]]) for et in ets}
    counter = {et: _window_counter(eid[et], key[et], nn[et[2]]) for et in key}
    n_checked = 0
    for et in ets:
        s_t, _, d_t = et
        row, col, edge = (out.row[et].long().cpu(), out.col[et].long().cpu(),
                          out.edge[et].long().cpu())
        assert sum(out.num_sampled_edges[et]) == row.numel() == col.numel() == edge.numel()
        ei = eid[et].long()
        assert torch.equal(node[s_t][row], ei[0, edge])      # maps back through `edge`
        assert torch.equal(node[d_t][col], ei[1, edge])
        assert torch.equal(batch[s_t][row], batch[d_t][col])  # both ends in one tree
        if et in key:                                         # every sampled edge is eligible
            assert bool((key[et][edge] <= st[batch[d_t][col]]).all()), et
        off = 0
        for h, m in enumerate(out.num_sampled_edges[et]):
            c, e = col[off:off + m], edge[off:off + m]
            lo, hi = bounds[d_t][h], bounds[d_t][h + 1]      # nodes of dst added in hop h - 1
            assert bool(((c >= lo) & (c < hi)).all())
            k = fan[et][h]
            v, tree = node[d_t][lo:hi], batch[d_t][lo:hi]
            w = counter[et](v, st[tree]) if et in key else deg[et][v]
            want = (w > 0).long() * k if replace else w.clamp(max=k)
            per = torch.bincount(c - lo, minlength=hi - lo) if m else torch.zeros(
                hi - lo, dtype=torch.long)
            assert torch.equal(per, want), (et, h)
            if not replace:                                   # no repeated slot per destination
                pe = c * (ei.size(1) + 1) + e
                assert pe.unique().numel() == pe.numel()
            assert torch.equal(c, c.sort().values)           # ordered by destination
            n_checked += m
            off += m
    assert n_checked > 10000
    assert out.num_sampled_edges[ets[5]][0] == 0


# ---- 4. uniform over the eligible window, per edge type --------------------------------------------
def _within_sigmas(count, n, p, sig=5.0):
    sd = math.sqrt(max(p * (1 - p), 1e-12) / n)
    return abs(count / n - p) <= sig * sd + 1e-12


@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_marginals_on_the_window_per_edge_type(dev, dtype):
    """Paper 0 has 40 authors (author u at time u) and is cited by papers 1..30 (paper u at time
    u - 1).  With seed time 24 both windows hold 25 sources; k = 5 resp. 3."""
    W, C = ('author', 'writes', 'paper'), ('paper', 'cites', 'paper')
    eid = {W: torch.stack([torch.arange(40), torch.zeros(40, dtype=torch.long)]).to(dtype),
           C: torch.stack([torch.arange(1, 31), torch.zeros(30, dtype=torch.long)]).to(dtype)}
    nn = {'author': 40, 'paper': 31}
    nt = {'author': torch.arange(40), 'paper': torch.cat([torch.zeros(1, dtype=torch.long),
                                                          torch.arange(30)])}
    B, t, w = 4000, 24, 25
    ks = {W: 5, C: 3}
    seeds = torch.zeros(B, dtype=torch.long)
    st = torch.full((B, ), t, dtype=torch.long, device=dev)
    for replace in (False, True):
        smp = _sampler(eid, nn, {W: [5], C: [3]}, dev, node_time=nt, replace=replace, seed=5)
        out = smp.sample_from_nodes(('paper', seeds), time=st)
        for et, k in ks.items():
            assert out.num_sampled_edges[et] == [B * k]
            e = out.edge[et].long().cpu()
            cnt = torch.bincount(e, minlength=eid[et].size(1))
            assert int(cnt[w:].sum()) == 0                    # ineligible slots never drawn
            if not replace:
                per_tree = out.col[et].long().cpu() * 64 + e
                assert per_tree.unique().numel() == per_tree.numel()
            for u in range(w):
                if replace:
                    assert _within_sigmas(int(cnt[u]), B * k, 1 / w), (et, u, int(cnt[u]))
                else:
                    assert _within_sigmas(int(cnt[u]), B, k / w), (et, u, int(cnt[u]))
    # 'last' with replacement: k draws among the last k eligible slots only
    smp = _sampler(eid, nn, {W: [5], C: [3]}, dev, node_time=nt, replace=True,
                   temporal_strategy='last', seed=6)
    out = smp.sample_from_nodes(('paper', seeds), time=st)
    for et, k in ks.items():
        cnt = torch.bincount(out.edge[et].long().cpu(), minlength=eid[et].size(1))
        assert out.num_sampled_edges[et] == [B * k]
        assert int(cnt[:w - k].sum()) == 0 and int(cnt[w:].sum()) == 0
        for u in range(w - k, w):
            assert _within_sigmas(int(cnt[u]), B * k, 1 / k), (et, u, int(cnt[u]))


# ---- 5. one node type and one edge type: NeighborSampler's temporal batch ---------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('level', ['node', 'edge'])
@pytest.mark.parametrize('strategy', ['uniform', 'last'])
@pytest.mark.parametrize('replace', [False, True])
def test_single_type_is_the_homogeneous_temporal_sampler(dev, dtype, level, strategy, replace):
    from pytorch_geometric_amd.sampler import NeighborSampler
    N, E = 3000, 40000
    ei = _rand_ei(N, N, E, 11, dtype).to(dev)
    g = gen(12)
    nt = torch.randint(0, 50, (N, ), generator=g).to(dev)
    etime = torch.randint(-20, 30, (E, ), generator=g).to(dev)
    et = ('n', 'to', 'n')
    for fan in ([5, 3], [-1, 2]):
        if level == 'node':
            hom = NeighborSampler(ei, N, fan, replace=replace, node_time=nt,
                                  temporal_strategy=strategy)
            het = _sampler({et: ei}, {'n': N}, fan, dev, replace=replace, node_time={'n': nt},
                           temporal_strategy=strategy)
        else:
            hom = NeighborSampler(ei, N, fan, replace=replace, edge_time=etime,
                                  temporal_strategy=strategy)
            het = _sampler({et: ei}, {'n': N}, fan, dev, replace=replace, edge_time={et: etime},
                           temporal_strategy=strategy)
        for rng in (0, 7, 123):
            seeds = torch.randperm(N, generator=gen(rng))[:200].to(dev)
            times = [torch.randint(-25, 60, (200, ), generator=gen(rng + 1)).to(dev)]
            if level == 'node':
                times.append(None)
            for time in times:
                a = hom.sample_from_nodes(seeds, seed=rng, time=time)
                b = het.sample_from_nodes(('n', seeds), seed=rng, time=time)
                assert torch.equal(a.node, b.node['n']) and torch.equal(a.batch, b.batch['n'])
                assert torch.equal(a.row, b.row[et]) and torch.equal(a.col, b.col[et])
                assert torch.equal(a.edge, b.edge[et])
                assert a.num_sampled_nodes == b.num_sampled_nodes['n']
                assert a.num_sampled_edges == b.num_sampled_edges[et]
                assert sum(a.num_sampled_edges) > 0


# ---- 6. constant times: the non-temporal disjoint batch ---------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('replace', [False, True])
def test_constant_times_equal_the_disjoint_sampler_bit_for_bit(dev, dtype, replace):
    eid, nn = _scale_graph(dtype)
    ets = list(eid)
    fan = {ets[0]: [6, 3], ets[1]: [4, 2], ets[2]: [5, 4], ets[3]: [3, 1] if replace else [3, -1],
           ets[4]: [2, 2], ets[5]: [0, 3]}
    plain = _sampler(eid, nn, fan, dev, disjoint=True, replace=replace)
    by_node = _sampler(eid, nn, fan, dev, replace=replace,
                       node_time={t: torch.full((n, ), 7, dtype=torch.long)
                                  for t, n in nn.items()})
    by_edge = _sampler(eid, nn, fan, dev, replace=replace,
                       edge_time={et: torch.full((ei.size(1), ), -3, dtype=torch.long)
                                  for et, ei in eid.items()})
    seeds = torch.cat([torch.tensor([0]), torch.randperm(nn['paper'], generator=gen(5))[:255]])
    at, above = torch.full((256, ), 7), torch.full((256, ), 10 ** 12)
    for rng in range(2):
        a = _lists(plain.sample_from_nodes(('paper', seeds), seed=rng))
        assert sum(sum(v) for v in a[6].values()) > 1000
        assert _lists(by_node.sample_from_nodes(('paper', seeds), seed=rng)) == a   # default: 7
        assert _lists(by_node.sample_from_nodes(('paper', seeds), seed=rng, time=above)) == a
        assert _lists(by_edge.sample_from_nodes(('paper', seeds), seed=rng, time=at - 10)) == a
        assert _lists(by_edge.sample_from_nodes(('paper', seeds), seed=rng, time=above)) == a
    # one tick below the constant: nothing is eligible
    out = by_node.sample_from_nodes(('paper', seeds), time=at - 1)
    assert all(sum(v) == 0 for v in out.num_sampled_edges.values())


# ---- 7. the window search at a hub ------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('level', ['node', 'edge'])
def test_window_search_at_a_hub(dev, dtype, level):
    """Paper 0 has more than 64^2 in-edges on 'cites', the third edge type of the stack, so its
    column starts far from slot 0 and the search takes three rounds.  Seed times cut the column
    at ranks 0, 1, 63, 64, 65, 4095, 4096, 4097, the middle, D - 1 and D."""
    eid, nn = _scale_graph(dtype)
    ets = list(eid)
    cites = ('paper', 'cites', 'paper')
    assert ets.index(cites) == 2
    ei = eid[cites].long()
    g = gen(80)
    if level == 'node':    # distinct node times; equal sources of the hub still tie
        nt = {'paper': torch.randperm(nn['paper'], generator=g) * 3}
        kw = dict(node_time=nt)
        key = nt['paper'][ei[0]]
    else:
        key = torch.randperm(ei.size(1), generator=g) * 3 - 1000
        kw = dict(edge_time={cites: key})
    hub_e = (ei[1] == 0).nonzero().view(-1)
    D = hub_e.numel()
    assert D > 64 * 64
    order = hub_e[torch.argsort(key[hub_e] * (ei.size(1) + 1) + hub_e)]   # (time, position)
    hk = key[order]
    cuts = [0, 1, 63, 64, 65, 4095, 4096, 4097, D // 2, D - 1, D]
    # a time that admits exactly the first r slots: just below slot r's time (ties move the rank
    # to the end of the run, so the expected rank is recomputed from the times)
    st = torch.tensor([int(hk[r]) - 1 if r < D else int(hk[-1]) + 5 for r in cuts])
    ranks = [int((hk <= t).sum()) for t in st.tolist()]
    assert ranks[0] == 0 and ranks[-1] == D and len(set(ranks)) >= 9
    seeds = torch.zeros(len(cuts), dtype=torch.long)
    fan = {et: [0] for et in ets}
    fan[cites] = [-1]
    out = _sampler(eid, nn, fan, dev, **kw).sample_from_nodes(('paper', seeds), time=st)
    assert out.num_sampled_edges[cites] == [sum(ranks)]
    col, edge = out.col[cites].long().cpu(), out.edge[cites].long().cpu()
    for i, r in enumerate(ranks):
        assert torch.equal(edge[col == i], order[:r]), (i, r)
    # 'last', k = 7: exactly the 7 most recent eligible in-edges
    fan[cites] = [7]
    out = _sampler(eid, nn, fan, dev, temporal_strategy='last', **kw).sample_from_nodes(
        ('paper', seeds), time=st)
    col, edge = out.col[cites].long().cpu(), out.edge[cites].long().cpu()
    for i, r in enumerate(ranks):
        assert torch.equal(edge[col == i], order[max(0, r - 7):r]), (i, r)
    # 'uniform', k = 7: 7 distinct slots of the window
    out = _sampler(eid, nn, fan, dev, seed=1, **kw).sample_from_nodes(('paper', seeds), time=st)
    col, edge = out.col[cites].long().cpu(), out.edge[cites].long().cpu()
    for i, r in enumerate(ranks):
        mine = edge[col == i]
        assert mine.numel() == min(r, 7) and mine.unique().numel() == mine.numel()
        assert bool((key[mine] <= st[i]).all()) and bool((ei[1, mine] == 0).all())


# ---- 8. the reference's two loader tests ------------------------------------------------------------
def _karate_like():
    """A small undirected graph in place of the reference's karate club (34 nodes)."""
    ei = _rand_ei(34, 34, 78, 90)
    return torch.cat([ei, ei.flip(0)], 1)


def test_reference_temporal_hetero_loader_node_level(dev):
    """test_temporal_hetero_neighbor_loader_on_karate: time = arange(N, 0, -1), [-1, -1], batch
    size 1: no sampled node is newer than the seed."""
    from pytorch_geometric_amd.loader import HeteroNeighborLoader
    ei, N = _karate_like(), 34
    time = torch.arange(N, 0, -1)
    x = {'v': torch.randn(N, 3, generator=gen(1)).to(dev)}
    loader = HeteroNeighborLoader(x, {('v', 'to', 'v'): ei.to(dev)}, [-1, -1], input_nodes='v',
                                  batch_size=1, node_time={'v': time.to(dev)})
    n_more = 0
    for batch in loader:
        t = time[batch.n_id['v'].cpu()]
        assert bool((t[0] >= t[1:]).all())
        assert batch.seed_time.tolist() == [int(t[0])]
        assert batch.batch['v'].eq(0).all()
        n_more += t.numel() > 1
    assert len(loader) == N and n_more > N // 2


def test_reference_temporal_hetero_loader_edge_level(dev):
    """test_edge_level_temporal_hetero_neighbor_loader: every batch's edge times are <= 4."""
    from pytorch_geometric_amd.loader import HeteroNeighborLoader
    eid, nn, etime = edge_level_loader_graph()
    (et, ei), = eid.items()
    x = {'A': torch.zeros(5, 2, device=dev)}
    with pytest.raises(ValueError, match='needs the seed times'):
        HeteroNeighborLoader(x, {et: ei.to(dev)}, [-1, -1], input_nodes='A', batch_size=1,
                             edge_time={et: etime[et].to(dev)})
    loader = HeteroNeighborLoader(x, {et: ei.to(dev)}, [-1, -1], input_nodes='A', batch_size=1,
                                  edge_time={et: etime[et].to(dev)},
                                  input_time=torch.tensor([4, 4, 4, 4, 4]))
    n_edges = []
    for seed, batch in enumerate(loader):
        e = batch.e_id[et].cpu()
        assert e.numel() == batch.edge_index_dict[et].size(1)
        if e.numel() > 0:
            assert int(etime[et][e].max()) <= 4
        assert batch.seed_time.tolist() == [4]
        want = hetero_temporal_sample(eid, nn, {et: [-1, -1]}, 'A', [seed], edge_time=etime,
                                      seed_time=[4])
        assert batch.n_id['A'].tolist() == want[0]['A'] and e.tolist() == want[3][et]
        n_edges.append(e.numel())
    assert n_edges[2] == 3 and n_edges[4] == 0


def _import_reference():
    try:
        from oracle import make_ref
        make_ref.import_reference()
        import torch_geometric  # noqa: F401
    except ImportError:
        pytest.skip('torch_geometric cannot be imported')


def test_reference_node_loader_runs_both_cases_on_the_adapter(dev):
    _import_reference()
    from torch_geometric.data import HeteroData
    from torch_geometric.loader import NodeLoader
    from pytorch_geometric_amd import backend
    # node level
    data = HeteroData()
    data['v'].x = torch.randn(34, 3, generator=gen(1))
    data['v'].time = torch.arange(34, 0, -1)
    data['v', 'v'].edge_index = _karate_like()
    data = data.to(dev)
    smp = backend.neighbor_sampler(data, [-1, -1], time_attr='time')
    assert smp.is_temporal and smp.disjoint and set(smp.node_time) == {'v'}
    n = 0
    for batch in NodeLoader(data, node_sampler=smp, input_nodes='v', batch_size=1):
        assert bool((batch['v'].time[0] >= batch['v'].time[1:]).all())
        assert bool((batch['v'].time == data['v'].time[batch['v'].n_id]).all())
        n += 1
    assert n == 34
    # edge level
    eid, nn, etime = edge_level_loader_graph()
    (et, ei), = eid.items()
    data = HeteroData()
    data['A'].num_nodes = 5
    data['A', 'A'].edge_index = ei
    data['A', 'A'].edge_time = etime[et]
    data = data.to(dev)
    smp = backend.neighbor_sampler(data, [-1, -1], time_attr='edge_time')
    assert smp.is_temporal and set(smp.edge_time) == {et}
    loader = NodeLoader(data, node_sampler=smp, input_nodes='A', batch_size=1,
                        input_time=torch.tensor([4, 4, 4, 4, 4]))
    sizes = []
    for batch in loader:
        assert batch['A', 'A'].edge_time.numel() == batch['A', 'A'].num_edges
        if batch['A', 'A'].edge_time.numel() > 0:
            assert int(batch['A', 'A'].edge_time.max()) <= 4
        assert batch['A'].seed_time.tolist() == [4]
        sizes.append(batch['A', 'A'].num_edges)
    assert sizes[2] == 3 and sizes[4] == 0
    # without input_time an edge-level sampler has no default
    with pytest.raises(ValueError, match='needs the seed times'):
        next(iter(NodeLoader(data, node_sampler=smp, input_nodes='A', batch_size=1)))


# ---- 9. the loader shuffles input_time with the seeds ----------------------------------------------
@pytest.mark.parametrize('level', ['node', 'edge'])
def test_loader_shuffles_input_time_with_the_seeds(dev, level):
    from pytorch_geometric_amd.loader import HeteroNeighborLoader
    eid, nn = _small_graph(torch.int64)
    all_nt, all_et = _times(eid, nn, 95)
    kw = (dict(node_time={'paper': all_nt['paper'].to(dev)}) if level == 'node'
          else dict(edge_time={et: t.to(dev) for et, t in all_et.items()}))
    x = {t: torch.randn(n, 4, generator=gen(2)).to(dev) for t, n in nn.items()}
    nodes = torch.arange(1, 40, 2)
    input_time = nodes * 10 + 3                       # tells which seed a time belongs to
    eid = {k: v.to(dev) for k, v in eid.items()}
    common = dict(input_nodes=('paper', nodes), batch_size=6, shuffle=True, seed=4,
                  input_time=input_time, **kw)
    a = list(HeteroNeighborLoader(x, eid, [3, 2], prefetch=0, **common))
    b = list(HeteroNeighborLoader(x, eid, [3, 2], prefetch=2, **common))
    assert len(a) == len(b) == 4
    seen = []
    for p, q in zip(a, b):
        bs = p.batch_size
        seeds = p.n_id['paper'][:bs].cpu()
        assert torch.equal(p.seed_time.cpu(), seeds * 10 + 3)
        assert torch.equal(p.seed_time.cpu(), input_time[p.input_id.cpu()])
        assert torch.equal(nodes[p.input_id.cpu()], seeds)
        assert p.seed_time.dtype == torch.int64 and p.seed_time.is_cuda
        assert torch.equal(p.seed_time, q.seed_time)
        for t in nn:
            assert torch.equal(p.n_id[t], q.n_id[t]) and torch.equal(p.batch[t], q.batch[t])
        seen += seeds.tolist()
    assert sorted(seen) == nodes.tolist() and seen != nodes.tolist()   # shuffled, each once
    if level == 'node':   # without input_time the seeds' own times are used
        loader = HeteroNeighborLoader(x, eid, [3, 2], input_nodes=('paper', nodes), batch_size=6,
                                      **kw)
        batch = next(iter(loader))
        assert torch.equal(batch.seed_time.cpu(), all_nt['paper'][nodes[:6]])
