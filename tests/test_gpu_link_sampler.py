"""Link-level sampling on the GPU: ``NeighborSampler.sample_from_edges`` and ``LinkNeighborLoader``,
the reference's ``edge_sample`` / ``neg_sample`` (sampler/neighbor_sampler.py:821-1096),
``NegativeSampling`` (sampler/base.py:840-929) and ``LinkLoader`` (loader/link_loader.py:155-192,
264-279).  The layouts are checked against the formulas of ``edge_sample`` given the negatives the
batch contains; the sampled subgraph against ``sample_from_nodes`` on the same seed vector; the
negatives' distributions against their marginals; the unique step against ``torch.unique``; and
the reference's own loader tests (test/loader/test_link_neighbor_loader.py) are restated.  The RNG
is counter-based: every statistical check below is deterministic for its fixed seeds."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests._util import gen

pytestmark = pytest.mark.gpu

DTYPES = [torch.int64, torch.int32]


def _graph(n, m, seed):
    g = gen(seed)
    return torch.randint(0, n, (2, m), generator=g)


def _sampler(ei, n, fan, dev, dtype=torch.int64, **kw):
    from pytorch_geometric_amd.sampler import NeighborSampler
    kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    return NeighborSampler(ei.to(dtype).to(dev), n, fan, **kw)


def _same_subgraph(a, b, B=None):
    assert torch.equal(a.node, b.node)
    assert torch.equal(a.row, b.row) and torch.equal(a.col, b.col)
    assert torch.equal(a.edge, b.edge)
    assert a.num_sampled_nodes == b.num_sampled_nodes
    assert a.num_sampled_edges == b.num_sampled_edges
    if B is not None:
        assert torch.equal(a.batch, b.batch % B)


# ---- layout ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('disjoint', [False, True])
@pytest.mark.parametrize('mode,amount', [('binary', 1), ('binary', 2), ('binary', 0.5),
                                         ('triplet', 1), ('triplet', 2)])
def test_layout(dev, dtype, disjoint, mode, amount):
    from pytorch_geometric_amd.sampler import NegativeSampling
    N, B = 300, 40
    ei = _graph(N, 3000, 1)
    smp = _sampler(ei, N, [3, 2], dev, dtype, disjoint=disjoint)
    pos = ei[:, torch.randperm(ei.size(1), generator=gen(2))[:B]].to(dev)
    out = smp.sample_from_edges(pos, NegativeSampling(mode, amount), seed=7)
    n_id = out.node.long()
    n0 = out.num_sampled_nodes[0]
    num_neg = math.ceil(B * amount)
    assert out.node.dtype == dtype
    if mode == 'binary':
        input_id, eli, label, src_time = out.metadata
        assert input_id is None and src_time is None
        assert eli.shape == (2, B + num_neg)
        pairs = n_id[eli]
        assert torch.equal(pairs[:, :B], pos)
        src_all, dst_all = pairs[0], pairs[1]
        assert torch.equal(label, torch.cat([torch.ones(B), torch.zeros(num_neg)]).to(dev))
        assert label.dtype == torch.float32
        if disjoint:
            assert torch.equal(eli, torch.arange(2 * (B + num_neg), device=dev).view(2, -1))
    else:
        input_id, src_index, dst_pos_index, dst_neg_index, src_time = out.metadata
        assert dst_neg_index.shape == ((B, ) if amount == 1 else (B, amount))
        assert torch.equal(n_id[src_index], pos[0])
        assert torch.equal(n_id[dst_pos_index], pos[1])
        if disjoint:
            assert torch.equal(src_index, torch.arange(B, device=dev))
            assert torch.equal(dst_pos_index, torch.arange(B, 2 * B, device=dev))
            flat = torch.arange(2 * B, 2 * B + num_neg, device=dev)
            assert torch.equal(dst_neg_index, flat.view(-1, B).t().reshape(B, -1).squeeze(-1))
            neg = n_id[flat]
        else:
            neg = n_id[dst_neg_index].reshape(-1)   # row-major: negative j at [j // amount]
        src_all, dst_all = pos[0], torch.cat([pos[1], neg])
    seed_vec = torch.cat([src_all, dst_all])
    assert bool((seed_vec >= 0).all() and (seed_vec < N).all())
    if disjoint:
        assert n0 == seed_vec.numel()
        assert torch.equal(n_id[:n0], seed_vec)
        assert torch.equal(out.batch[:n0].long(), torch.arange(n0, device=dev) % B)
        assert int(out.batch.max()) < B
    else:
        assert torch.equal(n_id[:n0], torch.unique(seed_vec))
        if mode == 'triplet':
            inv = torch.unique(seed_vec, return_inverse=True)[1]
            assert torch.equal(src_index, inv[:B]) and torch.equal(dst_pos_index, inv[B:2 * B])
            assert torch.equal(dst_neg_index, inv[2 * B:].view(B, -1).squeeze(-1))


@pytest.mark.parametrize('dtype', DTYPES)
def test_no_negatives_and_edge_sampler_input(dev, dtype):
    N, B = 200, 25
    ei = _graph(N, 1500, 3)
    smp = _sampler(ei, N, [4, 2], dev, dtype)
    pos = ei[:, :B]
    label = torch.arange(B) % 3
    inp = SimpleNamespace(row=pos[0], col=pos[1], label=label, time=None,
                          input_id=torch.arange(B), input_type=None)
    out = smp.sample_from_edges(inp, seed=4)
    input_id, eli, lab, src_time = out.metadata
    assert torch.equal(input_id, torch.arange(B)) and src_time is None
    assert torch.equal(lab.cpu(), label)                     # kept as given: no shift, no zeros
    assert torch.equal(out.node.long()[eli].cpu(), pos)
    with pytest.raises(NotImplementedError):
        smp.sample_from_edges(SimpleNamespace(row=pos[0], col=pos[1], input_type=('a', 'b', 'a')))
    with pytest.raises(ValueError, match="not temporal"):
        smp.sample_from_edges(SimpleNamespace(row=pos[0], col=pos[1], time=torch.arange(B)))
    with pytest.raises(ValueError, match="undefined for 'triplet'"):
        smp.sample_from_edges(inp, 'triplet')


# ---- equivalence with sample_from_nodes -------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind,disjoint', [('uniform', False), ('uniform', True),
                                           ('weighted', False), ('weighted', True),
                                           ('temporal', True)])   # (temporal is disjoint)
def test_subgraph_equals_sample_from_nodes(dev, dtype, kind, disjoint):
    N, B = 400, 32
    ei = _graph(N, 5000, 5)
    g = gen(6)
    kw = {}
    time = None
    if kind == 'weighted':
        kw['edge_weight'] = torch.rand(ei.size(1), generator=g)
    if kind == 'temporal':
        node_time = torch.randint(0, 50, (N, ), generator=g)
        kw['node_time'] = node_time
    smp = _sampler(ei, N, [5, 3], dev, dtype, disjoint=disjoint, **kw)
    pos = ei[:, torch.randperm(ei.size(1), generator=g)[:B]]
    if kind == 'temporal':
        time = torch.maximum(node_time[pos[0]], node_time[pos[1]]) + 10
    inp = SimpleNamespace(row=pos[0], col=pos[1], label=None, time=time, input_id=None)
    for neg in (None, dict(mode='binary', amount=1), dict(mode='triplet', amount=2)):
        out = smp.sample_from_edges(inp, neg, seed=11)
        n0 = out.num_sampled_nodes[0]
        seeds = out.node[:n0]
        seed_time = None
        if kind == 'temporal':
            st = out.metadata[-1].to(dev)                  # src_time
            if neg is not None and neg['mode'] == 'triplet':
                seed_time = torch.cat([st, st.repeat(1 + neg['amount'])])
            else:
                seed_time = torch.cat([st, st])
            assert seed_time.numel() == n0
        ref = smp.sample_from_nodes(seeds, seed=11, time=seed_time)
        _same_subgraph(out, ref, B if disjoint else None)


# ---- negatives --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_negatives_marginals(dev, dtype):
    from pytorch_geometric_amd import _native
    N, n = 97, 200_000
    out = _native.sample_negatives(n, N, 123, dev, dtype)
    assert out.dtype == dtype and out.numel() == n
    c = torch.bincount(out.long().cpu(), minlength=N)
    assert c.numel() == N
    p = 1 / N
    sigma = math.sqrt(n * p * (1 - p))
    assert float((c - n * p).abs().max()) <= 5 * sigma


@pytest.mark.parametrize('dtype', DTYPES)
def test_weighted_negatives_are_proportional(dev, dtype):
    from pytorch_geometric_amd import _native
    N, n = 60, 300_000
    w = (torch.arange(N) % 7).double()        # every 7th node has weight 0, node 0 included
    w[N - 1] = 0.0                            # the last one as well
    cdf = torch.cumsum(w, 0).to(dev)
    out = _native.sample_negatives(n, N, 9, dev, dtype, cdf=cdf).long().cpu()
    c = torch.bincount(out, minlength=N)
    assert int(c[w == 0].sum()) == 0
    p = w / w.sum()
    sigma = (n * p * (1 - p)).sqrt()
    assert bool(((c - n * p).abs() <= 5 * sigma + 1e-9).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_temporal_negatives_respect_the_bound(dev, dtype):
    from pytorch_geometric_amd import _native
    N, B = 500, 64
    g = gen(8)
    node_time = torch.randint(0, 100, (N, ), generator=g)
    bound = torch.randint(0, 100, (B, ), generator=g)
    fb = int(node_time.argmin())
    out = _native.sample_negatives(3 * B + 5, N, 17, dev, dtype, node_time=node_time.to(dev),
                                   bound=bound.to(dev), fallback=fb).long().cpu()
    j = torch.arange(out.numel())
    ok = (node_time[out] <= bound[j % B]) | (out == fb)
    assert bool(ok.all())
    # a bound below every node time: nothing is eligible, every draw is the fallback
    out = _native.sample_negatives(1000, N, 17, dev, dtype, node_time=node_time.to(dev),
                                   bound=torch.full((B, ), -1, device=dev), fallback=fb)
    assert bool((out == fb).all())
    # the weighted candidates go through the same test
    cdf = torch.cumsum(torch.rand(N, generator=g).double(), 0).to(dev)
    out = _native.sample_negatives(2000, N, 3, dev, dtype, cdf=cdf, node_time=node_time.to(dev),
                                   bound=bound.to(dev), fallback=fb).long().cpu()
    j = torch.arange(out.numel())
    assert bool(((node_time[out] <= bound[j % B]) | (out == fb)).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_temporal_negatives_in_the_sampler(dev, dtype):
    """Negatives of a node-level temporal sampler have node_time <= the time of their positive
    edge, or are the earliest node (smallest id among ties)."""
    N, B = 300, 50
    ei = _graph(N, 2000, 12)
    g = gen(13)
    node_time = torch.randint(5, 80, (N, ), generator=g)
    node_time[[17, 40]] = 1                                   # the earliest: 17 is the fallback
    smp = _sampler(ei, N, [2], dev, dtype, node_time=node_time)
    pos = ei[:, :B]
    t = torch.randint(0, 40, (B, ), generator=g)
    t[:5] = 0                                                 # no node is eligible there
    out = smp.sample_from_edges(SimpleNamespace(row=pos[0], col=pos[1], time=t), 'binary')
    eli = out.metadata[1]
    neg = out.node.long()[eli[:, B:]].cpu()
    ok = (node_time[neg] <= t) | (neg == 17)
    assert bool(ok.all())
    assert bool((neg[:, :5] == 17).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_negatives_reproducible_and_fresh(dev, dtype):
    from pytorch_geometric_amd import _native
    a = _native.sample_negatives(5000, 1000, 42, dev, dtype)
    assert torch.equal(a, _native.sample_negatives(5000, 1000, 42, dev, dtype))
    assert not torch.equal(a, _native.sample_negatives(5000, 1000, 43, dev, dtype))
    bump = torch.ones(1, dtype=torch.int64, device=dev)
    assert not torch.equal(a, _native.sample_negatives(5000, 1000, 42, dev, dtype, seed_dev=bump))
    N, B = 1000, 200
    ei = _graph(N, 4000, 14)
    smp = _sampler(ei, N, [2], dev, dtype, seed=3)
    pos = ei[:, :B]
    negs = []
    for _ in range(2):
        out = smp.sample_from_edges(pos, 'binary')
        negs.append(out.node.long()[out.metadata[1][:, B:]])
    assert not torch.equal(negs[0], negs[1])                  # successive calls: fresh draws
    smp2 = _sampler(ei, N, [2], dev, dtype, seed=3)
    out = smp2.sample_from_edges(pos, 'binary')
    assert torch.equal(out.node.long()[out.metadata[1][:, B:]], negs[0])   # same seed, same batch


@pytest.mark.parametrize('dtype', DTYPES)
def test_weighted_negatives_in_the_sampler(dev, dtype):
    from pytorch_geometric_amd.sampler import NegativeSampling
    N, B = 120, 400
    ei = _graph(N, 1000, 15)
    smp = _sampler(ei, N, [2], dev, dtype)
    sw = torch.zeros(N)
    sw[:10] = 1.0
    dw = torch.zeros(N, device=dev)
    dw[100:] = 3.0
    ns = NegativeSampling('binary', 2, src_weight=sw, dst_weight=dw)
    out = smp.sample_from_edges(ei[:, :B], ns)
    neg = out.node.long()[out.metadata[1][:, B:]]
    assert bool((neg[0] < 10).all()) and bool((neg[1] >= 100).all())
    assert len(smp._neg_cdf) == 2
    smp.sample_from_edges(ei[:, :B], ns)
    assert len(smp._neg_cdf) == 2                             # the CDFs are cached
    with pytest.raises(ValueError, match='positive sum'):
        smp.sample_from_edges(ei[:, :B], NegativeSampling('binary', 1, src_weight=torch.zeros(N)))


# ---- unique -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,N', [(4096, 1000), (1_200_000, 500_000), (1, 7)])
def test_unique_inverse_equals_torch_unique(dev, dtype, n, N):
    from pytorch_geometric_amd import _native
    keys = torch.randint(0, N, (n, ), generator=gen(n)).to(dtype).to(dev)
    uniq, inv = _native.unique_inverse(keys, max_value=N - 1)
    ref_u, ref_i = torch.unique(keys, return_inverse=True)
    assert uniq.dtype == keys.dtype and inv.dtype == torch.int64
    assert torch.equal(uniq, ref_u) and torch.equal(inv, ref_i)


# ---- the reference's loader tests (test/loader/test_link_neighbor_loader.py), homogeneous ---------
def _pairs(ei):
    return set(map(tuple, ei.t().tolist()))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('subgraph_type', ['directional', 'bidirectional'])
@pytest.mark.parametrize('neg_sampling_ratio', [None, 1.0])
def test_reference_basic(dev, dtype, subgraph_type, neg_sampling_ratio):
    """test_homo_link_neighbor_loader_basic (lines 25-108)."""
    from pytorch_geometric_amd.loader import LinkNeighborLoader
    g = gen(25)
    pos_edge_index = torch.randint(0, 50, (2, 500), generator=g)
    neg_edge_index = torch.randint(0, 50, (2, 500), generator=g) + 50
    input_edges = torch.cat([pos_edge_index, neg_edge_index], dim=-1)
    edge_label = torch.cat([torch.ones(500), torch.zeros(500)])
    x = torch.arange(100, dtype=torch.float32).view(-1, 1).to(dev)
    loader = LinkNeighborLoader(
        x, pos_edge_index.to(dtype).to(dev), [-1] * 2, batch_size=20,
        edge_label_index=input_edges.to(dev),
        edge_label=edge_label.to(dev) if neg_sampling_ratio is None else None,
        subgraph_type=subgraph_type, neg_sampling_ratio=neg_sampling_ratio, shuffle=True)
    assert len(loader) == 1000 / 20
    inputs = _pairs(input_edges)
    for batch in loader:
        n = batch.n_id.numel()
        assert batch.x.size(0) == n and batch.x.min() >= 0 and batch.x.max() < 100
        assert batch.e_id.numel() == batch.edge_index.size(1)
        assert batch.input_id.numel() == 20
        if batch.edge_index.numel():
            assert batch.edge_index.min() >= 0 and batch.edge_index.max() < n
            assert batch.e_id.min() >= 0 and batch.e_id.max() < 500
        edge_index = _pairs(batch.edge_index.cpu())
        eli, lab = batch.edge_label_index.cpu(), batch.edge_label.cpu()
        if neg_sampling_ratio is None:
            assert eli.size(1) == 20
            assert _pairs(eli[:, lab == 1]) <= edge_index      # positives are in the subgraph
            assert not (_pairs(eli[:, lab == 0]) & edge_index)  # negatives are not
        else:
            assert eli.size(1) == 40
            assert bool((lab[:20] == 1).all()) and bool((lab[20:] == 0).all())
        glob = _pairs(batch.n_id.long().cpu()[eli][:, lab >= 1])
        assert glob <= inputs


@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_edge_label(dev, dtype):
    """test_link_neighbor_loader_edge_label (lines 187-214)."""
    from pytorch_geometric_amd.loader import LinkNeighborLoader
    ei = torch.randint(0, 100, (2, 500), generator=gen(187)).to(dtype).to(dev)
    x = torch.arange(100, dtype=torch.float32).view(-1, 1).to(dev)
    for batch in LinkNeighborLoader(x, ei, [-1] * 2, batch_size=10, neg_sampling_ratio=1.0):
        assert batch.edge_label.dtype == torch.float
        assert bool((batch.edge_label[:10] == 1.0).all())
        assert bool((batch.edge_label[10:] == 0.0).all())
    loader = LinkNeighborLoader(x, ei, [-1] * 2, batch_size=10,
                                edge_label=torch.ones(500, dtype=torch.long, device=dev),
                                neg_sampling_ratio=1.0)
    for batch in loader:
        assert batch.edge_label.dtype == torch.long
        assert bool((batch.edge_label[:10] == 1).all())
        assert bool((batch.edge_label[10:] == 0).all())
    # labels whose minimum is 0 are shifted by +1 under binary negatives (link_loader.py:172-175)
    lab = torch.arange(500, device=dev) % 2
    loader = LinkNeighborLoader(x, ei, [2], batch_size=50, edge_label=lab, neg_sampling_ratio=0.5)
    batch = next(iter(loader))
    assert torch.equal(batch.edge_label[:50], lab[:50] + 1)
    assert bool((batch.edge_label[50:] == 0).all()) and batch.edge_label.numel() == 75


@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_temporal_homo(dev, dtype):
    """test_temporal_homo_link_neighbor_loader (lines 219-246)."""
    from pytorch_geometric_amd.loader import LinkNeighborLoader
    g = gen(219)
    x = torch.randn(10, 5, generator=g).to(dev)
    ei = torch.randint(0, 10, (2, 123), generator=g)
    time = torch.arange(10)
    edge_label_time = torch.max(time[ei[0]], time[ei[1]])
    loader = LinkNeighborLoader(x, ei.to(dtype).to(dev), [-1], node_time=time.to(dev),
                                edge_label=torch.ones(123, device=dev),
                                edge_label_time=edge_label_time.to(dev), batch_size=1,
                                shuffle=True)
    for batch in loader:
        assert batch.edge_label_index.size() == (2, 1)
        assert batch.edge_label_time.size() == (1, )
        assert batch.edge_label.size() == (1, )
        assert bool((time.to(dev)[batch.n_id.long()] <= batch.edge_label_time).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_no_edges(dev, dtype):
    """test_homo_link_neighbor_loader_no_edges (lines 363-375)."""
    from pytorch_geometric_amd.loader import LinkNeighborLoader
    x = torch.zeros(100, 1, device=dev)
    ei = torch.empty(2, 0, dtype=dtype, device=dev)
    eli = torch.randint(0, 100, (2, 100), generator=gen(363)).to(dev)
    for batch in LinkNeighborLoader(x, ei, [], batch_size=20, edge_label_index=eli):
        assert batch.input_id.numel() == 20
        assert batch.edge_label_index.size(1) == 20
        assert batch.n_id.numel() == batch.edge_label_index.unique().numel()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('disjoint', [False, True])
@pytest.mark.parametrize('temporal', [False, True])
@pytest.mark.parametrize('amount', [1, 2])
def test_reference_triplet(dev, dtype, disjoint, temporal, amount):
    """test_homo_link_neighbor_loader_triplet (lines 402-478)."""
    from pytorch_geometric_amd.loader import LinkNeighborLoader
    if not disjoint and temporal:
        return
    g = gen(402)
    x = torch.arange(100, dtype=torch.float32).view(-1, 1).to(dev)
    ei = torch.randint(0, 100, (2, 400), generator=g)
    eli = torch.randint(0, 100, (2, 500), generator=g)
    node_time = edge_label_time = None
    if temporal:
        node_time = torch.arange(100)
        edge_label_time = torch.max(node_time[eli[0]], node_time[eli[1]]) + 50
        node_time, edge_label_time = node_time.to(dev), edge_label_time.to(dev)
    batch_size = 20
    loader = LinkNeighborLoader(x, ei.to(dtype).to(dev), [-1] * 2, batch_size=batch_size,
                                edge_label_index=eli.to(dev), edge_label_time=edge_label_time,
                                node_time=node_time, disjoint=disjoint,
                                neg_sampling=dict(mode='triplet', amount=amount), shuffle=True)
    assert len(loader) == 500 / batch_size
    eli = eli.to(dev)
    for batch in loader:
        bx = batch.x.view(-1).long()
        assert torch.equal(bx[batch.src_index], eli[0, batch.input_id])
        assert torch.equal(bx[batch.dst_pos_index], eli[1, batch.input_id])
        if amount == 1:
            assert batch.dst_neg_index.size() == (batch_size, )
        else:
            assert batch.dst_neg_index.size() == (batch_size, amount)
        n = batch.n_id.numel()
        assert batch.dst_neg_index.min() >= 0 and batch.dst_neg_index.max() < n
        if disjoint:
            assert batch.src_index.min() == 0 and batch.src_index.max() == batch_size - 1
            assert batch.dst_pos_index.min() == batch_size
            assert batch.dst_pos_index.max() == 2 * batch_size - 1
            assert batch.dst_neg_index.min() == 2 * batch_size
            max_seed_nodes = 2 * batch_size + batch_size * amount
            assert batch.dst_neg_index.max() == max_seed_nodes - 1
            assert batch.batch.min() == 0 and batch.batch.max() == batch_size - 1
            for i in range(0, max_seed_nodes, batch_size):
                assert torch.equal(batch.batch[i:i + batch_size].long(),
                                   torch.arange(batch_size, device=dev))
        if temporal:
            t = node_time[batch.n_id.long()]
            for i in range(batch_size):
                assert t[batch.batch == i].max() <= batch.seed_time[i]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('prefetch', [0, 2])
def test_reference_mapping(dev, dtype, prefetch):
    """test_link_neighbor_loader_mapping (lines 583-603); with the prefetch thread as well."""
    from pytorch_geometric_amd.loader import LinkNeighborLoader
    edge_index = torch.tensor([[0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 5],
                               [1, 2, 3, 4, 5, 8, 6, 7, 9, 10, 6, 11]])
    x = torch.zeros(12, 1, device=dev)
    ei = edge_index.to(dtype).to(dev)
    loader = LinkNeighborLoader(x, ei, [1], edge_label_index=ei, batch_size=2, shuffle=True,
                                prefetch=prefetch)
    seen = 0
    for batch in loader:
        assert torch.equal(batch.n_id.long()[batch.edge_index.long()].cpu(),
                           edge_index[:, batch.e_id.long().cpu()])
        seen += batch.input_id.numel()
    assert seen == 12


# ---- the reference-facing adapter -------------------------------------------------------------------
def test_adapter_sample_from_edges_and_link_loader(dev):
    try:
        from oracle import make_ref
        make_ref.import_reference()
        from torch_geometric.data import Data
        from torch_geometric.loader import LinkLoader
        from torch_geometric.sampler import EdgeSamplerInput, NegativeSampling
    except ImportError:
        pytest.skip('torch_geometric cannot be imported')
    from pytorch_geometric_amd import backend
    N, B = 200, 30
    ei = _graph(N, 1500, 31)
    data = Data(x=torch.randn(N, 8, generator=gen(32)), edge_index=ei, num_nodes=N).to(dev)
    smp = backend.neighbor_sampler(data, [3, 2], seed=5)
    inp = EdgeSamplerInput(torch.arange(B), ei[0, :B], ei[1, :B])
    out = smp.sample_from_edges(inp, NegativeSampling('binary', 1.0))
    assert len(out.metadata) == 4
    input_id, eli, label, src_time = out.metadata
    assert eli.shape == (2, 2 * B) and src_time is None
    assert torch.equal(out.node.long()[eli[:, :B]].cpu(), ei[:, :B])
    out = smp.sample_from_edges(inp, NegativeSampling('triplet', 2))
    assert len(out.metadata) == 5 and out.metadata[3].shape == (B, 2)
    assert torch.equal(out.node[out.metadata[1]].cpu(), ei[0, :B])
    loader = LinkLoader(data, link_sampler=smp, edge_label_index=ei[:, :100].to(dev),
                        neg_sampling=NegativeSampling('binary', 1.0), batch_size=25)
    n = 0
    for batch in loader:
        assert batch.edge_label_index.size(1) == 50
        g = batch.n_id[batch.edge_label_index]
        assert torch.equal(g[:, :25].cpu(), ei[:, batch.input_id.cpu()])
        assert torch.equal(batch.x, data.x[batch.n_id])
        n += 1
    assert n == 4
