"""The sparse-sparse product on the GPU (csrc/spgemm.hip) against the dense float64 product of the
densified operands: structure and values EXACTLY on integer values (every sum stays below 2^24, so
no summation order can round), bit-identical runs, the floating-point bound on real values;
``EdgeIndex.matmul(EdgeIndex)`` and ``GraphUNet`` against the real reference on the CPU copy."""
import pytest
import torch

from tests._util import _call_counts, assert_close_scaled

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_REF = {}


def csr(lens, rule):
    """rowptr, col of the matrix whose row i holds the columns ``rule(i, arange(lens[i]))``"""
    lens = torch.as_tensor(lens, dtype=torch.long)
    cols = [rule(i, torch.arange(int(n))).long() for i, n in enumerate(lens.tolist())]
    rowptr = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
    return rowptr, torch.cat(cols) if cols else lens.new_zeros(0)


def dense(rowptr, col, val, n_cols, dtype=torch.float64):
    row = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr.diff())
    out = torch.zeros(rowptr.numel() - 1, n_cols, dtype=dtype)
    return out.index_put((row, col), val.to(dtype), accumulate=True)


def constants():
    from pytorch_geometric_amd import _native
    return _native.SPGEMM_WAVE_UB, _native.SPGEMM_GROUP_SMALL_UB, _native.SPGEMM_GROUP_UB


def power_law():
    """1,500 rows, row 0 a hub of 1,200; columns of a row distinct (7 is coprime to 1,500)"""
    n = 1500
    lens = (400.0 / torch.arange(1, n + 1).float().pow(0.75)).long().clamp(min=1)
    lens[0], lens[7], lens[1499] = 1200, 0, 0   # (rows per tier of A @ A: 2, 1478, 18, 1, 1)
    return csr(lens, lambda i, j: (11 * i + 7 * j) % n), n


def spread(T):
    """rows with T - 1, T, T + 1 products, all on distinct columns: B's rows own disjoint column
    ranges, of 16 columns (rows 0 .. R - 1), 15 (row R) and 1 (row R + 1)"""
    R = T // 16
    b = csr([16] * R + [15, 1], lambda k, j: 16 * k + j)
    picks = [list(range(R - 1)) + [R], list(range(R)), list(range(R)) + [R + 1]]
    a = csr([len(p) for p in picks], lambda i, j: torch.tensor(picks[i])[j])
    return a, b, (3, R + 2, 16 * (R + 2))


def pile(T):
    """the same products, all on ONE column: T + 1 rows of B hold column 5 only"""
    b = csr([1] * (T + 1), lambda k, j: j + 5)
    a = csr([T - 1, T, T + 1], lambda i, j: (j + i) % (T + 1))
    return a, b, (3, T + 1, 9)


def cases():
    t_w, t_s, t_g = constants()
    out = {}
    # an empty row of A, a row of A that reaches only empty rows of B, and an empty B
    a = csr([2, 0, 1, 3, 1], lambda i, j: (2 * i + 3 * j) % 7)
    out['rectangular'] = (a, csr([0, 2, 0, 1, 3, 0, 2], lambda k, j: (k + j) % 3), (5, 7, 3))
    out['row_onto_empty'] = (csr([2, 1], lambda i, j: j * 2), csr([0, 2, 0], lambda k, j: j),
                             (2, 3, 3))
    out['empty_b'] = (a, csr([0] * 7, lambda k, j: j), (5, 7, 3))
    for name, T in (('wave', t_w), ('group_small', t_s), ('group', t_g)):
        assert T % 16 == 0
        out[f'{name}_spread'], out[f'{name}_pile'] = spread(T), pile(T)
    full = csr([64] * 64, lambda i, j: j)
    out['full_block'] = (full, full, (64, 64, 64))
    # (values +1, -1 are set by the test) onto two identical rows: an explicit zero
    out['cancel'] = (csr([2], lambda i, j: j), csr([3, 3], lambda k, j: 2 * j), (1, 2, 6))
    # a duplicated entry and unsorted columns in A
    out['loose_a'] = (csr([4, 3], lambda i, j: torch.tensor([[3, 1, 3, 0], [2, 0, 1, 0]])[i][j]),
                      csr([2, 3, 1, 2], lambda k, j: (k + 2 * j) % 5), (2, 4, 5))
    (ptr, col), n = power_law()
    out['power_law'] = ((ptr, col), (ptr, col), (n, n, n))
    return out


CASES = None


def case(name):
    global CASES
    CASES = CASES or cases()
    return CASES[name]


NAMES = ['rectangular', 'row_onto_empty', 'empty_b', 'wave_spread', 'wave_pile',
         'group_small_spread', 'group_small_pile', 'group_spread', 'group_pile', 'full_block',
         'cancel', 'loose_a', 'power_law']


def run(a, b, va, vb, size, dtype):
    from pytorch_geometric_amd import _native
    dev = lambda t: None if t is None else t.to(DEV)
    out = _native.spgemm(a[0].to(dtype).to(DEV), a[1].to(dtype).to(DEV), dev(va),
                         b[0].to(dtype).to(DEV), b[1].to(dtype).to(DEV), dev(vb), *size)
    torch.cuda.synchronize()
    return out


def integer_values(n, seed, name):
    if name == 'cancel':   # A = [+1, -1] onto two identical rows of B
        return torch.tensor([1., -1.] if seed == 0 else [2., 1., -2., 2., 1., -2.])
    return torch.randint(-2, 3, (n, ), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize('with_values', [True, False])
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('name', NAMES)
def test_product_is_exact_on_integers(name, dtype, with_values):
    a, b, (M, K, N) = case(name)
    va = integer_values(a[1].numel(), 0, name) if with_values else None
    vb = integer_values(b[1].numel(), 1, name) if with_values else None
    ones = lambda m: torch.ones(m[1].numel())
    da = dense(*a, ones(a) if va is None else va, K)
    db = dense(*b, ones(b) if vb is None else vb, N)
    want = da @ db
    pattern = (dense(*a, ones(a), K) != 0).double() @ (dense(*b, ones(b), N) != 0).double() > 0
    assert float(want.abs().max()) < 2 ** 24 if want.numel() else True
    rowptr, col, val = run(a, b, va, vb, (M, K, N), dtype)
    assert rowptr.dtype == col.dtype == dtype and val.dtype == torch.float32
    want_ptr = torch.cat([torch.zeros(1, dtype=torch.long), pattern.sum(1).cumsum(0)])
    assert torch.equal(rowptr.cpu().long(), want_ptr), 'rowptr_c'
    assert torch.equal(col.cpu().long(), pattern.nonzero()[:, 1]), 'col_c (ascending per row)'
    assert torch.equal(val.cpu(), want[pattern].float()), 'val_c'
    if name == 'cancel' and with_values:
        assert val.numel() == 3 and not val.any()     # stored, and exactly zero
    again = run(a, b, va, vb, (M, K, N), dtype)
    assert all(torch.equal(x, y) for x, y in zip((rowptr, col, val), again)), 'second run'


def test_real_values_stay_within_the_summation_bound():
    """|C - C64| <= 2 d 2^-24 (|A| |B|), d the longest row of A: the first-order error of d
    products and d - 1 additions in any order, with a factor of two to spare"""
    a, b, (M, K, N) = case('power_law')
    g = torch.Generator().manual_seed(5)
    va, vb = torch.randn(a[1].numel(), generator=g), torch.randn(b[1].numel(), generator=g)
    rowptr, col, val = run(a, b, va, vb, (M, K, N), torch.int64)
    da, db = dense(*a, va, K), dense(*b, vb, N)
    got = dense(rowptr.cpu(), col.cpu(), val.cpu(), N)
    d = int(a[0].diff().max())
    bound = 2 * d * 2.0 ** -24 * (da.abs() @ db.abs())
    err = (got - da @ db).abs()
    print(f'max err {float(err.max()):.3e}, smallest slack {float((bound - err).min()):.3e}')
    assert bool((err <= bound).all())


# ---- EdgeIndex.matmul(EdgeIndex) ---------------------------------------------------------------
def handle(m, size, dev=DEV):
    from pytorch_geometric_amd.edge_index import EdgeIndex
    row = torch.repeat_interleave(torch.arange(m[0].numel() - 1), m[0].diff())
    return EdgeIndex(torch.stack([row, m[1]]).to(dev), size, validate=False)


def dense_of(ei, val, size):
    out = torch.zeros(size, dtype=torch.float64)
    return out.index_put((ei[0].cpu(), ei[1].cpu()), val.cpu().double(), accumulate=True)


def test_edge_index_matmul_power_law(monkeypatch):
    a, _, (n, _, _) = case('power_law')
    va = integer_values(a[1].numel(), 0, '')
    A = handle(a, (n, n))
    out = {}
    counts = _call_counts(monkeypatch,
                          lambda: out.update(r=A.matmul(A, va.to(DEV), va.to(DEV), fuse=True)))
    for fn in ('workspace_size', 'symbolic', 'numeric'):
        assert counts.get(f'pygamd_spgemm_{fn}') == 1, counts
    prod, val = out['r']
    rowptr, col, want = run(a, a, va, va, (n, n, n), torch.int64)
    assert prod.sparse_size == (n, n) and prod.sort_order == 'row'
    assert torch.equal(prod.get_csr()[0][0], rowptr) and torch.equal(prod.edge_index[1], col)
    assert bool((prod.edge_index[0][1:] >= prod.edge_index[0][:-1]).all())
    assert torch.equal(val, want)
    # a result carries the mark: as `other` it is not coalesced again
    counts = _call_counts(monkeypatch, lambda: A.matmul(prod, None, val, fuse=True))
    assert 'pygamd_edge_key' not in counts and counts.get('pygamd_spgemm_numeric') == 1


def test_edge_index_matmul_transpose_and_duplicates():
    a, b, (M, K, N) = case('rectangular')
    va, vb = integer_values(a[1].numel(), 3, ''), integer_values(b[1].numel(), 4, '')
    A, B = handle(a, (M, K)), handle(b, (K, N))
    # transpose: (A^T)[K x M] needs an `other` with M rows
    other = handle(csr([2, 1, 0, 3, 2], lambda k, j: (k + j) % 4), (M, 4))
    vo = integer_values(other.num_edges, 6, '')
    prod, val = A.matmul(other, va.to(DEV), vo.to(DEV), transpose=True, fuse=True)
    want = dense_of(A.edge_index, va, (M, K)).t() @ dense_of(other.edge_index, vo, (M, 4))
    assert prod.sparse_size == (K, 4)
    assert torch.equal(dense_of(prod.edge_index, val, (K, 4)), want)
    # an `other` with every edge twice, shuffled: the coalesced product
    from pytorch_geometric_amd.edge_index import EdgeIndex
    perm = torch.randperm(2 * B.num_edges, generator=torch.Generator().manual_seed(2))
    twice = EdgeIndex(torch.cat([B.edge_index, B.edge_index], 1)[:, perm.to(DEV)], (K, N),
                      validate=False)
    vb2 = torch.cat([vb, vb])[perm]
    for value in (vb2, None):
        prod, val = A.matmul(twice, va.to(DEV), None if value is None else value.to(DEV),
                             fuse=True)
        db = dense_of(twice.edge_index, torch.ones(twice.num_edges) if value is None else value,
                      (K, N))
        assert torch.equal(dense_of(prod.edge_index, val, (M, N)),
                           dense_of(A.edge_index, va, (M, K)) @ db)
        assert int(prod.get_csr()[0][0][-1]) == prod.num_edges == val.numel()


# ---- GraphUNet ---------------------------------------------------------------------------------
def reference_unet():
    if not _REF:
        from oracle import make_ref
        make_ref.import_reference()
        from torch_geometric.nn import GraphUNet
        _REF.update(GraphUNet=GraphUNet)
    return _REF['GraphUNet']


def two_graphs(seed=0):
    """40 nodes in two graphs of 20, 120 edges inside the graphs (self loops and duplicates
    included, as they come), integer weights"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 20, (120, ), generator=g)
    dst = torch.randint(0, 20, (120, ), generator=g)
    off = (torch.arange(120) % 2) * 20
    batch = torch.arange(40) // 20
    weight = torch.randint(1, 4, (120, ), generator=g).float()
    return torch.stack([src + off, dst + off]), batch, weight


def test_augment_adj_equals_the_reference():
    from pytorch_geometric_amd.nn import GraphUNet
    ei, _, weight = two_graphs()
    ref = reference_unet()(3, 16, 2, depth=2)
    want_ei, want_w = ref.augment_adj(ei, weight, 40)
    model = GraphUNet(3, 16, 2, depth=2)
    model.fuse = True
    got_ei, got_w = model.augment_adj(ei.to(DEV), weight.to(DEV), 40)
    # (the reference's CSR product on the CPU leaves the columns of a row in no particular
    # order: compared in row-major order, which is the order of ours)
    order = (want_ei[0] * 40 + want_ei[1]).argsort()
    assert torch.equal(got_ei.cpu(), want_ei[:, order]) and torch.equal(got_w.cpu(), want_w[order])


@pytest.mark.parametrize('sum_res', [True, False])
def test_graph_unet_matches_the_reference(sum_res):
    from pytorch_geometric_amd.nn import GraphUNet
    ei, batch, _ = two_graphs(1)
    torch.manual_seed(3)
    ref = reference_unet()(5, 16, 4, depth=2, pool_ratios=0.6, sum_res=sum_res)
    model = GraphUNet(5, 16, 4, depth=2, pool_ratios=0.6, sum_res=sum_res)
    assert [k for k, _ in model.named_parameters()] == [k for k, _ in ref.named_parameters()]
    model.load_state_dict(ref.state_dict())
    model = model.to(DEV)
    model.fuse = True
    x = torch.randn(40, 5)
    want = ref(x, ei, batch)
    want.square().sum().backward()
    got = model(x.to(DEV), ei.to(DEV), batch.to(DEV))
    got.square().sum().backward()
    assert_close_scaled(got, want, what='GraphUNet output')
    grads = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        assert_close_scaled(p.grad, grads[name].grad, what=name)
