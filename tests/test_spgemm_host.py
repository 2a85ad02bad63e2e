"""The sparse-sparse product without a GPU: the entry points' argument checks, the generic route
of ``EdgeIndex.matmul(EdgeIndex)`` against the dense product, ``GraphUNet``'s interface and its
``augment_adj`` against the reference's."""
import ctypes

import pytest
import torch


def test_entry_points_validate_without_a_device():
    from pytorch_geometric_amd import _lib
    lib = _lib.load()
    plan, long = ctypes.c_size_t(0), ctypes.c_size_t(0)
    sizes = (ctypes.byref(plan), ctypes.byref(long))
    assert lib.pygamd_spgemm_workspace_size(_lib.IDX_I64, 1000, 0, 0, *sizes) == 0
    assert plan.value >= 5 * 8 * 1000 and long.value == 0
    assert lib.pygamd_spgemm_workspace_size(_lib.IDX_I64, 1000, 2, 5000, *sizes) == 0
    assert long.value >= 5000 * (3 * 8 + 4)
    assert lib.pygamd_spgemm_workspace_size(7, 1000, 0, 0, *sizes) == 1          # dtype
    assert lib.pygamd_spgemm_workspace_size(_lib.IDX_I32, -1, 0, 0, *sizes) == 1  # size
    assert lib.pygamd_spgemm_workspace_size(_lib.IDX_I32, 4, 0, 0, None, None) == 1
    assert lib.pygamd_spgemm_workspace_size(_lib.IDX_I32, 4, 1, 2 ** 31, *sizes) == 2
    ptr = ctypes.c_void_p(256)   # never dereferenced: every call below fails its checks first
    totals = (ctypes.c_int64 * 4)()
    sym = lambda *a: lib.pygamd_spgemm_symbolic(*a)
    assert sym(None, None, None, None, 1, 4, 4, 4, 0, 0, None, None, None, 0, None) == 1
    assert sym(ptr, ptr, ptr, ptr, 9, 4, 4, 4, 1, 1, ptr, totals, ptr, 1 << 20, None) == 1
    assert sym(ptr, ptr, ptr, ptr, 1, 4, -4, 4, 1, 1, ptr, totals, ptr, 1 << 20, None) == 1
    assert sym(ptr, None, ptr, ptr, 1, 4, 4, 4, 1, 1, ptr, totals, ptr, 1 << 20, None) == 1
    assert sym(ptr, ptr, ptr, ptr, 1, 4, 4, 2 ** 31, 1, 1, ptr, totals, ptr, 1 << 20, None) == 2
    assert sym(ptr, ptr, ptr, ptr, 1, 4, 4, 4, 1, 1, ptr, totals, ptr, 8, None) == 3
    num = lambda *a: lib.pygamd_spgemm_numeric(*a)
    tail = (0, 0, ptr, 1 << 20, None, 0, None)
    assert num(None, None, None, None, None, None, 1, 4, 4, 4, 0, 0, None, 0, None, None,
               *tail) == 1
    assert num(ptr, ptr, None, ptr, ptr, None, 1, 4, 4, 4, 1, 1, ptr, 3, None, None, *tail) == 1
    assert num(ptr, ptr, None, ptr, ptr, None, 1, 4, 4, 4, 1, 1, ptr, -1, ptr, ptr, *tail) == 1
    assert num(ptr, ptr, None, ptr, ptr, None, 1, 4, 4, 4, 1, 1, ptr, 3, ptr, ptr, 0, 0, ptr, 8,
               None, 0, None) == 3
    assert num(ptr, ptr, None, ptr, ptr, None, 1, 4, 4, 4, 1, 1, ptr, 3, ptr, ptr, 1, 9, ptr,
               1 << 20, ptr, 8, None) == 3


def test_tier_bounds_are_header_constants():
    from pytorch_geometric_amd import _lib, _native
    c = _lib.CONSTANTS
    assert (_native.SPGEMM_WAVE_UB, _native.SPGEMM_GROUP_SMALL_UB, _native.SPGEMM_GROUP_UB) == (
        c['PYGAMD_SPGEMM_WAVE_UB'], c['PYGAMD_SPGEMM_GROUP_SMALL_UB'], c['PYGAMD_SPGEMM_GROUP_UB'])
    assert 0 < _native.SPGEMM_WAVE_UB < _native.SPGEMM_GROUP_SMALL_UB < _native.SPGEMM_GROUP_UB
    assert c['PYGAMD_SPGEMM_TIERS'] == 5


def handles(dtype=torch.int64, value_dtype=torch.float32):
    from pytorch_geometric_amd.edge_index import EdgeIndex
    g = torch.Generator().manual_seed(0)
    a = torch.stack([torch.randint(0, 5, (14, ), generator=g),
                     torch.randint(0, 7, (14, ), generator=g)]).to(dtype)
    b = torch.stack([torch.randint(0, 7, (11, ), generator=g),
                     torch.randint(0, 3, (11, ), generator=g)]).to(dtype)
    va = torch.randint(-2, 3, (14, ), generator=g).to(value_dtype)
    vb = torch.randint(-2, 3, (11, ), generator=g).to(value_dtype)
    return (EdgeIndex(a, (5, 7), validate=False), va), (EdgeIndex(b, (7, 3), validate=False), vb)


def dense_of(ei, val, size):
    val = torch.ones(ei.size(1)) if val is None else val
    return torch.zeros(size, dtype=torch.float64).index_put((ei[0].long(), ei[1].long()),
                                                            val.double(), accumulate=True)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('value_dtype', [torch.float32, torch.float64, None])
def test_generic_route_equals_the_dense_product(dtype, value_dtype):
    (A, va), (B, vb) = handles(dtype, value_dtype or torch.float32)
    if value_dtype is None:
        va = vb = None
    prod, val = A.matmul(B, va, vb)
    assert prod.sparse_size == (5, 3) and prod.sort_order == 'row' and prod.dtype == dtype
    want = dense_of(A.edge_index, va, (5, 7)) @ dense_of(B.edge_index, vb, (7, 3))
    assert torch.equal(dense_of(prod.edge_index, val, (5, 3)), want)
    key = prod.edge_index[0].long() * 3 + prod.edge_index[1].long()
    assert bool((key[1:] > key[:-1]).all())          # row-major, columns ascending and unique
    assert torch.equal(prod.get_csr()[0][0].long(),
                       torch._convert_indices_from_coo_to_csr(prod.edge_index[0].long(), 5))
    # transpose: A^T [7 x 5] @ A [5 x 7]
    prod, val = A.matmul(A, va, va, transpose=True)
    assert prod.sparse_size == (7, 7)
    da = dense_of(A.edge_index, va, (5, 7))
    assert torch.equal(dense_of(prod.edge_index, val, (7, 7)), da.t() @ da)


def test_errors_follow_the_reference():
    (A, va), (B, vb) = handles()
    with pytest.raises(NotImplementedError, match="reduce='mean'"):
        A.matmul(B, va, vb, reduce='mean')
    with pytest.raises(ValueError, match="'other_value' not supported"):
        A.matmul(torch.randn(7, 2), va, vb)
    with pytest.raises(ValueError, match='sparse sizes'):
        A.matmul(A, va, va)


def test_graph_unet_interface():
    from pytorch_geometric_amd import nn
    from pytorch_geometric_amd.nn.models import GraphUNet
    assert nn.GraphUNet is GraphUNet
    model = GraphUNet(3, 16, 2, depth=3, pool_ratios=[0.8, 0.5])
    assert repr(model) == 'GraphUNet(3, 16, 2, depth=3, pool_ratios=[0.8, 0.5, 0.5])'
    names = [k for k, _ in model.named_parameters()]
    assert names[:4] == ['down_convs.0.bias', 'down_convs.0.lin.weight', 'down_convs.1.bias',
                         'down_convs.1.lin.weight']
    assert 'pools.2.select.weight' in names and 'up_convs.2.lin.weight' in names
    assert len(names) == 4 * 2 + 3 + 3 * 2
    assert isinstance(model.fuse, bool)
    cat = GraphUNet(3, 16, 2, depth=1, sum_res=False)
    assert cat.up_convs[0].lin.weight.shape == (2, 32)


def test_augment_adj_equals_the_reference_on_the_cpu():
    from oracle import make_ref
    if make_ref.staged_path() is None:
        pytest.skip('the reference is not staged')
    make_ref.import_reference()
    from torch_geometric.nn import GraphUNet as Reference
    from pytorch_geometric_amd.nn import GraphUNet
    g = torch.Generator().manual_seed(0)
    ei = torch.randint(0, 30, (2, 90), generator=g)
    weight = torch.randint(1, 4, (90, ), generator=g).float()
    ref, model = Reference(3, 8, 2, depth=1), GraphUNet(3, 8, 2, depth=1)
    assert [k for k, _ in model.named_parameters()] == [k for k, _ in ref.named_parameters()]
    model.load_state_dict(ref.state_dict())
    want_ei, want_w = ref.augment_adj(ei, weight, 30)
    got_ei, got_w = model.augment_adj(ei, weight, 30)
    # (the reference's CSR product leaves the columns of a row in no particular order here:
    # compared in row-major order, which is the order of ours)
    order = (want_ei[0] * 30 + want_ei[1]).argsort()
    assert torch.equal(got_ei, want_ei[:, order]) and torch.equal(got_w, want_w[order])
