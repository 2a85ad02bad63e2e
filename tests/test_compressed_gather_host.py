"""Host side of the compressed gather source (`x_format = PYGAMD_X_COMPRESSED`) — WITHOUT a device:
the C entry points are asked only for what their validation answers before any launch (a launch
that passes validation with a hub plan asks for its workspace and answers PYGAMD_ERR_WORKSPACE for
a NULL one)."""
import ctypes

import pytest
import torch

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3


def _spmm_args(F=256, n_rows=64, reduce=None, hubs=True):
    from pytorch_geometric_amd import _lib
    host = torch.zeros(n_rows * (F + 64) + 64, dtype=torch.float32)
    p = (host.data_ptr() + 15) // 16 * 16
    a = _lib.SpmmArgs()
    a.rowptr = a.col = a.x = a.out = p
    a.n_rows, a.n_src, a.F = n_rows, n_rows, F
    a.ldx, a.ldo = (F + 12 + 31) // 32 * 32, F
    a.idx_dtype, a.reduce = _lib.IDX_I64, _lib.SUM if reduce is None else reduce
    a.w_heads, a.head_dim = 1, F
    a.x_format = _lib.X_COMPRESSED
    if hubs:
        a.hub_rows = a.hub_chunk_ptr = p
        a.n_hub, a.n_chunks, a.hub_threshold, a.hub_chunk = 1, 3, 200, 96
    return a, p, host


def _fused_args(a, p, Fo=256):
    from pytorch_geometric_amd import _lib
    f = _lib.SageFusedArgs()
    f.x_root, f.ld_root = p, a.F
    f.w, f.ldw = p, 2 * a.F
    f.Fo, f.relu, f.save_agg = Fo, 0, 0
    f.y, f.ldy = p, Fo
    return f


@pytest.fixture
def split_lib():
    from pytorch_geometric_amd import _lib, _native
    lib = _lib.load()
    prev = _native.set_gemm_mode('split')
    yield lib
    _native.set_gemm_mode(prev)


def _spmm(lib, a):
    return lib.pygamd_spmm_csr(ctypes.byref(a), None, 0, None)


def _fused(lib, a, f):
    return lib.pygamd_sage_layer_fused(ctypes.byref(a), ctypes.byref(f), None, 0, None)


def _ws(lib, a, f):
    n = ctypes.c_size_t(0)
    assert lib.pygamd_sage_layer_fused_workspace_bytes(ctypes.byref(a), ctypes.byref(f),
                                                      ctypes.byref(n)) == OK
    return n.value


def test_spmm_takes_live_lists_over_compressed_rows(split_lib):
    from pytorch_geometric_amd import _lib
    a, p, _keep = _spmm_args()
    assert _spmm(split_lib, a) == WORKSPACE            # compressed rows alone: as before
    a.rowend = p
    assert _spmm(split_lib, a) == WORKSPACE            # ... with rowend: validation passes now
    a.reduce = _lib.MEAN                               # rowend with a hub plan: the plain sum only
    assert _spmm(split_lib, a) == UNSUPPORTED
    a.reduce = _lib.MAX
    assert _spmm(split_lib, a) == UNSUPPORTED
    a.reduce = _lib.SUM
    a.src_bits = p                                     # compressed rows carry no row bitmap
    assert _spmm(split_lib, a) == UNSUPPORTED
    a.src_bits = None
    a.src_scale = p
    assert _spmm(split_lib, a) == UNSUPPORTED
    a.src_scale = None
    a.ldx = a.F + 8                                    # no room for header + values
    assert _spmm(split_lib, a) in (INVALID, UNSUPPORTED)


def test_split_schedule_takes_compressed_rows_wider_than_128(split_lib):
    from pytorch_geometric_amd import _lib
    a, p, _keep = _spmm_args()
    f = _fused_args(a, p)
    assert _fused(split_lib, a, f) == WORKSPACE        # validation passed
    a.rowend = p
    assert _fused(split_lib, a, f) == WORKSPACE        # live lists over compressed rows
    a.reduce = _lib.MEAN                               # (with a hub plan: the plain sum only)
    assert _fused(split_lib, a, f) == UNSUPPORTED
    a.reduce, a.rowend = _lib.SUM, None
    a.ldx = a.F + 8
    assert _fused(split_lib, a, f) == INVALID
    a.ldx = 288
    a.src_bits = p
    assert _fused(split_lib, a, f) == INVALID
    a.src_bits = None
    f.save_agg = 2                                     # rows given: the stored rows are dense
    assert _fused(split_lib, a, f) in (INVALID, UNSUPPORTED)


def test_workspace_query_sizes_the_weight_planes_for_a_compressed_source(split_lib):
    from pytorch_geometric_amd import _lib
    a, p, keep = _spmm_args(hubs=False)
    f = _fused_args(a, p)
    planes = _ws(split_lib, a, f)
    a.x_format, a.ldx = _lib.X_DENSE, a.F
    assert planes == _ws(split_lib, a, f) > 0          # the same planes as for dense rows
    # kept refusals of the split schedule: these launches run the fp32-instruction kernel, which
    # needs no planes
    a.x_format, a.ldx = _lib.X_COMPRESSED, 288
    f.compressed_out, f.ld_compressed = keep.data_ptr(), 288
    assert _ws(split_lib, a, f) == 0
    a2, p2, _keep2 = _spmm_args(F=128, hubs=False)     # compressed rows of <= 128 columns
    assert _ws(split_lib, a2, _fused_args(a2, p2)) == 0


@pytest.mark.parametrize('scaled', [False, True])
def test_rows_compress_argument_errors(scaled):
    from pytorch_geometric_amd import _lib
    lib = _lib.load()
    host = torch.zeros(1024, dtype=torch.float32)
    p = host.data_ptr()

    def call(x, ldx, n, F, out, ldo):
        if scaled:
            return lib.pygamd_rows_compress_scaled(x, ldx, n, F, p, out, ldo, None)
        return lib.pygamd_rows_compress(x, ldx, n, F, out, ldo, None)

    assert call(p, 260, 2, 260, p, 288) == INVALID     # more than 256 columns
    assert call(p, 64, 2, 64, p, 64 + 8) == INVALID    # pitch below F + 12
    assert call(p, 32, 2, 64, p, 96) == INVALID        # ldx below F
    assert call(p, 64, -1, 64, p, 96) == INVALID
    assert call(p, 64, 2, 64, None, 96) == INVALID
    assert call(None, 64, 2, 64, p, 96) == INVALID
    assert call(None, 64, 0, 64, None, 96) == OK       # nothing to do
