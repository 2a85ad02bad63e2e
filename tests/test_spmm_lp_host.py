"""Host side of the 16-bit CSR aggregation: the build list, the C boundary and its derived binding,
and what still refuses."""
import ctypes

import pytest
import torch


def test_source_boundary_and_binding():
    from pytorch_geometric_amd import _build, _lib
    assert 'spmm_lp.hip' in _build.SOURCES and _lib.ABI_VERSION == 11
    P, I, L, G = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_lib.Csr)
    S = _lib.SIGNATURES
    assert S['pygamd_spmm_lp_supported'] == (I, [I, L])
    assert S['pygamd_spmm_lp_workspace_size'] == (ctypes.c_size_t, [G, L])
    assert S['pygamd_spmm_lp'] == (I, [G, P, P, P, P, I, L, L, P, L, L, I, P, P, ctypes.c_size_t, P])
    assert (_lib.CONSTANTS['PYGAMD_DTYPE_F16'], _lib.CONSTANTS['PYGAMD_DTYPE_BF16']) == (1, 2)


def test_envelope():
    from pytorch_geometric_amd import _lib, _native
    lib = _lib.load()
    for dtype in (torch.float16, torch.bfloat16):
        assert all(_native.spmm_lp_supported(dtype, F) for F in (1, 8, 520, 100000))
        assert not _native.spmm_lp_supported(dtype, 0)
    assert not _native.spmm_lp_supported(torch.float32, 64)
    assert not _native.spmm_lp_supported(torch.float64, 64)
    assert lib.pygamd_spmm_lp_supported(0, 64) == 0 and lib.pygamd_spmm_lp_supported(3, 64) == 0
    g = _lib.Csr(n_hub=2, n_chunks=7)
    assert lib.pygamd_spmm_lp_workspace_size(ctypes.byref(g), 24) == 7 * 24 * 12
    assert lib.pygamd_spmm_lp_workspace_size(ctypes.byref(_lib.Csr()), 24) == 0


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float64])
def test_host_and_float64_tensors_still_refused(dtype):
    import pytorch_geometric_amd as pga
    h = pga.EdgeIndex(torch.tensor([[0, 1], [1, 0]]), (2, 2), validate=False)
    with pytest.raises(NotImplementedError, match='float32 only'):
        pga.utils.spmm(h, torch.ones(2, 4, dtype=dtype))
