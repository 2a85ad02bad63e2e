"""Host side of the one-kernel 16-bit SAGE layer: the build list, the C boundary with its derived
binding, and the edges of the envelope query."""
import ctypes

import pytest


def test_source_boundary_and_binding():
    from pytorch_geometric_amd import _build, _lib
    assert 'sage_fused_lp.hip' in _build.SOURCES and _lib.ABI_VERSION == 11
    P, I, L, G = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_lib.Csr)
    S = _lib.SIGNATURES
    assert S['pygamd_sage_layer_lp_supported'] == (I, [I, L, L, I])
    assert S['pygamd_sage_layer_lp_workspace_size'] == (ctypes.c_size_t, [G, L])
    assert S['pygamd_sage_layer_lp'] == (I, [G, P, L, P, P, P, P, L, P, I, L, L, I, P,
                                             ctypes.c_size_t, P])


@pytest.mark.parametrize('dtype,F,Fo,reduce,ok', [
    (1, 8, 1, 'sum', 1), (2, 512, 512, 'mean', 1), (1, 512, 1, 'mean', 1), (2, 8, 512, 'sum', 1),
    (1, 0, 8, 'sum', 0), (1, 4, 8, 'sum', 0), (2, 12, 8, 'mean', 0), (2, 520, 8, 'sum', 0),
    (1, 64, 0, 'sum', 0), (2, 64, 513, 'mean', 0), (0, 64, 64, 'sum', 0), (3, 64, 64, 'sum', 0),
    (1, 64, 64, 'max', 0)])
def test_envelope(dtype, F, Fo, reduce, ok):
    from pytorch_geometric_amd import _lib
    lib = _lib.load()
    assert lib.pygamd_sage_layer_lp_supported(dtype, F, Fo, _lib.REDUCE_IDS[reduce]) == ok


def test_workspace_is_the_hub_partials():
    from pytorch_geometric_amd import _lib
    lib = _lib.load()
    g = _lib.Csr(n_hub=2, n_chunks=7)
    assert lib.pygamd_sage_layer_lp_workspace_size(ctypes.byref(g), 24) == 7 * 24 * 4
    assert lib.pygamd_sage_layer_lp_workspace_size(ctypes.byref(_lib.Csr()), 24) == 0
