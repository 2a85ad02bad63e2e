"""Host side of the 16-bit grouped GEMM: the build list, the C boundary and its derived binding,
argument checks that answer before any launch, and what still refuses."""
import ctypes

import pytest
import torch


def test_source_boundary_and_binding():
    from pytorch_geometric_amd import _build, _lib
    assert 'segmm_lp.hip' in _build.SOURCES and _lib.ABI_VERSION == 11
    S = _lib.SIGNATURES
    assert len(S['pygamd_segment_matmul_lp_supported'][1]) == 3
    assert len(S['pygamd_segment_matmul_lp'][1]) == 18
    assert S['pygamd_segment_matmul_lp_wgrad_workspace_size'][0] == ctypes.c_size_t
    assert len(S['pygamd_segment_matmul_lp_wgrad_workspace_size'][1]) == 3
    assert len(S['pygamd_segment_matmul_lp_wgrad'][1]) == 17


def test_envelope_and_workspace():
    from pytorch_geometric_amd import _lib
    lib = _lib.load()
    for dtype in (_lib.CONSTANTS['PYGAMD_DTYPE_F16'], _lib.CONSTANTS['PYGAMD_DTYPE_BF16']):
        for K in (1, 100, 4096):
            for N in (1, 100, 4096):
                assert lib.pygamd_segment_matmul_lp_supported(dtype, K, N) == 1
        assert lib.pygamd_segment_matmul_lp_supported(dtype, 0, 8) == 0
    assert lib.pygamd_segment_matmul_lp_supported(0, 8, 8) == 0
    assert lib.pygamd_segment_matmul_lp_supported(3, 8, 8) == 0
    assert lib.pygamd_segment_matmul_lp_wgrad_workspace_size(7, 24, 40) == 4 * 7 * 24 * 40


def test_bad_arguments_are_rejected_before_any_launch():
    """NULL pointers with work to do, negative sizes, pitches below the width: a status, no launch
    (there is no device here to launch on)."""
    from pytorch_geometric_amd import _lib
    lib = _lib.load()
    bf16 = _lib.CONSTANTS['PYGAMD_DTYPE_BF16']
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def product(x=p, ldx=8, w=p, n_tiles=1, K=8, N=8, blocks=1, out=p, ldo=8, tiles=p, dtype=bf16):
        return lib.pygamd_segment_matmul_lp(x, dtype, ldx, None, w, 64, 8, 1, 1, tiles, n_tiles, K,
                                            N, blocks, out, ldo, None, None)

    for bad in (dict(x=None), dict(w=None), dict(out=None), dict(tiles=None), dict(n_tiles=-1),
                dict(K=-1), dict(N=-8), dict(blocks=0), dict(ldx=7), dict(ldo=7), dict(dtype=0)):
        assert product(**bad) != 0, bad

    def wgrad(x=p, ldx=8, g=p, ldg=8, chunks=p, n_chunks=1, n_seg=1, K=8, N=8, blocks=1, gw=p,
              ws=p, ws_bytes=256, dtype=bf16):
        return lib.pygamd_segment_matmul_lp_wgrad(x, ldx, None, g, ldg, None, chunks, n_chunks,
                                                  n_seg, K, N, blocks, dtype, gw, ws, ws_bytes,
                                                  None)

    for bad in (dict(x=None), dict(g=None), dict(chunks=None), dict(gw=None), dict(ws=None),
                dict(ws_bytes=255), dict(n_chunks=-1), dict(n_seg=-1), dict(K=-1), dict(blocks=0),
                dict(ldx=7), dict(ldg=7), dict(dtype=3)):
        assert wgrad(**bad) != 0, bad


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float64])
def test_host_and_float64_tensors_still_refused(dtype):
    from pytorch_geometric_amd import utils
    with pytest.raises(NotImplementedError, match='float32'):
        utils.segment_matmul(torch.ones(2, 4, dtype=dtype), (0, 2), torch.ones(1, 4, 4, dtype=dtype))
