"""ctypes binding of ``libpyg_amd.so`` — the C ABI declared in ``include/pyg_amd.h``.

This module is the only place that touches the shared object.  There is deliberately no CPU
fallback: if the library is missing (and cannot be built) or a call fails, we raise.
"""
import ctypes
import os
from ctypes import Structure

from . import _build, _header
from ._header import PygAmdError


def _read(name):
    path = os.path.join(os.path.dirname(_build.PKG_DIR), 'include', name)
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise PygAmdError(f"{path} is missing: the ctypes binding of the library is derived from "
                          f"the header that declares it ({e})") from None


# Everything below that mirrors the C boundary — constants, argument structs, signatures — is read
# from the two headers, once, here.
_H = _header.parse(_read('pyg_amd.h'))
_LAB = _header.parse(_read('pyg_amd_lab.h'), included=_H)
CONSTANTS = _H.constants  # every `#define PYGAMD_X <integer>` and enumerator of include/pyg_amd.h

ABI_VERSION = CONSTANTS['PYGAMD_ABI_VERSION']
X_DENSE, X_COMPRESSED = CONSTANTS['PYGAMD_X_DENSE'], CONSTANTS['PYGAMD_X_COMPRESSED']
AGG_GIVEN = CONSTANTS['PYGAMD_AGG_GIVEN']  # save_agg of the one-kernel SAGE layer, "rows given"
IDX_I32, IDX_I64 = CONSTANTS['PYGAMD_IDX_I32'], CONSTANTS['PYGAMD_IDX_I64']
SUM, MEAN, MIN, MAX, MUL, ANY = (CONSTANTS['PYGAMD_' + r]
                                 for r in ('SUM', 'MEAN', 'MIN', 'MAX', 'MUL', 'ANY'))
REDUCE_IDS = {'sum': SUM, 'add': SUM, 'mean': MEAN, 'min': MIN, 'amin': MIN, 'max': MAX,
              'amax': MAX, 'mul': MUL, 'any': ANY}
ERR_UNSUPPORTED, ERR_HIP = CONSTANTS['PYGAMD_ERR_UNSUPPORTED'], CONSTANTS['PYGAMD_ERR_HIP']
GEMM_MODES = {'fp32': CONSTANTS['PYGAMD_GEMM_FP32'], 'split': CONSTANTS['PYGAMD_GEMM_SPLIT_BF16']}


class SpmmArgs(Structure):
    """Mirror of ``pygamd_spmm_args`` (include/pyg_amd.h)."""
    _fields_ = _header.fields(_H.structs['pygamd_spmm_args'])


class Csr(Structure):
    """Mirror of ``pygamd_csr`` (include/pyg_amd.h): a CSR handle with its hub plan."""
    _fields_ = _header.fields(_H.structs['pygamd_csr'])


class HopArgs(Structure):
    """Mirror of ``pygamd_hop_args`` (include/pyg_amd.h): one propagation step and its epilogue."""
    _fields_ = _header.fields(_H.structs['pygamd_hop_args'])


class SageFusedArgs(Structure):
    """Mirror of ``pygamd_sage_fused_args`` (include/pyg_amd.h)."""
    _fields_ = _header.fields(_H.structs['pygamd_sage_fused_args'])


MIRRORS = {'pygamd_spmm_args': SpmmArgs, 'pygamd_csr': Csr, 'pygamd_hop_args': HopArgs,
           'pygamd_sage_fused_args': SageFusedArgs}

# name -> (restype, argtypes) of every PYGAMD_API symbol of include/pyg_amd.h, and of
# include/pyg_amd_lab.h: schedules measured and not adopted + timing probes (NOT the boundary;
# exported by libpyg_amd_lab.so only)
SIGNATURES = _header.signatures(_H, MIRRORS)
LAB_SIGNATURES = _header.signatures(_LAB, MIRRORS)

_lib = None       # libpyg_amd.so: the product library (include/pyg_amd.h, nothing else)
_lab = None       # libpyg_amd_lab.so: the same sources + the laboratory entry points
_use_lab = False  # route load() to the laboratory build (tests / scripts that select a variant)


def lib_path():
    return _build.LIB_PATH


def _open(path, signatures):
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in signatures:
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.pygamd_abi_version() != ABI_VERSION:
        raise PygAmdError(f'ABI mismatch: {path} reports {lib.pygamd_abi_version()}')
    return lib


def _default_mode():
    # 'split' (round 4): error against fp64 at or below the fp32 matrix instruction's on the same
    # inputs (tests/test_gpu_split_accept.py, test_gpu_gemm.py), 2.7 x fewer matrix-pipe cycles;
    # PYGAMD_GEMM_MODE=fp32 selects the exact instruction (bitwise an fmaf chain)
    mode = os.environ.get('PYGAMD_GEMM_MODE', 'split')
    if mode not in GEMM_MODES:
        raise PygAmdError(f"PYGAMD_GEMM_MODE must be one of {sorted(GEMM_MODES)}, got '{mode}'")
    return GEMM_MODES[mode]


def load():
    """The product library (building first if the in-tree .so is missing/stale and hipcc
    exists) — or the laboratory build while :func:`use_lab` routes there."""
    global _lib
    if _use_lab:
        return load_lab()
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    if _build.is_stale():
        if _build.find_hipcc() is not None and os.environ.get('PYG_AMD_NO_BUILD') != '1':
            _build.build_library(verbose=False)
        elif not os.path.exists(path):
            raise PygAmdError(
                f"{path} is missing and hipcc is unavailable: run "
                f"`python -c 'import __graft_entry__ as g; g.build()'` on a machine with ROCm. "
                f"There is no CPU fallback for the pytorch_geometric_amd kernels.")
    lib = _open(path, list(SIGNATURES.items()))
    lib.pygamd_set_gemm_mode(_default_mode())
    _lib = lib
    return lib


def load_lab():
    """``libpyg_amd_lab.so``: the product sources plus csrc/sage_fused_lab.hip and the weight-
    gradient probes (include/pyg_amd_lab.h) — schedules measured and not adopted, timing probes,
    the copy-rate probe of bench.py's side figure.  Loaded by scripts/, the tests that pin those
    schedules to the production results, and that side figure; never by the product path."""
    global _lab
    if _lab is not None:
        return _lab
    path = _build.LAB_LIB_PATH
    if _build.lab_is_stale():
        if _build.find_hipcc() is not None and os.environ.get('PYG_AMD_NO_BUILD') != '1':
            _build.build_lab_library(verbose=False)
        elif not os.path.exists(path):
            raise PygAmdError(f"{path} is missing and hipcc is unavailable (the laboratory "
                              f"build: `python -m pytorch_geometric_amd._build`)")
    lab = _open(path, list(SIGNATURES.items()) + list(LAB_SIGNATURES.items()))
    # (its own copy of the process-wide switches: start from the product library's mode)
    lab.pygamd_set_gemm_mode(_lib.pygamd_get_gemm_mode() if _lib is not None else _default_mode())
    _lab = lab
    return lab


def use_lab(flag: bool) -> None:
    global _use_lab
    _use_lab = bool(flag)
    if _use_lab:
        load_lab()


def lab_active() -> bool:
    return _use_lab


def loaded():
    """The library objects that are open (for process-wide switches kept per library)."""
    if _lib is None and _lab is None:
        load()
    return [l for l in (_lib, _lab) if l is not None]


def check(rc, what=''):
    if rc != 0:
        lib = load()
        msg = lib.pygamd_status_string(rc).decode()
        extra = f' (hipError {lib.pygamd_last_hip_error()})' if rc == ERR_HIP else ''
        raise PygAmdError(f'{what or "pygamd call"} failed: {msg}{extra}')
