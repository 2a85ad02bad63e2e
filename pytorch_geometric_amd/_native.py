"""Tensor-level wrappers over the C ABI: validate, allocate outputs with the torch caching
allocator, pass raw device pointers + the current HIP stream.  No arithmetic happens here.

PyTorch is plumbing only (device memory, streams).  Every function requires HIP device tensors
and raises otherwise — there is no CPU fallback.
"""
import collections
import ctypes
import os
import threading
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import _compiled, _lib
from ._lib import REDUCE_IDS, Csr, PygAmdError, SpmmArgs, check

# rows with more stored entries than this are split into chunks (see csrc/spmm.hip)
HUB_THRESHOLD = 1024
# (256-slot chunks: a chunk is ONE wave's chain of gathers — at 1,024 slots the ~700 chunks of the
# products shape were 700 waves on 1,024 SIMDs, 151 us per 256-wide launch; at 256: 71 us.  128
# gains nothing more: profiles/r06_bench_kernel_stats.md)
HUB_CHUNK = int(os.environ.get('PYGAMD_HUB_CHUNK', '256'))


def _require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise PygAmdError(
                'pytorch_geometric_amd kernels need HIP device tensors (got a '
                f'{t.device} tensor); there is no CPU fallback on this path')


def _idx_dtype(t: Tensor) -> int:
    if t.dtype == torch.int64:
        return _lib.IDX_I64
    if t.dtype == torch.int32:
        return _lib.IDX_I32
    raise ValueError(f"index tensors must be int32 or int64 (got {t.dtype})")


def _p(t: Optional[Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(ref: Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(ref.device).cuda_stream)


def _f32_rows(t: Tensor, name: str) -> Tensor:
    """2-D fp32 view with unit inner stride (row stride may exceed the width)."""
    if t.dtype != torch.float32:
        raise ValueError(f"'{name}' must be float32 (got {t.dtype})")
    if t.dim() != 2:
        raise ValueError(f"'{name}' must be two-dimensional (got {t.dim()} dimensions)")
    if t.size(1) > 0 and t.size(0) > 0 and (t.stride(1) != 1 or t.stride(0) < t.size(1)):
        t = t.contiguous()
    return t


def _ld(t: Tensor) -> int:
    return t.stride(0) if (t.size(0) > 1 and t.size(1) > 0) else max(t.size(1), 1)


def _plain(*tensors) -> bool:
    """Every given tensor is a 2-D fp32 HIP tensor: the operands the compiled binding
    (csrc/torch_binding.cpp, `torch.ops.pyg_amd_c`) takes as they are.  Anything else goes through
    the Python path below, which raises this package's typed errors."""
    for t in tensors:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
            return False
    return True


class HubPlan(NamedTuple):
    """The split of one row pointer's long rows: the hub rows, the exclusive scan of their chunk
    counts and the ``(threshold, chunk)`` the scan was computed for.  The three only mean something
    together, so a launch takes all of them from here (:func:`_csr`, :func:`_hub_args`,
    :func:`_hub6`) and never pairs a cached plan with the module's current settings."""
    rows: Optional[Tensor]         # None when n_hub == 0
    chunk_ptr: Optional[Tensor]    # [n_hub + 1]; None when n_hub == 0
    n_hub: int
    n_chunks: int
    threshold: int
    chunk: int


def no_hubs(threshold: Optional[int] = None, chunk: Optional[int] = None) -> HubPlan:
    """The plan of a row pointer none of whose rows needs splitting at these settings (default,
    as for :func:`hub_plan`: the module's, read now)."""
    return HubPlan(None, None, 0, 0, HUB_THRESHOLD if threshold is None else threshold,
                   HUB_CHUNK if chunk is None else chunk)


def _hub6(hub: Optional[HubPlan]) -> HubPlan:
    """The six loose hub arguments of a compiled route (``*_hub6(hub)``, in the plan's field
    order); None: no hub rows, and the module's pair, which no kernel reads without them."""
    return no_hubs() if hub is None else hub


def _hub_args(a: SpmmArgs, hub: Optional[HubPlan]) -> None:
    """The hub fields of a ``pygamd_spmm_args`` from a plan; without hub rows they stay zero.  The
    caller keeps ``hub`` bound until the launch has returned."""
    if hub is not None and hub.n_hub > 0:
        a.hub_rows, a.hub_chunk_ptr = hub.rows.data_ptr(), hub.chunk_ptr.data_ptr()
        a.n_hub, a.n_chunks = hub.n_hub, hub.n_chunks
        a.hub_threshold, a.hub_chunk = hub.threshold, hub.chunk


def _csr(rowptr: Tensor, col: Tensor, n_rows: int, hub: Optional[HubPlan]) -> Csr:
    """``pygamd_csr`` of a handle and its hub plan (``hub``: what :func:`hub_plan` returned for
    this ``rowptr``, or None: no hub rows), split at the plan's own threshold and chunk.  The
    struct keeps the tensors given here alive; the result of a ``.contiguous()`` the caller made
    for another argument of the launch is still the caller's to keep."""
    rows, cptr, n_hub, n_chunks, threshold, chunk = _hub6(hub)
    g = Csr(rowptr=rowptr.data_ptr(), col=col.data_ptr(), idx_dtype=_idx_dtype(rowptr),
            n_rows=n_rows, hub_rows=None if rows is None else rows.data_ptr(),
            hub_chunk_ptr=None if cptr is None else cptr.data_ptr(), n_hub=n_hub,
            n_chunks=n_chunks, hub_threshold=threshold, hub_chunk=chunk)
    g._keep = (rowptr, col, hub)
    return g


def _workspace(size_fn, dims, device, needed: bool = True):
    """``(buffer | None, bytes)`` for the ``pygamd_*_workspace_bytes`` query ``size_fn`` at
    ``dims``; no query when the caller does not need one."""
    if not needed:
        return None, 0
    nbytes = ctypes.c_size_t(0)
    check(size_fn(*dims, ctypes.byref(nbytes)))
    if nbytes.value == 0:
        return None, 0
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device), nbytes.value


def _strided_rows(t: Tensor, name: str, width: int) -> Tensor:
    """``[n, width]`` float32 rows with unit column stride: a contiguous tensor or a column block
    of a wider one (the halves of a packed key | value projection) is taken in place."""
    if t.dtype != torch.float32 or t.dim() != 2 or t.size(1) != width:
        raise ValueError(f"'{name}' must be a float32 [n, {width}] tensor (got {t.dtype} "
                         f"{tuple(t.shape)})")
    return t.contiguous() if t.stride(1) != 1 or t.stride(0) < width else t


def _dense_rows(t: Tensor, name: str, width: int) -> Tensor:
    """:func:`_strided_rows` for an operand that has no row stride: always contiguous."""
    return _strided_rows(t, name, width).contiguous()


def _grad_rows(rows: int, n_rows: int, width: int, device) -> Tensor:
    """An uninitialised ``[rows, width]`` gradient whose first ``n_rows`` rows a kernel writes;
    rows beyond them (destinations may be a prefix of the tensor's rows) take no gradient: 0."""
    alloc = torch.empty if rows == n_rows else torch.zeros
    return alloc(rows, width, dtype=torch.float32, device=device)


def _edge_rows(edge_attr: Tensor, E: int, width: str = 'De') -> Tensor:
    """``edge_attr`` checked to be a float32 ``[E, .]`` tensor, contiguous."""
    if edge_attr.dtype != torch.float32 or edge_attr.dim() != 2 or edge_attr.size(0) != E:
        raise ValueError(f"'edge_attr' must be a float32 [{E}, {width}] tensor (got "
                         f"{edge_attr.dtype} {tuple(edge_attr.shape)})")
    return edge_attr.contiguous()


def _edge_id(edge_id: Optional[Tensor], rowptr: Tensor, col: Tensor, name: str = 'edge_id'):
    """The slot -> edge map of a handle (None: the slots are the edges) checked, contiguous."""
    if edge_id is None:
        return None
    if edge_id.dtype != rowptr.dtype or edge_id.numel() != col.numel():
        raise ValueError(f"'{name}' must have the index dtype and one entry per slot")
    return edge_id.contiguous()


# ---- integer side --------------------------------------------------------------------------------
def index_sort(keys: Tensor, max_value: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    _require_device(keys)
    if keys.dim() != 1:
        raise ValueError("'inputs' must be one-dimensional")
    keys = keys.contiguous()
    lib = _lib.load()
    n = keys.numel()
    out = torch.empty_like(keys)
    perm = torch.empty(n, dtype=torch.int64, device=keys.device)
    if n == 0:
        return out, perm
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_index_sort_workspace_bytes(_idx_dtype(keys), n, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=keys.device)
    check(lib.pygamd_index_sort(_p(keys), _idx_dtype(keys), n,
                                -1 if max_value is None else int(max_value), _p(out), _p(perm),
                                _p(ws), nbytes.value, _stream(keys)), 'index_sort')
    return out, perm


def index2ptr(index: Tensor, size: int) -> Tensor:
    _require_device(index)
    C = _compiled.ops()
    if C is not None and index.dtype in (torch.int32, torch.int64):
        return C.index2ptr(index, size)
    index = index.contiguous()
    lib = _lib.load()
    ptr = torch.empty(size + 1, dtype=index.dtype, device=index.device)
    check(lib.pygamd_index2ptr(_p(index), _idx_dtype(index), index.numel(), size, _p(ptr),
                               _stream(index)), 'index2ptr')
    return ptr


def ptr2index(ptr: Tensor, n: int) -> Tensor:
    _require_device(ptr)
    C = _compiled.ops()
    if C is not None and ptr.dtype in (torch.int32, torch.int64):
        return C.ptr2index(ptr, n)
    ptr = ptr.contiguous()
    lib = _lib.load()
    out = torch.empty(n, dtype=ptr.dtype, device=ptr.device)
    check(lib.pygamd_ptr2index(_p(ptr), _idx_dtype(ptr), ptr.numel() - 1, n, _p(out),
                               _stream(ptr)), 'ptr2index')
    return out


def index_minmax(index: Tensor) -> Tuple[int, int]:
    """(min, max) of an index tensor; one host sync (the reference syncs here too)."""
    _require_device(index)
    index = index.contiguous()
    lib = _lib.load()
    mm = torch.empty(2, dtype=torch.int64, device=index.device)
    check(lib.pygamd_index_minmax(_p(index), _idx_dtype(index), index.numel(), _p(mm),
                                  _stream(index)), 'index_minmax')
    lo, hi = mm.tolist()
    return lo, hi


def permute_index(src: Tensor, perm: Tensor) -> Tensor:
    _require_device(src, perm)
    src = src.contiguous()
    lib = _lib.load()
    out = torch.empty(perm.numel(), dtype=src.dtype, device=src.device)
    check(lib.pygamd_permute_index(_p(src), _idx_dtype(src), _p(perm), perm.numel(), _p(out),
                                   _stream(src)), 'permute_index')
    return out


def cast_index(src: Tensor, dtype: torch.dtype) -> Tensor:
    _require_device(src)
    if src.dtype == dtype:
        return src
    assert src.dtype == torch.int64
    lib = _lib.load()
    out = torch.empty(src.numel(), dtype=dtype, device=src.device)
    check(lib.pygamd_cast_index(_p(src), src.numel(), _idx_dtype(out), _p(out), _stream(src)),
          'cast_index')
    return out


def index_guard(index: Tensor, size: int, err: Optional[Tensor] = None,
                dtype: Optional[torch.dtype] = None) -> Tensor:
    """A copy of ``index`` (as ``dtype``, default its own) with every entry outside ``[0, size)``
    replaced by the sentinel ``size``; ``err`` (device int32[1]) is set when there was one.  No
    host read."""
    _require_device(index, err)
    index = index.contiguous()
    out = torch.empty(index.numel(), dtype=dtype or index.dtype, device=index.device)
    lib = _lib.load()
    check(lib.pygamd_index_guard(_p(index), _idx_dtype(index), index.numel(), int(size), _p(out),
                                 _idx_dtype(out), _p(err), _stream(index)), 'index_guard')
    return out


def cumsum(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """``torch.cumsum(x, 0)`` of a 1-D int32 / int64 device tensor on the own scan kernels
    (``pygamd_cumsum``; ``out`` may be ``x`` or a contiguous slice such as ``offsets[1:]``)."""
    _require_device(x, out)
    if x.dim() != 1 or x.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"'x' must be a one-dimensional int32 / int64 tensor (got {x.dtype}, "
                         f"{x.dim()} dimensions)")
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError("'out' must be contiguous with the shape and dtype of 'x'")
    n = x.numel()
    if n == 0:
        return out
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_cumsum_workspace_bytes(_idx_dtype(x), n, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
    check(lib.pygamd_cumsum(_p(x), _idx_dtype(x), n, _p(out), _p(ws), nbytes.value, _stream(x)),
          'cumsum')
    return out


def hub_plan(rowptr: Tensor, threshold: Optional[int] = None,
             chunk: Optional[int] = None) -> HubPlan:
    """The :class:`HubPlan` of ``rowptr`` at ``(threshold, chunk)`` (default: the module's, read
    now); without a hub row the tensors are None and the counts 0."""
    _require_device(rowptr)
    none = no_hubs(threshold, chunk)
    threshold, chunk = none.threshold, none.chunk
    n_rows = rowptr.numel() - 1
    if n_rows <= 0:
        return none
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_hub_plan_workspace_bytes(_idx_dtype(rowptr), n_rows, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=rowptr.device)
    rows = torch.empty(n_rows, dtype=rowptr.dtype, device=rowptr.device)
    cptr = torch.empty(n_rows + 1, dtype=rowptr.dtype, device=rowptr.device)
    n_hub, n_chunks = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.pygamd_hub_plan(_p(rowptr), _idx_dtype(rowptr), n_rows, threshold, chunk, _p(rows),
                              _p(cptr), n_rows, ctypes.byref(n_hub), ctypes.byref(n_chunks),
                              _p(ws), nbytes.value, _stream(rowptr)), 'hub_plan')
    if n_hub.value == 0:
        return none
    return HubPlan(rows[:n_hub.value].clone(), cptr[:n_hub.value + 1].clone(), n_hub.value,
                   n_chunks.value, threshold, chunk)


# ---- CSR SpMM --------------------------------------------------------------------------------------
# Optional launch timing (bench.py): when a list is installed here, every spmm_csr call appends
# (info, start_event, end_event) recorded on the launch stream around the kernel(s).
timing_sink = None


class _timed:
    """Context manager: when bench.py installed a sink, record HIP events on the launch stream
    around the call(s) inside and append ``(info, start, end)``."""

    def __init__(self, info: dict, ref: Tensor):
        self.sink, self.info, self.ref = timing_sink, info, ref

    def __enter__(self):
        if self.sink is not None:
            st = torch.cuda.current_stream(self.ref.device)
            self.ev0 = torch.cuda.Event(enable_timing=True)
            self.ev1 = torch.cuda.Event(enable_timing=True)
            self.ev0.record(st)
        return self

    def __exit__(self, exc_type, exc, tb):
        if self.sink is not None and exc_type is None:
            self.ev1.record(torch.cuda.current_stream(self.ref.device))
            self.sink.append((self.info, self.ev0, self.ev1))
        return False


def spmm_csr(rowptr: Tensor, col: Optional[Tensor], x: Tensor, reduce: str, *,
             n_rows: Optional[int] = None, eid: Optional[Tensor] = None,
             w: Optional[Tensor] = None, src_scale: Optional[Tensor] = None,
             hub=None, out: Optional[Tensor] = None, return_arg: bool = False,
             accumulate: bool = False, hub_phase: int = 0, save_arg32: bool = False,
             relu_mask: Optional[Tensor] = None, relu_bits: Optional[Tensor] = None,
             src_bits: Optional[Tensor] = None, src_bits_set: Optional[Tensor] = None,
             compressed_width: Optional[int] = None, rowend: Optional[Tensor] = None,
             accumulate_rows: int = 0):
    """out[i] = reduce_k m(k) * x[col[k]] — see pygamd_spmm_csr in include/pyg_amd.h.
    ``rowend`` ([n_rows], dtype of ``rowptr``): row ``r`` owns the slots ``[rowptr[r], rowend[r])``
    (fixed-stride slot blocks of a static-shape sampled batch; ``rowptr`` then has ``n_rows``
    entries).  ``accumulate_rows``: with ``accumulate``, only rows below it have an old value.
    ``compressed_width=F``: ``x`` is the int32 block of :func:`rows_compress` holding ``F`` columns
    per row (sum / mean only; the same sums bit for bit).
    ``src_bits`` (from :func:`rows_pack`): one bit per row of ``x``, clear = the row is all zero
    and is not read; ``src_bits_set``: the device counter of set bits (dense inputs then ignore the
    bits)."""
    _require_device(rowptr, col, x, eid, w, src_scale, relu_mask, relu_bits, src_bits,
                    src_bits_set)
    if relu_mask is not None and relu_bits is not None:
        raise ValueError("pass at most one of 'relu_mask' / 'relu_bits'")
    if src_bits is not None:
        if (src_bits.dtype != torch.int32 or not src_bits.is_contiguous()
                or src_bits.numel() < (x.size(0) + 31) // 32):
            raise ValueError(f"'src_bits' must be contiguous int32 with one bit per row of x "
                             f'({(x.size(0) + 31) // 32} words)')
        if src_bits_set is not None and (src_bits_set.dtype != torch.int64
                                         or src_bits_set.numel() != 1):
            raise ValueError("'src_bits_set' must be one int64")
    if compressed_width is not None:
        return _spmm_csr_compressed(rowptr, col, x, reduce, compressed_width, n_rows, hub, out,
                                    hub_phase, rowend)
    if rowend is not None:
        _require_device(rowend)
        if rowend.dtype != rowptr.dtype or not rowend.is_contiguous() or n_rows is None \
                or rowend.numel() < n_rows or rowptr.numel() < n_rows:
            raise ValueError("'rowend' needs 'n_rows', the dtype of 'rowptr' and one entry per row")
    C = _compiled.ops()
    if (C is not None and not return_arg and src_bits is None and _plain(x, relu_mask)
            and rowend is None and accumulate_rows == 0
            and (w is None or (w.dtype == torch.float32 and
                               (w.dim() == 1 or x.size(1) % max(w.size(1), 1) == 0)))
            and rowptr.dtype in (torch.int32, torch.int64)):
        nr = rowptr.numel() - 1 if n_rows is None else n_rows
        F = x.size(1)
        if relu_mask is None or tuple(relu_mask.shape) == (nr, F):
            _check_bits(relu_bits, nr, F)
            if out is None:
                out = torch.empty(nr, F, dtype=torch.float32, device=x.device)
            arg32 = None
            if save_arg32 and reduce in ('min', 'max'):
                arg32 = torch.empty(nr, F, dtype=torch.int32, device=x.device)
            hub = _hub6(hub)
            with _timed({'n_rows': nr, 'n_src': x.size(0),
                         'nnz': col.numel() if col is not None else x.size(0), 'F': F,
                         'reduce': reduce, 'idx_bytes': rowptr.element_size(),
                         'weighted': w is not None, 'src_scale': src_scale is not None,
                         'accumulate': bool(accumulate), 'relu_mask': relu_mask is not None,
                         'relu_bits': relu_bits is not None, 'n_hub': hub.n_hub}, x):
                C.spmm_csr(rowptr, col, x, REDUCE_IDS[reduce], nr, eid, w, src_scale, *hub, out,
                           accumulate, hub_phase, arg32, relu_mask, relu_bits)
            return (out, arg32) if save_arg32 else out
    lib = _lib.load()
    x2 = _f32_rows(x, 'x')
    n_rows = rowptr.numel() - 1 if n_rows is None else n_rows
    F = x2.size(1)
    if out is None:
        out = torch.empty(n_rows, F, dtype=torch.float32, device=x.device)
    red = REDUCE_IDS[reduce]
    a = SpmmArgs()
    a.rowptr = rowptr.data_ptr()
    a.col = 0 if col is None else col.data_ptr()
    a.eid = 0 if eid is None else eid.data_ptr()
    w_heads, head_dim = 1, F
    if w is not None:
        if w.dtype != torch.float32:
            raise ValueError("edge weights must be float32")
        w = w.contiguous()
        w_heads = 1 if w.dim() == 1 else w.size(1)
        if w_heads > 1:
            if F % w_heads != 0:
                raise ValueError('feature width must be divisible by the number of heads')
            head_dim = F // w_heads
        a.w = w.data_ptr()
    if src_scale is not None:
        src_scale = src_scale.contiguous()
        a.src_scale = src_scale.data_ptr()
    a.x = x2.data_ptr()
    a.out = out.data_ptr()
    arg = None
    if return_arg:
        arg = torch.empty(n_rows, F, dtype=rowptr.dtype, device=x.device)
        a.arg_out = arg.data_ptr()
    arg32 = None
    if save_arg32 and red in (_lib.MIN, _lib.MAX):
        arg32 = torch.empty(n_rows, F, dtype=torch.int32, device=x.device)
        a.arg32_out = arg32.data_ptr()
    a.n_rows, a.n_src, a.F = n_rows, x2.size(0), F
    a.ldx, a.ldo = _ld(x2), _ld(out)
    a.idx_dtype, a.reduce = _idx_dtype(rowptr), red
    a.w_heads, a.head_dim = w_heads, head_dim
    a.accumulate = 1 if accumulate else 0
    a.hub_phase = hub_phase
    if rowend is not None:
        a.rowend = rowend.data_ptr()
    a.accumulate_rows = int(accumulate_rows)
    if relu_mask is not None:
        m2 = _f32_rows(relu_mask, 'relu_mask')
        if tuple(m2.shape) != (n_rows, F):
            raise ValueError(f"'relu_mask' must be [{n_rows}, {F}], got {tuple(m2.shape)}")
        a.relu_mask, a.ld_mask = m2.data_ptr(), _ld(m2)
    if relu_bits is not None:
        _check_bits(relu_bits, n_rows, F)
        a.relu_bits, a.ld_bits = relu_bits.data_ptr(), relu_bits.size(1)
    if src_bits is not None:
        a.src_bits = src_bits.data_ptr()
        a.src_bits_set = 0 if src_bits_set is None else src_bits_set.data_ptr()
    _hub_args(a, hub)
    ws, ws_bytes = None, 0
    # (min / max take the hub list only to schedule those rows first: no workspace)
    if a.n_hub > 0 and hub_phase != 1 and red in (_lib.SUM, _lib.MEAN):
        ws_bytes = a.n_chunks * F * 4
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    sink = timing_sink
    if sink is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(x.device))
    check(lib.pygamd_spmm_csr(ctypes.byref(a), _p(ws), ws_bytes, _stream(x)), 'spmm_csr')
    if sink is not None:
        ev1.record(torch.cuda.current_stream(x.device))
        nnz = (col.numel() if col is not None else x2.size(0))
        sink.append(({'n_rows': n_rows, 'n_src': x2.size(0), 'nnz': nnz, 'F': F,
                      'reduce': reduce, 'idx_bytes': rowptr.element_size(),
                      'weighted': w is not None, 'src_scale': src_scale is not None,
                      'accumulate': bool(accumulate), 'relu_mask': relu_mask is not None,
                      'relu_bits': relu_bits is not None, 'src_bits': src_bits is not None,
                      'n_hub': a.n_hub}, ev0, ev1))
    if save_arg32:
        return out, arg32
    return (out, arg) if return_arg else out


def compressed_pitch(F: int) -> int:
    """Row pitch (32-bit words) of a compressed block of ``F`` columns: 8 mask words + F values + 4
    words of slack for the 16-byte value loads, rounded up to 128-byte lines (288 for F = 256)."""
    return (8 + F + 4 + 31) // 32 * 32


def _check_compressed(z: Tensor, F: int, name: str):
    if (z.dim() != 2 or z.dtype != torch.int32 or (z.size(0) > 1 and z.stride(0) < F + 12)
            or (z.size(1) > 1 and z.stride(1) != 1) or z.size(1) < F + 12):
        raise ValueError(f"'{name}' must be an int32 [n, >= {F + 12}] block of compressed rows")
    if F > 256 or F % 4 != 0:
        raise ValueError('compressed rows hold at most 256 columns, a multiple of 4')


def rows_compress(x: Tensor, out: Optional[Tensor] = None,
                  row_scale: Optional[Tensor] = None) -> Tensor:
    """``x`` ([n, F <= 256] float32) as compressed rows ``[8 mask words | kept values]`` — the
    lossless zero-skipping layout the row gathers read (``pygamd_rows_compress``).  ``row_scale``
    (float32, one entry per row): the rows of ``x * row_scale[:, None]`` instead, one fp32 multiply
    per element (``pygamd_rows_compress_scaled``)."""
    _require_device(x, out, row_scale)
    x2 = _f32_rows(x, 'x')
    n, F = x2.shape
    if F > 256:
        raise ValueError('compressed rows hold at most 256 columns')
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or row_scale.numel() != n:
            raise ValueError("'row_scale' must be float32 with one entry per row")
        row_scale = row_scale.contiguous()
    if out is None:
        out = torch.empty(n, compressed_pitch(F), dtype=torch.int32, device=x.device)
    elif (out.dim() != 2 or out.dtype != torch.int32 or out.size(0) != n or out.size(1) < F + 12
          or (out.size(1) > 1 and out.stride(1) != 1)):
        raise ValueError(f"'out' must be int32 [{n}, >= {F + 12}]")
    if row_scale is None:
        check(_lib.load().pygamd_rows_compress(_p(x2), _ld(x2), n, F, _p(out), _ld(out),
                                               _stream(x)), 'rows_compress')
    else:
        check(_lib.load().pygamd_rows_compress_scaled(_p(x2), _ld(x2), n, F, _p(row_scale),
                                                      _p(out), _ld(out), _stream(x)),
              'rows_compress')
    return out


def _spmm_csr_compressed(rowptr, col, z, reduce, F, n_rows, hub, out, hub_phase, rowend=None):
    _require_device(rowptr, col, z, out, rowend)
    if rowend is not None and (rowend.dtype != rowptr.dtype or not rowend.is_contiguous()
                               or n_rows is None or rowend.numel() < n_rows
                               or rowptr.numel() < n_rows):
        raise ValueError("'rowend' needs 'n_rows', the dtype of 'rowptr' and one entry per row")
    _check_compressed(z, F, 'x')
    if reduce not in ('sum', 'mean'):
        raise ValueError("compressed rows: reduce must be 'sum' or 'mean'")
    n_rows = rowptr.numel() - 1 if n_rows is None else n_rows
    if out is None:
        out = torch.empty(n_rows, F, dtype=torch.float32, device=z.device)
    a = SpmmArgs()
    a.rowptr = rowptr.data_ptr()
    a.col = 0 if col is None else col.data_ptr()
    a.x, a.out = z.data_ptr(), out.data_ptr()
    a.n_rows, a.n_src, a.F = n_rows, z.size(0), F
    a.ldx, a.ldo = _ld(z), _ld(out)
    a.idx_dtype, a.reduce = _idx_dtype(rowptr), REDUCE_IDS[reduce]
    a.w_heads, a.head_dim = 1, max(F, 1)
    a.hub_phase = hub_phase
    a.x_format = _lib.X_COMPRESSED
    if rowend is not None:
        a.rowend = rowend.data_ptr()
    _hub_args(a, hub)
    ws, ws_bytes = None, 0
    if a.n_hub > 0 and hub_phase != 1:
        ws_bytes = a.n_chunks * F * 4
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=z.device)
    sink = timing_sink
    if sink is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(z.device))
    check(_lib.load().pygamd_spmm_csr(ctypes.byref(a), _p(ws), ws_bytes, _stream(z)), 'spmm_csr')
    if sink is not None:
        ev1.record(torch.cuda.current_stream(z.device))
        sink.append(({'n_rows': n_rows, 'n_src': z.size(0), 'nnz': col.numel(), 'F': F,
                      'reduce': reduce, 'idx_bytes': rowptr.element_size(), 'weighted': False,
                      'src_scale': False, 'accumulate': False, 'compressed_src': True,
                      'n_hub': a.n_hub}, ev0, ev1))
    return out


def rows_pack(g: Tensor, row_scale: Optional[Tensor] = None, *, scaled: Optional[Tensor] = None,
              copy: Optional[Tensor] = None, count: bool = True):
    """(row_bits, n_set) of ``g`` ([n, F], unit column stride): bit i of ``row_bits`` (int32 words)
    = row i has a non-zero entry; ``n_set`` = one device int64 with the number of such rows (None
    with ``count=False``).  In the same pass: ``scaled[:, :F] = g * row_scale[:, None]`` and
    ``copy[:, :F] = g``, both zero-filled up to their own width (``pygamd_rows_pack``)."""
    _require_device(g, row_scale, scaled, copy)
    if g.dim() != 2 or g.dtype != torch.float32 or (g.size(1) > 1 and g.stride(1) != 1):
        raise ValueError("'g' must be a float32 matrix with unit column stride")
    n, F = g.shape
    for name, t in (('scaled', scaled), ('copy', copy)):
        if t is None:
            continue
        if (t.dim() != 2 or t.dtype != torch.float32 or t.size(0) != n or t.size(1) < F
                or (t.size(1) > 1 and t.stride(1) != 1)):
            raise ValueError(f"'{name}' must be float32 [{n}, >= {F}] with unit column stride")
        if t.data_ptr() == g.data_ptr() and n * F > 0:
            raise ValueError(f"'{name}' may not be 'g' itself")
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or row_scale.numel() != n:
            raise ValueError(f"'row_scale' must be {n} float32 values")
        row_scale = row_scale.contiguous()
    bits = torch.empty((n + 31) // 32, dtype=torch.int32, device=g.device)
    n_set = torch.empty(1, dtype=torch.int64, device=g.device) if count else None
    lib = _lib.load()
    check(lib.pygamd_rows_pack(_p(g), _ld(g), n, F, _p(row_scale), _p(scaled),
                               0 if scaled is None else _ld(scaled),
                               0 if scaled is None else scaled.size(1), _p(copy),
                               0 if copy is None else _ld(copy),
                               0 if copy is None else copy.size(1), _p(bits), _p(n_set),
                               _stream(g)), 'rows_pack')
    return bits, n_set


def live_lists_flag(bits: Tensor, stored: Tensor, n_src: int, flag: Tensor,
                    force: bool = False) -> None:
    """``flag[0] = [bits != stored]`` over ``n_src`` bits (1 as well when ``force``), decided on
    the device; ``stored`` then holds ``bits`` (``pygamd_live_lists_flag``)."""
    _require_device(bits, stored, flag)
    words = (n_src + 31) // 32
    for name, t in (('bits', bits), ('stored', stored)):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < words:
            raise ValueError(f"'{name}' must be contiguous int32 with one bit per row ({words} "
                             'words)')
    if flag.dtype != torch.int32 or flag.numel() != 1:
        raise ValueError("'flag' must be one int32")
    check(_lib.load().pygamd_live_lists_flag(_p(bits), _p(stored), n_src, int(bool(force)),
                                             _p(flag), _stream(bits)), 'live_lists_flag')


def live_lists_build(rowptr: Tensor, col: Tensor, n_src: int, live: Tensor, flag: Tensor, *,
                     hub=None, live2: Optional[Tensor] = None, n_set: Optional[Tensor] = None,
                     col_live: Optional[Tensor] = None, rowend_live: Optional[Tensor] = None,
                     row_has_live: Optional[Tensor] = None) -> None:
    """The live-source lists of a CSR handle into the caller's persistent buffers, or nothing at
    all when ``flag[0] == 0`` (``pygamd_live_lists_build``: a stable per-row partition by the bits
    ``live | live2``; rows longer than the plan's threshold and every row of a dense bitmap are
    copied whole)."""
    _require_device(rowptr, col, live, live2, n_set, flag, col_live, rowend_live, row_has_live)
    n_rows, words = rowptr.numel() - 1, (n_src + 31) // 32
    for name, t in (('live', live), ('live2', live2)):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()
                              or t.numel() < words):
            raise ValueError(f"'{name}' must be contiguous int32 with one bit per source row")
    if not rowptr.is_contiguous() or not col.is_contiguous() or col.dtype != rowptr.dtype:
        raise ValueError("'rowptr' / 'col' must be contiguous and share a dtype")
    if (col_live is None) != (rowend_live is None):
        raise ValueError("'col_live' and 'rowend_live' go together")
    if col_live is not None and (col_live.dtype != col.dtype or rowend_live.dtype != col.dtype
                                 or not col_live.is_contiguous()
                                 or not rowend_live.is_contiguous()
                                 or col_live.numel() < col.numel()
                                 or rowend_live.numel() < n_rows):
        raise ValueError("'col_live' / 'rowend_live' need the dtype of 'col', one slot per stored "
                         'entry and one end per row')
    if row_has_live is not None and (row_has_live.dtype != torch.int32
                                     or not row_has_live.is_contiguous()
                                     or row_has_live.numel() < (n_rows + 31) // 32):
        raise ValueError("'row_has_live' must be contiguous int32 with one bit per row")
    if flag.dtype != torch.int32 or flag.numel() != 1:
        raise ValueError("'flag' must be one int32")
    if n_set is not None and (n_set.dtype != torch.int64 or n_set.numel() != 1):
        raise ValueError("'n_set' must be one int64")
    threshold = hub.threshold if (hub is not None and hub.n_hub > 0) else 0
    check(_lib.load().pygamd_live_lists_build(
        _p(rowptr), _p(col), _idx_dtype(rowptr), n_rows, n_src, threshold, _p(live), _p(live2),
        _p(n_set), _p(flag), _p(col_live), _p(rowend_live), _p(row_has_live), _stream(rowptr)),
        'live_lists_build')


def live_lists_builds() -> int:
    """Builder launches that ran for real on this device so far (synchronises; test use only)."""
    n = ctypes.c_int64(0)
    check(_lib.load().pygamd_live_lists_builds(ctypes.byref(n)), 'live_lists_builds')
    return n.value


def multi_reduce_csr(rowptr: Tensor, perm: Optional[Tensor], x: Tensor, want):
    """{'sum' | 'pow_sum' | 'min' | 'max': [n_groups, F]} for the requested names in ONE read of the
    rows (group g = rows x[perm[k]], k in [rowptr[g], rowptr[g+1]); ``perm=None``: rows are already
    grouped)."""
    _require_device(rowptr, perm, x)
    lib = _lib.load()
    x2 = _f32_rows(x, 'x')
    n_rows, F = rowptr.numel() - 1, x2.size(1)
    names = ('sum', 'pow_sum', 'min', 'max')
    outs = {k: torch.empty(n_rows, F, dtype=torch.float32, device=x.device)
            for k in names if k in want}
    if perm is not None:
        perm = perm.contiguous()
        if perm.dtype != rowptr.dtype:
            perm = perm.to(rowptr.dtype)
    check(lib.pygamd_multi_reduce_csr(_p(rowptr), _p(perm), _idx_dtype(rowptr), _p(x2), _ld(x2),
                                      n_rows, F, *[_p(outs.get(k)) for k in names], max(F, 1),
                                      _stream(x)), 'multi_reduce_csr')
    return outs


def colsum(x: Tensor) -> Tensor:
    """x.sum(0) for a 2-D fp32 tensor (bias gradient)."""
    _require_device(x)
    lib = _lib.load()
    x2 = _f32_rows(x, 'x')
    out = torch.empty(x2.size(1), dtype=torch.float32, device=x.device)
    check(lib.pygamd_colsum(_p(x2), _ld(x2), x2.size(0), x2.size(1), _p(out), _stream(x)),
          'colsum')
    return out


def spmm_minmax_backward_dst(rowptr: Tensor, col: Optional[Tensor], x: Tensor, out: Tensor,
                             grad_out: Tensor, n_src: int, count_self: bool = True,
                             arg32: Optional[Tensor] = None) -> Tensor:
    """Gradient of the min/max aggregation w.r.t. ``x`` (reference tie rule) from the forward's
    destination-sorted handle.  With the forward's ``arg32`` the outputs with a unique extremum
    take the one-atomic fast path and only the marked ones the two-pass kernel."""
    _require_device(rowptr, col, x, out, grad_out, arg32)
    lib = _lib.load()
    x2, o2, g2 = _f32_rows(x, 'x'), _f32_rows(out, 'out'), _f32_rows(grad_out, 'grad_out')
    F = x2.size(1)
    grad_x = torch.empty(n_src, F, dtype=torch.float32, device=x.device)
    if arg32 is None:
        check(lib.pygamd_spmm_csr_minmax_backward_dst(
            _p(rowptr), _p(col), _idx_dtype(rowptr), _p(x2), _ld(x2), _p(o2), _ld(o2), _p(g2),
            _ld(g2), rowptr.numel() - 1, n_src, F, int(count_self), _p(grad_x), _ld(grad_x),
            _stream(x)), 'spmm_minmax_backward_dst')
    else:
        check(lib.pygamd_spmm_csr_minmax_backward_arg(
            _p(rowptr), _p(col), _idx_dtype(rowptr), _p(arg32.contiguous()), _p(x2), _ld(x2),
            _p(o2), _ld(o2), _p(g2), _ld(g2), rowptr.numel() - 1, n_src, F, int(count_self),
            _p(grad_x), _ld(grad_x), _stream(x)), 'spmm_minmax_backward_arg')
    return grad_x


def spmm_minmax_backward_src(fwd, bwd, slot_map: Tensor, x: Tensor, out: Tensor,
                             grad_out: Tensor, arg32: Tensor, count_self: bool = True
                             ) -> Optional[Tensor]:
    """The min/max gradient without the N x F scattered atomics (``pygamd_spmm_csr_minmax_backward_
    src``): ``fwd`` / ``bwd`` = the destination- / source-sorted CSR of the graph, ``slot_map`` =
    ``EdgeIndex.src_slot_to_dst_slot()``.  Returns ``None`` when the layout is not supported
    (``F % 4``, alignment): the caller then takes :func:`spmm_minmax_backward_dst`."""
    _require_device(fwd.ptr, fwd.idx, bwd.ptr, bwd.idx, slot_map, x, out, grad_out, arg32)
    lib = _lib.load()
    x2, o2, g2 = _f32_rows(x, 'x'), _f32_rows(out, 'out'), _f32_rows(grad_out, 'grad_out')
    F, n_src, nnz = x2.size(1), bwd.ptr.numel() - 1, bwd.idx.numel()
    if F % 4 or _ld(g2) % 4 or g2.data_ptr() % 16:
        return None
    grad_x = torch.empty(n_src, F, dtype=torch.float32, device=x.device)
    nbytes = lib.pygamd_minmax_backward_src_workspace_bytes(fwd.ptr.numel() - 1, nnz, F)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    a32 = arg32.contiguous()
    rc = lib.pygamd_spmm_csr_minmax_backward_src(
        _p(fwd.ptr), _p(fwd.idx), _p(bwd.ptr), _p(bwd.idx), _p(slot_map), _idx_dtype(fwd.ptr),
        _p(a32), _p(x2), _ld(x2), _p(o2), _ld(o2), _p(g2), _ld(g2), fwd.ptr.numel() - 1, n_src,
        nnz, F, int(count_self), _p(ws), nbytes, _p(grad_x), _ld(grad_x), _stream(x))
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    check(rc, 'spmm_minmax_backward_src')
    return grad_x


def bias_act(x: Tensor, bias: Optional[Tensor], relu: bool) -> Tensor:
    """``act(x + bias)`` as a new contiguous ``[n, F]`` tensor in one pass (``x`` may be a
    row-strided view)."""
    _require_device(x, bias)
    x2 = _f32_rows(x, 'x')
    out = torch.empty(x2.size(0), x2.size(1), dtype=torch.float32, device=x.device)
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != x2.size(1):
            raise ValueError(f"'bias' must be float32 with {x2.size(1)} entries")
        bias = bias.contiguous()
    check(_lib.load().pygamd_bias_act(_p(x2), _ld(x2), _p(bias), x2.size(0), x2.size(1),
                                      int(relu), _p(out), _ld(out), _stream(x)), 'bias_act')
    return out


def relu_backward_colsum(grad: Tensor, act: Tensor, want_colsum: bool = True):
    """(grad * (act > 0) as a new contiguous tensor, its column sums | None) in one pass; ``act``
    is the ReLU output.  Inputs may be row-strided views."""
    _require_device(grad, act)
    lib = _lib.load()
    g2, a2 = _f32_rows(grad, 'grad'), _f32_rows(act, 'act')
    if g2.shape != a2.shape:
        raise ValueError(f'shape mismatch: {tuple(g2.shape)} vs {tuple(a2.shape)}')
    out = torch.empty(g2.size(0), g2.size(1), dtype=torch.float32, device=grad.device)
    cs = torch.empty(g2.size(1), dtype=torch.float32, device=grad.device) if want_colsum else None
    check(lib.pygamd_relu_backward_colsum(_p(g2), _ld(g2), _p(a2), _ld(a2), g2.size(0),
                                          g2.size(1), _p(out), _ld(out), _p(cs), _stream(grad)),
          'relu_backward_colsum')
    return out, cs


def spmm_tie_count(rowptr, col, x, out, count_self: bool) -> Tensor:
    _require_device(rowptr, col, x, out)
    lib = _lib.load()
    x2, o2 = _f32_rows(x, 'x'), _f32_rows(out, 'out')
    ntie = torch.empty_like(o2, memory_format=torch.contiguous_format)
    o2 = o2.contiguous()
    check(lib.pygamd_spmm_csr_tie_count(_p(rowptr), _p(col), _idx_dtype(rowptr), _p(x2), _ld(x2),
                                        _p(o2), _ld(o2), o2.size(0), o2.size(1),
                                        1 if count_self else 0, _p(ntie), _stream(x)),
          'spmm_tie_count')
    return ntie


def spmm_minmax_backward(rowptr_t, col_t, x, out, grad_out, ntie) -> Tensor:
    _require_device(rowptr_t, col_t, x, out, grad_out, ntie)
    lib = _lib.load()
    x2 = _f32_rows(x, 'x')
    o2, g2, n2 = out.contiguous(), grad_out.contiguous(), ntie.contiguous()
    grad_x = torch.empty(x2.size(0), x2.size(1), dtype=torch.float32, device=x.device)
    check(lib.pygamd_spmm_csr_minmax_backward(_p(rowptr_t), _p(col_t), _idx_dtype(rowptr_t),
                                              _p(x2), _ld(x2), _p(o2), _p(g2), _p(n2), _ld(o2),
                                              x2.size(0), x2.size(1), _p(grad_x), _ld(grad_x),
                                              _stream(x)), 'spmm_minmax_backward')
    return grad_x


def sddmm_csr(rowptr, col, eid, grad_out, x, n_edges: int, w_heads: int) -> Tensor:
    _require_device(rowptr, col, eid, grad_out, x)
    C = _compiled.ops()
    if C is not None and _plain(grad_out, x):
        return C.sddmm_csr(rowptr, col, eid, grad_out, x, n_edges, w_heads)
    lib = _lib.load()
    g2, x2 = _f32_rows(grad_out, 'grad_out'), _f32_rows(x, 'x')
    F = x2.size(1)
    grad_w = torch.zeros(n_edges, w_heads, dtype=torch.float32, device=x.device)
    check(lib.pygamd_sddmm_csr(_p(rowptr), _p(col), _p(eid), _idx_dtype(rowptr), _p(g2), _ld(g2),
                               _p(x2), _ld(x2), rowptr.numel() - 1, F, w_heads,
                               F // max(w_heads, 1), _p(grad_w), _stream(x)), 'sddmm_csr')
    return grad_w


def sddmm_spmm_csr(rowptr, col, eid, rows, x, w, n_edges: int, w_heads: int):
    """(grad_w [n_edges, w_heads], agg [n_rows, F]) from ONE gather of ``x[col[k]]``:
    ``grad_w[e(k), h] = <rows[r, head h], x[col[k], head h]>`` and
    ``agg[r] = sum_k w[e(k), head] * x[col[k]]`` (``pygamd_sddmm_spmm_csr``)."""
    _require_device(rowptr, col, eid, rows, x, w)
    lib = _lib.load()
    r2, x2 = _f32_rows(rows, 'rows'), _f32_rows(x, 'x')
    F = x2.size(1)
    if r2.size(1) != F:
        raise ValueError("'rows' and 'x' must have the same width")
    w2 = w.reshape(-1, w_heads).contiguous()
    if w2.dtype != torch.float32 or w2.size(0) < n_edges:
        raise ValueError("'w' must hold one float32 weight per edge and head")
    n_rows = rowptr.numel() - 1
    agg = torch.empty(n_rows, F, dtype=torch.float32, device=x.device)
    # One 64-lane pass of 16-byte lanes covers 256 columns: every head's dot product is then
    # finished inside the wave and stored.  Wider rows, or rows that only take 4-byte lanes
    # (unaligned views), are covered by several lane groups whose partial sums meet in atomic adds
    # on a zeroed buffer.
    one_pass = (F % 4 == 0 and F <= 256 and (F // max(w_heads, 1)) % 4 == 0
                and all(t.data_ptr() % 16 == 0 and _ld(t) % 4 == 0 for t in (r2, x2, agg)))
    alloc = torch.empty if one_pass else torch.zeros
    grad_w = alloc(n_edges, w_heads, dtype=torch.float32, device=x.device)
    check(lib.pygamd_sddmm_spmm_csr(_p(rowptr), _p(col), _p(eid), _idx_dtype(rowptr), _p(r2),
                                    _ld(r2), _p(x2), _ld(x2), n_rows, F, w_heads,
                                    F // max(w_heads, 1), _p(w2), _p(grad_w), _p(agg), _ld(agg),
                                    _stream(x)), 'sddmm_spmm_csr')
    return grad_w, agg


# ---- unsorted gather / scatter ----------------------------------------------------------------
class IndexOutOfRange(PygAmdError, IndexError):
    """An index outside [0, size) reached a scatter/gather kernel (the reference's ATen CPU
    kernels raise 'index ... is out of bounds' at the same place)."""


# How the error flag of the scatter kernels reaches the host:
#   'async' (default)  the flag is copied to pinned host memory behind the kernel and looked at —
#                      without waiting — at the next scatter call or by `check_index_errors()`
#                      (the reference's GPU path reports such indices as an asynchronous device
#                      assert too; a per-call blocking read would serialise host and device on
#                      every scatter / degree / aggregation forward);
#   'sync'             one blocking 4-byte read per call (raises at the call site);
#   'off'              the kernels still skip such rows, nothing is reported.
INDEX_CHECK = os.environ.get('PYGAMD_CHECK_INDEX', 'async')


class _FlagRing:
    """256 device flags + their pinned host mirrors, handed out round-robin per device."""
    SLOTS = 256

    def __init__(self, device):
        self.dev = torch.zeros(self.SLOTS, dtype=torch.int32, device=device)
        self.host = torch.zeros(self.SLOTS, dtype=torch.int32).pin_memory()
        self.next = 0
        self.pending = collections.deque()  # (slot, event, what, size, index, style)

    def acquire(self) -> int:
        slot = self.next
        self.next = (self.next + 1) % self.SLOTS
        while self.pending and self.pending[0][0] == slot:  # the ring wrapped: wait for the oldest
            self.pending[0][1].synchronize()
            self.poll()
        return slot

    def publish(self, slot: int, what: str, size: int, index: Tensor, on_flag=None, report=None):
        """``on_flag``: called (before the error is raised) when this launch turns out flagged —
        lets the owner of a CACHED object built from ``index`` (a sorted-scatter plan) remember
        it, so that later uses of the cache report the same indices again.  ``report``: raises
        the error of a flagged launch in place of the ``[0, size)`` report over ``index`` (a
        launch whose indices have no single bound: :func:`hetero_spmm`)."""
        self.host[slot:slot + 1].copy_(self.dev[slot:slot + 1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev.device))
        self.pending.append((slot, ev, what, size, index, _error_style.value, on_flag, report))

    def poll(self, wait: bool = False):
        while self.pending:
            slot, ev, what, size, index, style, on_flag, report = self.pending[0]
            if wait:
                ev.synchronize()
            elif not ev.query():
                return
            self.pending.popleft()
            if int(self.host[slot]) != 0:
                self.host[slot] = 0
                self.dev[slot:slot + 1].zero_()
                if on_flag is not None:
                    on_flag()
                if report is not None:
                    report()
                _raise_out_of_range(index, size, what, style)


_flag_rings = {}


def _flag_ring(device) -> _FlagRing:
    ring = _flag_rings.get(device)
    if ring is None:
        ring = _flag_rings[device] = _FlagRing(device)
    return ring


def check_index_errors():
    """Waits for every scatter launched so far (on any device) and raises `IndexOutOfRange` if one
    of them met an index outside ``[0, dim_size)`` (see ``INDEX_CHECK``)."""
    for ring in list(_flag_rings.values()):
        ring.poll(wait=True)


# 'dim_size' while an `Aggregation.__call__` is running: a flagged launch is then reported the way
# the reference's wrapper reports it (nn/aggr/base.py:131-141), whenever the flag arrives.  Per
# thread (a DataLoader worker thread's aggregation must not restyle another thread's error) and
# recorded per launch by `_FlagRing.publish`.
class _ErrorStyle(threading.local):
    value = None


_error_style = _ErrorStyle()


def set_error_style(style):
    """Sets this thread's report style for flagged launches; returns the previous one."""
    prev, _error_style.value = _error_style.value, style
    return prev


def _index_flag(device, active: bool):
    """(ring, slot, flag tensor or None) for one index-checking launch, per ``INDEX_CHECK``."""
    if not active or INDEX_CHECK == 'off':
        return None, None, None
    if INDEX_CHECK == 'async' and not torch.cuda.is_current_stream_capturing():
        ring = _flag_ring(device)
        ring.poll()  # raises for an EARLIER launch whose flag has arrived meanwhile
        slot = ring.acquire()
        return ring, slot, ring.dev[slot:slot + 1]
    return None, None, torch.zeros(1, dtype=torch.int32, device=device)


def _index_flag_done(ring, slot, err, what: str, size: int, index: Tensor, on_flag=None):
    if ring is not None:
        ring.publish(slot, what, size, index, on_flag)
    elif err is not None and INDEX_CHECK == 'sync':
        try:
            _raise_if_flagged(err, index, size, what)
        except IndexError:
            if on_flag is not None:
                on_flag()
            raise


def poll_index_errors(wait: bool = False, device=None):
    """Looks at the flags that have arrived (``wait=True``: at all of them, blocking) and raises
    for the first flagged launch.  ``device``: only that device's ring (a caller that knows where
    its launch ran does not touch — or wait on — the other GPUs' rings).  Called at the entry of
    the scatter backward and at the end of an ``Aggregation`` call with a caller-supplied
    ``dim_size``."""
    if device is not None:
        ring = _flag_rings.get(torch.device(device))
        if ring is not None:
            ring.poll(wait=wait)
        return
    for ring in list(_flag_rings.values()):
        ring.poll(wait=wait)


def _raise_out_of_range(index: Tensor, size: int, what: str, style=None):
    lo, hi = index_minmax(index)
    if style == 'edge_index':  # the texts of MessagePassing._index_select_safe
        if lo < 0:
            raise IndexError(
                f"Found negative indices in 'edge_index' (got {lo}). Please ensure that all "
                f"indices in 'edge_index' point to valid indices in the interval [0, {size}) in "
                f"your node feature matrix and try again.")
        raise IndexError(
            f"Found indices in 'edge_index' that are larger than {size - 1} (got {hi}). Please "
            f"ensure that all indices in 'edge_index' point to valid indices in the interval "
            f"[0, {size}) in your node feature matrix and try again.")
    if style == 'dim_size' and size <= hi:
        raise ValueError(f"Encountered invalid 'dim_size' (got '{size}' but expected "
                         f">= '{hi + 1}')")
    bad = hi if hi >= size else lo
    raise IndexOutOfRange(f'{what}: index {bad} is out of bounds for dimension 0 with size '
                          f'{size} (indices span [{lo}, {hi}])')


def _raise_if_flagged(err: Tensor, index: Tensor, size: int, what: str):
    """One 4-byte host read of the kernel's error flag ('sync' mode).  Skipped while the stream is
    being captured into a hipGraph (no sync allowed there; the kernels still skip such rows)."""
    if torch.cuda.is_current_stream_capturing():
        return
    if int(err.item()) != 0:
        style = _error_style.value
        _raise_out_of_range(index, size, what, style if style == 'edge_index' else None)


def gather_rows(x: Tensor, index: Tensor, check_bounds=False) -> Tensor:
    """``x[index]`` for float32 rows.  ``check_bounds``: ``False`` (the caller vouches for the
    index), ``True`` (one blocking flag read, IndexError at the call) or ``'edge_index'`` — the
    gather of ``MessagePassing._index_select``: the reference's IndexError texts
    (message_passing.py:269-290), delivered as ``INDEX_CHECK`` says (async flag ring / blocking
    read / not at all); flagged rows are skipped by the kernel in every mode."""
    _require_device(x, index)
    as_edges = check_bounds == 'edge_index'
    if as_edges and INDEX_CHECK == 'off':
        as_edges = check_bounds = False
    C = _compiled.ops()
    if C is not None and not check_bounds and _plain(x) \
            and index.dtype in (torch.int32, torch.int64):
        return C.gather_rows(x, index)
    lib = _lib.load()
    x2 = _f32_rows(x, 'x')
    index = index.contiguous()
    n, F = index.numel(), x2.size(1)
    out = torch.empty(n, F, dtype=torch.float32, device=x.device)
    ring = slot = None
    if as_edges:
        ring, slot, err = _index_flag(x.device, n > 0 and F > 0)
    else:
        err = torch.zeros(1, dtype=torch.int32, device=x.device) if check_bounds else None
    check(lib.pygamd_gather_rows(_p(x2), _ld(x2), x2.size(0), _p(index), _idx_dtype(index), n, F,
                                 _p(out), _ld(out), _p(err), _stream(x)), 'gather_rows')
    if as_edges:
        prev = set_error_style('edge_index')
        try:
            _index_flag_done(ring, slot, err, 'gather', x2.size(0), index)
        finally:
            set_error_style(prev)
        return out
    if check_bounds and int(err.item()) != 0:
        lo, hi = index_minmax(index)
        raise IndexError(
            f"Found indices in 'edge_index' outside the valid range [0, {x2.size(0) - 1}] "
            f"(got interval [{lo}, {hi}])")
    return out


def scatter_rows(src: Tensor, index: Tensor, dim_size: int, reduce: str,
                 return_count: bool = False):
    _require_device(src, index)
    lib = _lib.load()
    s2 = _f32_rows(src, 'src')
    index = index.contiguous()
    n, F = index.numel(), s2.size(1)
    red = REDUCE_IDS[reduce]
    out = torch.empty(dim_size, F, dtype=torch.float32, device=src.device)
    need_count = red in (_lib.MEAN, _lib.MIN, _lib.MAX)
    count = torch.empty(dim_size, dtype=torch.float32, device=src.device) if need_count else None
    st = _stream(src)
    check(lib.pygamd_scatter_init(_p(out), _ld(out), dim_size, F, red, _p(count), st),
          'scatter_init')
    capturing = torch.cuda.is_current_stream_capturing()
    ring = slot = None
    if INDEX_CHECK == 'async' and not capturing and n > 0 and F > 0:
        ring = _flag_ring(src.device)
        ring.poll()  # raises for an EARLIER launch whose flag has arrived meanwhile
        slot = ring.acquire()
        err = ring.dev[slot:slot + 1]
    else:
        err = torch.zeros(1, dtype=torch.int32, device=src.device)
    check(lib.pygamd_scatter_rows(_p(s2), _ld(s2), _p(index), _idx_dtype(index), n, F, _p(out),
                                  _ld(out), dim_size, red, _p(count), _p(err), st), 'scatter_rows')
    if ring is not None:
        ring.publish(slot, 'scatter', dim_size, index)
    elif INDEX_CHECK == 'sync' and n > 0 and F > 0:
        # before anything is saved for a backward that would index with the same values
        _raise_if_flagged(err, index, dim_size, 'scatter')
    check(lib.pygamd_scatter_finalize(_p(out), _ld(out), dim_size, F, red, _p(count), st),
          'scatter_finalize')
    return (out, count) if return_count else out


def scatter_minmax_backward(src, index, out, grad_out) -> Tensor:
    _require_device(src, index, out, grad_out)
    lib = _lib.load()
    s2 = _f32_rows(src, 'src')
    o2, g2 = out.contiguous(), grad_out.contiguous()
    index = index.contiguous()
    n, F, dim_size = index.numel(), s2.size(1), o2.size(0)
    ntie = torch.empty_like(o2)
    st = _stream(src)
    check(lib.pygamd_scatter_minmax_tie_count(_p(s2), _ld(s2), _p(index), _idx_dtype(index), n, F,
                                              _p(o2), _ld(o2), dim_size, _p(ntie), st),
          'scatter_minmax_tie_count')
    grad_src = torch.empty(n, F, dtype=torch.float32, device=src.device)
    check(lib.pygamd_scatter_minmax_backward(_p(s2), _ld(s2), _p(index), _idx_dtype(index), n, F,
                                             _p(o2), _p(g2), _p(ntie), _ld(o2), dim_size,
                                             _p(grad_src), _ld(grad_src), st),
          'scatter_minmax_backward')
    return grad_src


def scatter_mul_backward(src, index, out, grad_out) -> Tensor:
    """Gradient of scatter(reduce='mul') w.r.t. ``src`` with ATen's zero-count rule."""
    _require_device(src, index, out, grad_out)
    lib = _lib.load()
    s2 = _f32_rows(src, 'src')
    o2, g2 = out.contiguous(), grad_out.contiguous()
    index = index.contiguous()
    n, F, dim_size = index.numel(), s2.size(1), o2.size(0)
    grad_src = torch.empty(n, F, dtype=torch.float32, device=src.device)
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_scatter_mul_backward_workspace_bytes(dim_size, F, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=src.device)
    check(lib.pygamd_scatter_mul_backward(_p(s2), _ld(s2), _p(index), _idx_dtype(index), n, F,
                                          _p(o2), _p(g2), _ld(o2) if dim_size else max(F, 1),
                                          dim_size, _p(grad_src), _ld(grad_src), _p(ws),
                                          nbytes.value, _stream(src)), 'scatter_mul_backward')
    return grad_src


def scatter_argmax(src: Tensor, index: Tensor, dim_size: int) -> Tensor:
    _require_device(src, index)
    lib = _lib.load()
    src = src.contiguous()
    index = index.contiguous()
    gmax = torch.empty(dim_size, dtype=torch.float32, device=src.device)
    arg = torch.empty(dim_size, dtype=index.dtype, device=src.device)
    check(lib.pygamd_scatter_argmax(_p(src), _p(index), _idx_dtype(index), index.numel(),
                                    dim_size, _p(gmax), _p(arg), _stream(src)), 'scatter_argmax')
    return arg


# ---- softmax ---------------------------------------------------------------------------------
def segment_softmax_forward(src: Tensor, ptr: Tensor) -> Tensor:
    _require_device(src, ptr)
    C = _compiled.ops()
    if C is not None and _plain(src):
        return C.segment_softmax_forward(src, ptr)
    lib = _lib.load()
    s2 = src.contiguous()
    out = torch.empty_like(s2)
    check(lib.pygamd_segment_softmax_forward(_p(s2), _p(ptr), _idx_dtype(ptr), ptr.numel() - 1,
                                             s2.size(1), _p(out), _stream(src)),
          'segment_softmax_forward')
    return out


def segment_softmax_backward(out: Tensor, grad_out: Tensor, ptr: Tensor) -> Tensor:
    _require_device(out, grad_out, ptr)
    C = _compiled.ops()
    if C is not None and _plain(out, grad_out):
        return C.segment_softmax_backward(out, grad_out, ptr)
    lib = _lib.load()
    o2, g2 = out.contiguous(), grad_out.contiguous()
    grad_src = torch.empty_like(o2)
    check(lib.pygamd_segment_softmax_backward(_p(o2), _p(g2), _p(ptr), _idx_dtype(ptr),
                                              ptr.numel() - 1, o2.size(1), _p(grad_src),
                                              _stream(out)), 'segment_softmax_backward')
    return grad_src


def softmax_index_forward(src: Tensor, index: Tensor, num_groups: int) -> Tensor:
    """Softmax of ``src [n, H]`` within the groups of an unsorted ``index`` (4 launches)."""
    _require_device(src, index)
    lib = _lib.load()
    s2, idx = src.contiguous(), index.contiguous()
    n, H = s2.shape
    out = torch.zeros_like(s2)
    ws = torch.empty(2 * max(num_groups, 1) * max(H, 1), dtype=torch.float32, device=src.device)
    # an index outside [0, num_groups) is skipped by the kernels and reported like a scatter's
    # (the reference's scatter / index_select path raises there, utils/_softmax.py:82-88)
    ring, slot, err = _index_flag(src.device, n > 0 and H > 0)
    check(lib.pygamd_softmax_index_forward(_p(s2), _p(idx), _idx_dtype(idx), n, H, num_groups,
                                           _p(ws), _p(out), _p(err), _stream(src)),
          'softmax_index_forward')
    _index_flag_done(ring, slot, err, 'softmax', num_groups, idx)
    return out


def softmax_index_backward(out: Tensor, grad_out: Tensor, index: Tensor,
                           num_groups: int) -> Tensor:
    _require_device(out, grad_out, index)
    lib = _lib.load()
    o2, g2, idx = out.contiguous(), grad_out.contiguous(), index.contiguous()
    n, H = o2.shape
    grad_src = torch.empty_like(o2)
    ws = torch.empty(max(num_groups, 1) * max(H, 1), dtype=torch.float32, device=out.device)
    check(lib.pygamd_softmax_index_backward(_p(o2), _p(g2), _p(idx), _idx_dtype(idx), n, H,
                                            num_groups, _p(ws), _p(grad_src), _stream(out)),
          'softmax_index_backward')
    return grad_src


def segment_logsumexp_forward(src: Tensor, ptr: Tensor) -> Tensor:
    _require_device(src, ptr)
    lib = _lib.load()
    s2 = src.contiguous()
    out = torch.empty(ptr.numel() - 1, s2.size(1), dtype=torch.float32, device=src.device)
    check(lib.pygamd_segment_logsumexp_forward(_p(s2), _p(ptr), _idx_dtype(ptr), ptr.numel() - 1,
                                               s2.size(1), _p(out), _stream(src)),
          'segment_logsumexp_forward')
    return out


def segment_logsumexp_backward(src: Tensor, out: Tensor, grad_out: Tensor, ptr: Tensor) -> Tensor:
    _require_device(src, out, grad_out, ptr)
    lib = _lib.load()
    s2, o2, g2 = src.contiguous(), out.contiguous(), grad_out.contiguous()
    grad_src = torch.empty_like(s2)
    check(lib.pygamd_segment_logsumexp_backward(_p(s2), _p(o2), _p(g2), _p(ptr), _idx_dtype(ptr),
                                                ptr.numel() - 1, s2.size(1), _p(grad_src),
                                                _stream(src)), 'segment_logsumexp_backward')
    return grad_src


def gat_edge_softmax_forward(rowptr, col, alpha_src, alpha_dst, slope: float) -> Tensor:
    _require_device(rowptr, col, alpha_src, alpha_dst)
    lib = _lib.load()
    a_s, a_d = alpha_src.contiguous(), alpha_dst.contiguous()
    H = a_s.size(1)
    out = torch.empty(col.numel(), H, dtype=torch.float32, device=a_s.device)
    check(lib.pygamd_gat_edge_softmax_forward(_p(rowptr), _p(col), _idx_dtype(rowptr), _p(a_s),
                                              _p(a_d), rowptr.numel() - 1, H, float(slope),
                                              _p(out), _stream(a_s)), 'gat_edge_softmax_forward')
    return out


def gat_edge_softmax_backward(rowptr, col, alpha_src, alpha_dst, alpha, grad_alpha, slope: float):
    _require_device(rowptr, col, alpha_src, alpha_dst, alpha, grad_alpha)
    lib = _lib.load()
    a_s, a_d = alpha_src.contiguous(), alpha_dst.contiguous()
    al, g = alpha.contiguous(), grad_alpha.contiguous()
    H = a_s.size(1)
    g_src = torch.zeros_like(a_s)
    g_dst = torch.zeros_like(a_d)
    check(lib.pygamd_gat_edge_softmax_backward(_p(rowptr), _p(col), _idx_dtype(rowptr), _p(a_s),
                                               _p(a_d), _p(al), _p(g), rowptr.numel() - 1, H,
                                               float(slope), _p(g_src), _p(g_dst),
                                               _stream(a_s)), 'gat_edge_softmax_backward')
    return g_src, g_dst


# ---- GATv2 attention (csrc/gatv2.hip) ------------------------------------------------------------
def gatv2_supported(H: int, C: int) -> bool:
    """The one-pass kernels serve this head layout (H * C <= 512, H <= 64)."""
    return bool(_lib.load().pygamd_gatv2_supported(int(H), int(C)))


def gatv2_forward(rowptr: Tensor, col: Tensor, x_l: Tensor, x_r: Tensor, att: Tensor, H: int,
                  C: int, slope: float, *, hub=None, aggregate: bool = True):
    """``(alpha [nnz, H] in slot order, out [n_rows, H * C] | None)`` of one GATv2 attention step
    on a by-destination handle; ``aggregate=False`` is the score mode (alpha only)."""
    _require_device(rowptr, col, x_l, x_r, att)
    lib = _lib.load()
    W = H * C
    x_l, x_r = _dense_rows(x_l, 'x_l', W), _dense_rows(x_r, 'x_r', W)
    att = att.reshape(-1).contiguous()
    n_rows = rowptr.numel() - 1
    if att.numel() != W or x_r.size(0) < n_rows:
        raise ValueError(f"'att' needs {W} entries and 'x_r' at least {n_rows} rows")
    g = _csr(rowptr, col, n_rows, hub)
    alpha = torch.empty(col.numel(), H, dtype=torch.float32, device=x_l.device)
    out = torch.empty(n_rows, W, dtype=torch.float32, device=x_l.device) if aggregate else None
    if col.numel() == 0:  # no edges: every row is empty
        return alpha, (out.zero_() if aggregate else None)
    ws, ws_bytes = _workspace(lib.pygamd_gatv2_workspace_bytes, (g.n_chunks, H, C), x_l.device,
                              g.n_chunks > 0)
    with _timed({'kind': 'gatv2', 'op': 'forward' if aggregate else 'score', 'n_rows': n_rows,
                 'E': col.numel(), 'H': H, 'C': C, 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, x_l):
        check(lib.pygamd_gatv2_forward(ctypes.byref(g), _p(x_l), _p(x_r), _p(att), x_l.size(0), H,
                                       C, float(slope), _p(alpha), _p(out), _p(ws), ws_bytes,
                                       _stream(x_l)), 'gatv2_forward')
    return alpha, out


def gatv2_backward_dst(rowptr: Tensor, col: Tensor, x_l: Tensor, x_r: Tensor, att: Tensor,
                       alpha: Tensor, H: int, C: int, slope: float, *,
                       grad_out: Optional[Tensor] = None, out: Optional[Tensor] = None,
                       grad_alpha: Optional[Tensor] = None, hub=None):
    """``(grad_s [nnz, H], grad_x_r [rows of x_r, H * C], grad_att [H * C])``; ``grad_alpha``
    given = score mode, otherwise ``grad_out`` and ``out``."""
    _require_device(rowptr, col, x_l, x_r, att, alpha, grad_out, out, grad_alpha)
    lib = _lib.load()
    W = H * C
    x_l, x_r = _dense_rows(x_l, 'x_l', W), _dense_rows(x_r, 'x_r', W)
    att, alpha = att.reshape(-1).contiguous(), alpha.contiguous()
    n_rows = rowptr.numel() - 1
    if grad_alpha is None:
        grad_out, out = _dense_rows(grad_out, 'grad_out', W), _dense_rows(out, 'out', W)
    else:
        grad_alpha = grad_alpha.contiguous()
    g = _csr(rowptr, col, n_rows, hub)
    grad_s = torch.empty_like(alpha)
    grad_x_r = _grad_rows(x_r.size(0), n_rows, W, x_l.device)
    grad_att = torch.empty(W, dtype=torch.float32, device=x_l.device)
    if col.numel() == 0:
        return grad_s, grad_x_r.zero_(), grad_att.zero_()
    ws, ws_bytes = _workspace(lib.pygamd_gatv2_workspace_bytes, (g.n_chunks, H, C), x_l.device)
    with _timed({'kind': 'gatv2', 'op': 'backward_dst', 'n_rows': n_rows, 'E': col.numel(),
                 'H': H, 'C': C, 'n_hub': g.n_hub, 'score': grad_alpha is not None}, x_l):
        check(lib.pygamd_gatv2_backward_dst(
            ctypes.byref(g), _p(x_l), _p(x_r), _p(att), _p(alpha), _p(grad_out), _p(out),
            _p(grad_alpha), x_l.size(0), H, C, float(slope), _p(grad_s), _p(grad_x_r),
            _p(grad_att), _p(ws), ws_bytes, _stream(x_l)), 'gatv2_backward_dst')
    return grad_s, grad_x_r, grad_att


def gatv2_backward_src(rowptr_t: Tensor, col_t: Tensor, slot_map: Tensor, x_l: Tensor,
                       x_r: Tensor, att: Tensor, alpha: Tensor, grad_s: Tensor, H: int, C: int,
                       slope: float, *, grad_out: Optional[Tensor] = None, n_dst: int,
                       hub=None) -> Tensor:
    """``grad_x_l [n_src, H * C]`` on the by-source handle; ``grad_out=None`` = score mode."""
    _require_device(rowptr_t, col_t, slot_map, x_l, x_r, att, alpha, grad_s, grad_out)
    lib = _lib.load()
    W = H * C
    x_l, x_r = _dense_rows(x_l, 'x_l', W), _dense_rows(x_r, 'x_r', W)
    att, alpha, grad_s = att.reshape(-1).contiguous(), alpha.contiguous(), grad_s.contiguous()
    if grad_out is not None:
        grad_out = _dense_rows(grad_out, 'grad_out', W)
    n_src = rowptr_t.numel() - 1
    if x_l.size(0) != n_src or slot_map.dtype != rowptr_t.dtype:
        raise ValueError("'x_l' must have one row per source and 'slot_map' the index dtype")
    slot_map = slot_map.contiguous()
    g = _csr(rowptr_t, col_t, n_src, hub)
    grad_x_l = torch.empty(n_src, W, dtype=torch.float32, device=x_l.device)
    if col_t.numel() == 0:
        return grad_x_l.zero_()
    ws, ws_bytes = _workspace(lib.pygamd_gatv2_workspace_bytes, (g.n_chunks, H, C), x_l.device,
                              g.n_chunks > 0)
    with _timed({'kind': 'gatv2', 'op': 'backward_src', 'n_rows': n_src, 'E': col_t.numel(),
                 'H': H, 'C': C, 'n_hub': g.n_hub, 'score': grad_out is None}, x_l):
        check(lib.pygamd_gatv2_backward_src(
            ctypes.byref(g), _p(slot_map), _p(x_l), _p(x_r), _p(att), _p(alpha), _p(grad_s),
            _p(grad_out), n_dst, H, C, float(slope), _p(grad_x_l), _p(ws), ws_bytes,
            _stream(x_l)), 'gatv2_backward_src')
    return grad_x_l


# ---- HAN's typed additive attention (csrc/han.hip) -----------------------------------------------
def han_supported(H: int, C: int) -> bool:
    """The one-pass kernels serve this head layout (H * C <= 512, H <= 64)."""
    return bool(_lib.load().pygamd_han_supported(int(H), int(C)))


def _han_types(row_begin, val_shift, n_rows: int):
    """The host arrays of the kernels' by-value type table."""
    n_et = len(val_shift)
    if not 1 <= n_et <= MAX_HETERO_TYPES or len(row_begin) != n_et + 1:
        raise ValueError(f"'row_begin' needs one entry more than 'val_shift', which needs 1 to "
                         f"{MAX_HETERO_TYPES} (got {len(row_begin)} and {n_et})")
    if row_begin[0] != 0 or row_begin[-1] != n_rows or list(row_begin) != sorted(row_begin):
        raise ValueError(f"'row_begin' must rise from 0 to the {n_rows} rows of the handle")
    return ((ctypes.c_int64 * (n_et + 1))(*[int(v) for v in row_begin]),
            (ctypes.c_int64 * n_et)(*[int(v) for v in val_shift]), n_et)


def han_forward(rowptr: Tensor, col: Tensor, row_begin, val_shift, x_all: Tensor, a_src: Tensor,
                a_dst: Tensor, H: int, C: int, slope: float, relu: bool, *, hub=None):
    """``(alpha [nnz, H] in slot order, out [n_rows, H * C])`` of HAN's node-level attention for
    every edge type of a call on the stacked by-destination handle (``row_begin``, ``val_shift``:
    sequences of ints, see pygamd_han_forward).  The caller has range-checked the ids: column ``c``
    of edge type ``e`` reads row ``c + val_shift[e]`` of ``x_all``."""
    _require_device(rowptr, col, x_all, a_src, a_dst)
    lib = _lib.load()
    W = H * C
    x_all = _dense_rows(x_all, 'x_all', W)
    a_src, a_dst = _dense_rows(a_src, 'a_src', H), _dense_rows(a_dst, 'a_dst', H)
    n_rows = rowptr.numel() - 1
    if a_dst.size(0) != n_rows:
        raise ValueError(f"'a_dst' needs one row per row of the handle ({n_rows})")
    alpha = torch.empty(col.numel(), H, dtype=torch.float32, device=x_all.device)
    out = torch.empty(n_rows, W, dtype=torch.float32, device=x_all.device)
    if col.numel() == 0:  # no edges: every row is empty
        return alpha, out.zero_()
    rb, vs, n_et = _han_types(row_begin, val_shift, n_rows)
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_han_workspace_bytes, (g.n_chunks, H, C), x_all.device,
                              g.n_chunks > 0)
    with _timed({'kind': 'han', 'op': 'forward', 'n_rows': n_rows, 'E': col.numel(), 'H': H,
                 'C': C, 'n_et': n_et, 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, x_all):
        check(lib.pygamd_han_forward(ctypes.byref(g), rb, vs, n_et, _p(x_all), _p(a_src),
                                     _p(a_dst), a_src.size(0), H, C, float(slope), int(relu),
                                     _p(alpha), _p(out), _p(ws), ws_bytes, _stream(x_all)),
              'han_forward')
    return alpha, out


def han_backward_dst(rowptr: Tensor, col: Tensor, row_begin, val_shift, x_all: Tensor,
                     a_src: Tensor, a_dst: Tensor, alpha: Tensor, grad_out: Tensor, out: Tensor,
                     H: int, C: int, slope: float, relu: bool, *, hub=None):
    """``(grad_s [nnz, H] in slot order, grad_a_dst [n_rows, H])``"""
    _require_device(rowptr, col, x_all, a_src, a_dst, alpha, grad_out, out)
    lib = _lib.load()
    W = H * C
    x_all = _dense_rows(x_all, 'x_all', W)
    a_src, a_dst = _dense_rows(a_src, 'a_src', H), _dense_rows(a_dst, 'a_dst', H)
    grad_out, out = _dense_rows(grad_out, 'grad_out', W), _dense_rows(out, 'out', W)
    alpha = alpha.contiguous()
    n_rows = rowptr.numel() - 1
    if a_dst.size(0) != n_rows or out.size(0) != n_rows or grad_out.size(0) != n_rows:
        raise ValueError(f"'a_dst', 'out' and 'grad_out' need one row per row of the handle "
                         f"({n_rows})")
    grad_s = torch.empty_like(alpha)
    grad_a_dst = torch.empty(n_rows, H, dtype=torch.float32, device=x_all.device)
    if col.numel() == 0:
        return grad_s, grad_a_dst.zero_()
    rb, vs, n_et = _han_types(row_begin, val_shift, n_rows)
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_han_workspace_bytes, (g.n_chunks, H, C), x_all.device,
                              g.n_chunks > 0)
    with _timed({'kind': 'han', 'op': 'backward_dst', 'n_rows': n_rows, 'E': col.numel(), 'H': H,
                 'C': C, 'n_et': n_et, 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, x_all):
        check(lib.pygamd_han_backward_dst(
            ctypes.byref(g), rb, vs, n_et, _p(x_all), _p(a_src), _p(a_dst), _p(alpha),
            _p(grad_out), _p(out), a_src.size(0), H, C, float(slope), int(relu), _p(grad_s),
            _p(grad_a_dst), _p(ws), ws_bytes, _stream(x_all)), 'han_backward_dst')
    return grad_s, grad_a_dst


def han_backward_src(rowptr_t: Tensor, col_t: Tensor, slot_map: Tensor, alpha: Tensor,
                     grad_s: Tensor, grad_out: Tensor, out: Tensor, H: int, C: int, relu: bool, *,
                     hub=None):
    """``(grad_a_src [n_cols, H], grad_xv [n_cols, H * C])`` on the by-source handle, whose rows
    are the stacked (edge type, source) columns of the forward."""
    _require_device(rowptr_t, col_t, slot_map, alpha, grad_s, grad_out, out)
    lib = _lib.load()
    W = H * C
    grad_out, out = _dense_rows(grad_out, 'grad_out', W), _dense_rows(out, 'out', W)
    alpha, grad_s = alpha.contiguous(), grad_s.contiguous()
    n_cols = rowptr_t.numel() - 1
    if slot_map.dtype != rowptr_t.dtype or grad_out.size(0) != out.size(0):
        raise ValueError("'slot_map' must have the index dtype and 'grad_out' the rows of 'out'")
    slot_map = slot_map.contiguous()
    grad_a_src = torch.empty(n_cols, H, dtype=torch.float32, device=out.device)
    grad_xv = torch.empty(n_cols, W, dtype=torch.float32, device=out.device)
    if col_t.numel() == 0:
        return grad_a_src.zero_(), grad_xv.zero_()
    g = _csr(rowptr_t, col_t, n_cols, hub)
    ws, ws_bytes = _workspace(lib.pygamd_han_workspace_bytes, (g.n_chunks, H, C), out.device,
                              g.n_chunks > 0)
    with _timed({'kind': 'han', 'op': 'backward_src', 'n_rows': n_cols, 'E': col_t.numel(),
                 'H': H, 'C': C, 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, out):
        check(lib.pygamd_han_backward_src(
            ctypes.byref(g), _p(slot_map), _p(alpha), _p(grad_s), _p(grad_out), _p(out),
            out.size(0), H, C, int(relu), _p(grad_a_src), _p(grad_xv), _p(ws), ws_bytes,
            _stream(out)), 'han_backward_src')
    return grad_a_src, grad_xv


# ---- TransformerConv's dot-product attention (csrc/transformer.hip) ------------------------------
def transformer_supported(H: int, C: int) -> bool:
    """The one-pass kernels serve this head layout (H * C <= 512, H <= 64)."""
    return bool(_lib.load().pygamd_transformer_supported(int(H), int(C)))


def _key_value(key: Tensor, value: Optional[Tensor], W: int):
    """``key`` and ``value`` with one shared row stride (copies made contiguous if they differ)."""
    key = _strided_rows(key, 'key', W)
    if value is None:
        return key, None, key.stride(0)
    value = _strided_rows(value, 'value', W)
    if value.size(0) != key.size(0):
        raise ValueError("'key' and 'value' need one row per source each")
    if key.stride(0) != value.stride(0):
        key, value = key.contiguous(), value.contiguous()
    return key, value, key.stride(0)


def transformer_forward(rowptr: Tensor, col: Tensor, query: Tensor, key: Tensor,
                        value: Optional[Tensor], H: int, C: int, scale: float, *, hub=None,
                        aggregate: bool = True):
    """``(alpha [nnz, H] in slot order, out [n_rows, H * C] | None)`` of one dot-product attention
    step on a by-destination handle; ``aggregate=False`` is the score mode (alpha only, ``value``
    not read)."""
    _require_device(rowptr, col, query, key, value)
    lib = _lib.load()
    W = H * C
    query = _dense_rows(query, 'query', W)
    key, value, ld = _key_value(key, value if aggregate else None, W)
    n_rows = rowptr.numel() - 1
    if query.size(0) < n_rows:
        raise ValueError(f"'query' needs at least {n_rows} rows")
    g = _csr(rowptr, col, n_rows, hub)
    alpha = torch.empty(col.numel(), H, dtype=torch.float32, device=query.device)
    out = torch.empty(n_rows, W, dtype=torch.float32, device=query.device) if aggregate else None
    if col.numel() == 0:  # no edges: every row is empty
        return alpha, (out.zero_() if aggregate else None)
    ws, ws_bytes = _workspace(lib.pygamd_transformer_workspace_bytes, (g.n_chunks, H, C),
                              query.device, g.n_chunks > 0)
    with _timed({'kind': 'transformer', 'op': 'forward' if aggregate else 'score',
                 'n_rows': n_rows, 'E': col.numel(), 'H': H, 'C': C, 'ld': ld, 'n_hub': g.n_hub,
                 'n_chunks': g.n_chunks}, query):
        check(lib.pygamd_transformer_forward(
            ctypes.byref(g), _p(query), _p(key), _p(value), ld, key.size(0), H, C, float(scale),
            _p(alpha), _p(out), _p(ws), ws_bytes, _stream(query)), 'transformer_forward')
    return alpha, out


def transformer_backward_dst(rowptr: Tensor, col: Tensor, query: Tensor, key: Tensor,
                             value: Optional[Tensor], alpha: Tensor, H: int, C: int,
                             scale: float, *, grad_out: Optional[Tensor] = None,
                             out: Optional[Tensor] = None, grad_alpha: Optional[Tensor] = None,
                             hub=None):
    """``(grad_s [nnz, H], grad_query [rows of query, H * C])``; ``grad_alpha`` given = score mode
    (``value`` not read), otherwise ``grad_out`` and ``out``."""
    _require_device(rowptr, col, query, key, value, alpha, grad_out, out, grad_alpha)
    lib = _lib.load()
    W = H * C
    score = grad_alpha is not None
    key, value, ld = _key_value(key, None if score else value, W)
    alpha = alpha.contiguous()
    n_rows = rowptr.numel() - 1
    if score:
        grad_alpha = grad_alpha.contiguous()
    else:
        grad_out, out = _dense_rows(grad_out, 'grad_out', W), _dense_rows(out, 'out', W)
    g = _csr(rowptr, col, n_rows, hub)
    grad_s = torch.empty_like(alpha)
    grad_query = _grad_rows(query.size(0), n_rows, W, key.device)
    if col.numel() == 0:
        return grad_s, grad_query.zero_()
    ws, ws_bytes = _workspace(lib.pygamd_transformer_workspace_bytes, (g.n_chunks, H, C),
                              key.device)
    with _timed({'kind': 'transformer', 'op': 'backward_dst', 'n_rows': n_rows, 'E': col.numel(),
                 'H': H, 'C': C, 'ld': ld, 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'score': score}, key):
        check(lib.pygamd_transformer_backward_dst(
            ctypes.byref(g), _p(key), _p(value), ld, _p(alpha), _p(grad_out), _p(out),
            _p(grad_alpha), key.size(0), H, C, float(scale), _p(grad_s), _p(grad_query), _p(ws),
            ws_bytes, _stream(key)), 'transformer_backward_dst')
    return grad_s, grad_query


def transformer_backward_src(rowptr_t: Tensor, col_t: Tensor, slot_map: Tensor, query: Tensor,
                             alpha: Tensor, grad_s: Tensor, H: int, C: int, scale: float, *,
                             grad_out: Optional[Tensor] = None, n_dst: int, hub=None,
                             packed: bool = False):
    """``(grad_key, grad_value | None)``, ``[n_src, H * C]`` each, on the by-source handle;
    ``grad_out=None`` = score mode (``grad_key`` only).  ``packed``: the two are the halves of ONE
    ``[n_src, 2 * H * C]`` buffer (row stride ``2 * H * C``), the gradient of a packed key | value
    projection, and that buffer is returned in place of the pair's first entry (the second is
    None)."""
    _require_device(rowptr_t, col_t, slot_map, query, alpha, grad_s, grad_out)
    lib = _lib.load()
    W = H * C
    query = _dense_rows(query, 'query', W)
    alpha, grad_s = alpha.contiguous(), grad_s.contiguous()
    score = grad_out is None
    if not score:
        grad_out = _dense_rows(grad_out, 'grad_out', W)
    n_src = rowptr_t.numel() - 1
    if slot_map.dtype != rowptr_t.dtype:
        raise ValueError("'slot_map' must have the index dtype")
    slot_map = slot_map.contiguous()
    g = _csr(rowptr_t, col_t, n_src, hub)
    if packed and score:
        raise ValueError('the score mode has no value gradient to pack')
    if packed:
        both = torch.empty(n_src, 2 * W, dtype=torch.float32, device=query.device)
        grad_key, grad_value, ld = both[:, :W], both[:, W:], 2 * W
        result = (both, None)
    else:
        grad_key = torch.empty(n_src, W, dtype=torch.float32, device=query.device)
        grad_value = None if score else torch.empty_like(grad_key)
        ld = W
        result = (grad_key, grad_value)
    if col_t.numel() == 0:
        for t in result:
            if t is not None:
                t.zero_()
        return result
    ws, ws_bytes = _workspace(lib.pygamd_transformer_workspace_bytes, (g.n_chunks, H, C),
                              query.device, g.n_chunks > 0)
    with _timed({'kind': 'transformer', 'op': 'backward_src', 'n_rows': n_src,
                 'E': col_t.numel(), 'H': H, 'C': C, 'ld': ld, 'n_hub': g.n_hub,
                 'n_chunks': g.n_chunks, 'score': score}, query):
        check(lib.pygamd_transformer_backward_src(
            ctypes.byref(g), _p(slot_map), _p(query), _p(alpha), _p(grad_s), _p(grad_out), n_dst,
            H, C, float(scale), _p(grad_key), _p(grad_value), ld, _p(ws), ws_bytes,
            _stream(query)), 'transformer_backward_src')
    return result


# ---- ... with edge features inside the kernels (the edge variant of csrc/transformer.hip) --------
def transformer_edge_supported(H: int, C: int, De: int) -> bool:
    """The edge variant serves this layout: that of :func:`transformer_supported` and ``De <= 4 *
    lph``, ``lph`` the largest power of two with ``H * lph <= 64``."""
    return bool(_lib.load().pygamd_transformer_edge_supported(int(H), int(C), int(De)))


def transformer_edge_forward(rowptr: Tensor, col: Tensor, query: Tensor, key: Tensor,
                             value: Optional[Tensor], edge_attr: Tensor, bias: Tensor, H: int,
                             C: int, scale: float, *, hub=None, aggregate: bool = True):
    """``(alpha [nnz, H] in slot order, out [n_rows, H * C] | None, z [n_rows, H * De] | None)``
    of one attention step whose score carries ``<bias[i, h], edge_attr[k]>``; ``edge_attr [nnz,
    De]`` in SLOT order, ``bias [>= n_rows, H * De]``.  ``out`` is the weighted sum of ``value``
    alone, ``z`` that of the raw edge features; ``aggregate=False`` is the score mode (alpha
    only)."""
    _require_device(rowptr, col, query, key, value, edge_attr, bias)
    lib = _lib.load()
    W = H * C
    query = _dense_rows(query, 'query', W)
    key, value, ld = _key_value(key, value if aggregate else None, W)
    n_rows = rowptr.numel() - 1
    edge_attr = _edge_rows(edge_attr, col.numel())
    De = edge_attr.size(1)
    bias = _dense_rows(bias, 'bias', H * De)
    if query.size(0) < n_rows or bias.size(0) < n_rows:
        raise ValueError(f"'query' and 'bias' need at least {n_rows} rows")
    g = _csr(rowptr, col, n_rows, hub)
    alpha = torch.empty(col.numel(), H, dtype=torch.float32, device=query.device)
    out = torch.empty(n_rows, W, dtype=torch.float32, device=query.device) if aggregate else None
    z = torch.empty(n_rows, H * De, dtype=torch.float32, device=query.device) \
        if aggregate else None
    if col.numel() == 0:  # no edges: every row is empty
        return alpha, (out.zero_() if aggregate else None), (z.zero_() if aggregate else None)
    ws, ws_bytes = _workspace(lib.pygamd_transformer_edge_workspace_bytes,
                              (g.n_chunks, H, C, De), query.device, g.n_chunks > 0)
    with _timed({'kind': 'transformer', 'op': 'edge_forward' if aggregate else 'edge_score',
                 'n_rows': n_rows, 'E': col.numel(), 'H': H, 'C': C, 'De': De, 'ld': ld,
                 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, query):
        check(lib.pygamd_transformer_edge_forward(
            ctypes.byref(g), _p(query), _p(key), _p(value), ld, _p(edge_attr), _p(bias),
            key.size(0), H, C, De, float(scale), _p(alpha), _p(out), _p(z), _p(ws), ws_bytes,
            _stream(query)), 'transformer_edge_forward')
    return alpha, out, z


def transformer_edge_backward_dst(rowptr: Tensor, col: Tensor, query: Tensor, key: Tensor,
                                  value: Optional[Tensor], edge_attr: Tensor, bias: Tensor,
                                  alpha: Tensor, H: int, C: int, scale: float, *,
                                  grad_out: Optional[Tensor] = None, out: Optional[Tensor] = None,
                                  grad_z: Optional[Tensor] = None, z: Optional[Tensor] = None,
                                  grad_alpha: Optional[Tensor] = None,
                                  want_grad_edge_attr: bool = True, hub=None):
    """``(grad_s [nnz, H], grad_query [rows of query, H * C], grad_bias [rows of bias, H * De],
    grad_edge_attr [nnz, De] in slot order | None)``; ``grad_alpha`` given = score mode
    (``value`` not read, ``grad_edge_attr`` holds its ``grad_s * bias`` part), otherwise
    ``grad_out``, ``out``, ``grad_z`` and ``z``."""
    _require_device(rowptr, col, query, key, value, edge_attr, bias, alpha, grad_out, out, grad_z,
                    z, grad_alpha)
    lib = _lib.load()
    W = H * C
    De = edge_attr.size(1)
    Z = H * De
    score = grad_alpha is not None
    key, value, ld = _key_value(key, None if score else value, W)
    alpha, edge_attr = alpha.contiguous(), edge_attr.contiguous()
    bias = _dense_rows(bias, 'bias', Z)
    n_rows = rowptr.numel() - 1
    if score:
        grad_alpha = grad_alpha.contiguous()
    else:
        grad_out, out = _dense_rows(grad_out, 'grad_out', W), _dense_rows(out, 'out', W)
        grad_z, z = _dense_rows(grad_z, 'grad_z', Z), _dense_rows(z, 'z', Z)
    g = _csr(rowptr, col, n_rows, hub)
    grad_s = torch.empty_like(alpha)
    dev = key.device
    grad_query = _grad_rows(query.size(0), n_rows, W, dev)
    grad_bias = _grad_rows(bias.size(0), n_rows, Z, dev)
    grad_edge = torch.empty_like(edge_attr) if want_grad_edge_attr else None
    if col.numel() == 0:
        return grad_s, grad_query.zero_(), grad_bias.zero_(), grad_edge
    ws, ws_bytes = _workspace(lib.pygamd_transformer_edge_workspace_bytes,
                              (g.n_chunks, H, C, De), dev)
    with _timed({'kind': 'transformer', 'op': 'edge_backward_dst', 'n_rows': n_rows,
                 'E': col.numel(), 'H': H, 'C': C, 'De': De, 'ld': ld, 'n_hub': g.n_hub,
                 'n_chunks': g.n_chunks, 'score': score,
                 'grad_edge_attr': want_grad_edge_attr}, key):
        check(lib.pygamd_transformer_edge_backward_dst(
            ctypes.byref(g), _p(key), _p(value), ld, _p(edge_attr), _p(bias), _p(alpha),
            _p(grad_out), _p(out), _p(grad_z), _p(z), _p(grad_alpha), key.size(0), H, C, De,
            float(scale), _p(grad_s), _p(grad_query), _p(grad_bias), _p(grad_edge), _p(ws),
            ws_bytes, _stream(key)), 'transformer_edge_backward_dst')
    return grad_s, grad_query, grad_bias, grad_edge


# ---- GINEConv's edge message (csrc/gine.hip) -------------------------------------------------------
def gine_supported(F: int, De: int = 0) -> bool:
    """The kernel pair serves ``F <= 512`` and, in linear mode (``De >= 1``), ``De <= 32`` and
    ``F * De <= 4096``; ``De = 0`` is the wide mode."""
    return bool(_lib.load().pygamd_gine_supported(int(F), int(De)))


def _gine_edge(edge_attr: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], F: int,
               E: int):
    """(edge_attr, weight, bias, De) checked: wide mode without ``weight`` (``De = 0``)."""
    edge_attr = _edge_rows(edge_attr, E, 'width')
    if weight is None:
        if bias is not None:
            raise ValueError("'bias' needs 'weight'")
        if edge_attr.size(1) != F:
            raise ValueError(f"without 'weight' the edge features need width {F} (got "
                             f"{edge_attr.size(1)})")
        return edge_attr, None, None, 0
    De = edge_attr.size(1)
    if weight.dtype != torch.float32 or tuple(weight.shape) != (F, De) or De < 1:
        raise ValueError(f"'weight' must be float32 [{F}, {De}] (got {weight.dtype} "
                         f"{tuple(weight.shape)})")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (F,)):
        raise ValueError(f"'bias' must be float32 [{F}]")
    return edge_attr, weight.contiguous(), None if bias is None else bias.contiguous(), De


def _gine_no_edges(rowptr: Tensor, x: Tensor):
    """(col, edge_id, edge_attr) of a graph without edges: valid one-element buffers, never read"""
    return rowptr.new_zeros(1), None, x.new_zeros(1, 1)


def gine_forward(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], x_src: Tensor,
                 x_root: Optional[Tensor], eps: Optional[Tensor], edge_attr: Tensor,
                 weight: Optional[Tensor] = None, bias: Optional[Tensor] = None, *, hub=None):
    """``out [n_rows, F] = (1 + eps) * x_root[:n_rows] + sum_k relu(x_src[col[k]] + e_k)`` on a
    by-destination handle; ``e_k = edge_attr[edge_id[k]]`` (wide) or ``weight @ edge_attr[edge_id[k]]
    + bias`` (linear).  ``edge_attr`` stays in the caller's edge order (``edge_id=None``: it is in
    slot order); ``eps`` is a one-element device tensor; ``x_root`` and ``eps`` may be None.
    ``x_src`` and ``x_root`` may be column blocks of wider tensors (their row stride is passed)."""
    _require_device(rowptr, col, edge_id, x_src, x_root, eps, edge_attr, weight, bias)
    lib = _lib.load()
    if x_src.dim() != 2:
        raise ValueError("'x_src' must be two-dimensional")
    F = x_src.size(1)
    x_src = _strided_rows(x_src, 'x_src', F)
    n_rows = rowptr.numel() - 1
    if x_root is not None:
        x_root = _strided_rows(x_root, 'x_root', F)
        if x_root.size(0) < n_rows:
            raise ValueError(f"'x_root' needs at least {n_rows} rows")
        if eps is not None and (eps.dtype != torch.float32 or eps.numel() != 1):
            raise ValueError("'eps' must be one float32")
    else:
        eps = None
    edge_attr, weight, bias, De = _gine_edge(edge_attr, weight, bias, F, col.numel())
    edge_id = _edge_id(edge_id, rowptr, col)
    out = torch.empty(n_rows, F, dtype=torch.float32, device=x_src.device)
    if n_rows == 0:
        return out
    if col.numel() == 0:  # no edges: every row is its self term; the launch reads no slot
        col, edge_id, edge_attr = _gine_no_edges(rowptr, x_src)
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_gine_workspace_bytes, (g.n_chunks, F, De), x_src.device,
                              g.n_chunks > 0)
    with _timed({'kind': 'gine', 'op': 'forward', 'n_rows': n_rows, 'E': col.numel(), 'F': F,
                 'De': De, 'ld': _ld(x_src), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': False}, x_src):
        check(lib.pygamd_gine_forward(
            ctypes.byref(g), _p(edge_id), _p(x_src), _ld(x_src), _p(x_root),
            0 if x_root is None else _ld(x_root), _p(eps), _p(edge_attr), _p(weight), _p(bias),
            x_src.size(0), F, De, _p(out), _p(ws), ws_bytes, _stream(x_src)), 'gine_forward')
    return out


def gine_backward(rowptr_t: Tensor, col_t: Tensor, edge_id_t: Optional[Tensor], x_src: Tensor,
                  edge_attr: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                  grad_out: Tensor, *, want_grad_edge_attr: bool = True, hub=None):
    """``(grad_x_src [n_src, F], grad_edge_attr | None, grad_weight | None, grad_bias | None)`` on
    the by-SOURCE handle (``col_t`` = the destination of every out-slot, ``edge_id_t`` = that
    form's slot -> edge map); ``grad_edge_attr`` comes in the caller's edge order."""
    _require_device(rowptr_t, col_t, edge_id_t, x_src, edge_attr, weight, bias, grad_out)
    lib = _lib.load()
    F = x_src.size(1)
    x_src = _strided_rows(x_src, 'x_src', F)
    grad_out = _dense_rows(grad_out, 'grad_out', F)
    n_src = rowptr_t.numel() - 1
    if x_src.size(0) != n_src:
        raise ValueError(f"'x_src' needs {n_src} rows")
    edge_attr, weight, bias, De = _gine_edge(edge_attr, weight, bias, F, col_t.numel())
    edge_id_t = _edge_id(edge_id_t, rowptr_t, col_t, 'edge_id_t')
    dev = x_src.device
    grad_x = torch.empty(n_src, F, dtype=torch.float32, device=dev)
    grad_edge = torch.empty_like(edge_attr) if want_grad_edge_attr else None
    grad_w = torch.empty_like(weight) if weight is not None else None
    grad_b = torch.empty_like(bias) if bias is not None else None
    if n_src == 0:
        for t in (grad_w, grad_b):
            if t is not None:
                t.zero_()
        return grad_x, grad_edge, grad_w, grad_b
    if col_t.numel() == 0:
        col_t, edge_id_t, edge_attr = _gine_no_edges(rowptr_t, x_src)
    g = _csr(rowptr_t, col_t, n_src, hub)
    ws, ws_bytes = _workspace(lib.pygamd_gine_workspace_bytes, (g.n_chunks, F, De), dev,
                              g.n_chunks > 0 or De > 0)
    with _timed({'kind': 'gine', 'op': 'backward', 'n_rows': n_src, 'E': col_t.numel(), 'F': F,
                 'De': De, 'ld': _ld(x_src), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': bool(want_grad_edge_attr)}, x_src):
        check(lib.pygamd_gine_backward(
            ctypes.byref(g), _p(edge_id_t), _p(x_src), _ld(x_src), _p(edge_attr), _p(weight),
            _p(bias), _p(grad_out), grad_out.size(0), F, De, _p(grad_x), _p(grad_edge), _p(grad_w),
            _p(grad_b), _p(ws), ws_bytes, _stream(x_src)), 'gine_backward')
    return grad_x, grad_edge, grad_w, grad_b


# ---- PNAConv's multi-statistic aggregation (csrc/pna.hip) ------------------------------------------
PNA_STATS = ('mean', 'min', 'max', 'std')      # the kernel's order: bit q selects PNA_STATS[q]


def pna_supported(W: int, De: int = 0) -> bool:
    """The kernel pair serves message widths ``W <= 512`` and, with edge features (``De >= 1``),
    ``De <= 32`` and ``W * De <= 4096``."""
    return bool(_lib.load().pygamd_pna_supported(int(W), int(De)))


def _pna_mask(stats) -> int:
    stats = tuple(stats)
    if not stats or len(set(stats)) != len(stats) or any(s not in PNA_STATS for s in stats):
        raise ValueError(f"'stats' must be a non-empty subset of {PNA_STATS} (got {stats})")
    return sum(1 << PNA_STATS.index(s) for s in stats)


def _pna_edge(edge_attr: Optional[Tensor], wc: Optional[Tensor], W: int, E: int):
    """(edge_attr, wc, De) checked; both None without edge features (``De = 0``)."""
    if (edge_attr is None) != (wc is None):
        raise ValueError("'edge_attr' and 'wc' come together")
    if wc is None:
        return None, None, 0
    edge_attr = _edge_rows(edge_attr, E)
    De = edge_attr.size(1)
    if wc.dtype != torch.float32 or tuple(wc.shape) != (W, De) or De < 1:
        raise ValueError(f"'wc' must be float32 [{W}, {De}] (got {wc.dtype} {tuple(wc.shape)})")
    return edge_attr, wc.contiguous(), De


def pna_forward(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], p_src: Tensor,
                p_dst: Tensor, edge_attr: Optional[Tensor], wc: Optional[Tensor], stats, *,
                hub=None):
    """The statistics ``stats`` (a subset of :data:`PNA_STATS`) of the messages ``p_dst[i] + u_k``,
    ``u_k = p_src[col[k]] + wc @ edge_attr[edge_id[k]]``, over every row of a by-destination
    handle: ``(out [n_stats, n_rows, W], saved [6, n_rows, W])`` with the planes of ``out`` in the
    order of :data:`PNA_STATS` and ``saved`` = mean u, min u, max u, std, the numbers of slots
    attaining the minimum / the maximum.  Rows without slots are exactly 0.  ``p_src`` and
    ``p_dst`` may be column blocks of wider tensors (their row stride is passed)."""
    _require_device(rowptr, col, edge_id, p_src, p_dst, edge_attr, wc)
    lib = _lib.load()
    if p_src.dim() != 2:
        raise ValueError("'p_src' must be two-dimensional")
    W = p_src.size(1)
    mask = _pna_mask(stats)
    p_src, p_dst = _strided_rows(p_src, 'p_src', W), _strided_rows(p_dst, 'p_dst', W)
    n_rows = rowptr.numel() - 1
    if p_dst.size(0) < n_rows:
        raise ValueError(f"'p_dst' needs at least {n_rows} rows")
    edge_attr, wc, De = _pna_edge(edge_attr, wc, W, col.numel())
    edge_id = _edge_id(edge_id, rowptr, col)
    dev = p_src.device
    n_sel = bin(mask).count('1')
    if n_rows == 0 or col.numel() == 0:  # no slot anywhere: every statistic is 0, nothing to launch
        saved = torch.zeros(6, n_rows, W, dtype=torch.float32, device=dev)
        saved[4:] = 1.0
        return torch.zeros(n_sel, n_rows, W, dtype=torch.float32, device=dev), saved
    out = torch.empty(n_sel, n_rows, W, dtype=torch.float32, device=dev)
    saved = torch.empty(6, n_rows, W, dtype=torch.float32, device=dev)
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_pna_workspace_bytes, (g.n_chunks, W, 0), dev,
                              g.n_chunks > 0)
    with _timed({'kind': 'pna', 'op': 'forward', 'n_rows': n_rows, 'E': col.numel(), 'W': W,
                 'De': De, 'stats': mask, 'ld': _ld(p_src), 'n_hub': g.n_hub,
                 'n_chunks': g.n_chunks, 'grad_edge_attr': False}, p_src):
        check(lib.pygamd_pna_forward(
            ctypes.byref(g), _p(edge_id), _p(p_src), _ld(p_src), _p(p_dst), _ld(p_dst),
            _p(edge_attr), _p(wc), p_src.size(0), W, De, mask, _p(out), _p(saved), _p(ws),
            ws_bytes, _stream(p_src)), 'pna_forward')
    return out, saved


def pna_backward(rowptr_t: Tensor, col_t: Tensor, edge_id_t: Optional[Tensor], p_src: Tensor,
                 edge_attr: Optional[Tensor], wc: Optional[Tensor], coef: Tensor, stats, *,
                 want_grad_edge_attr: bool = True, hub=None):
    """``(grad_p_src [n_src, W], grad_edge_attr | None, grad_wc | None)`` on the by-SOURCE handle
    (``col_t`` = the destination of every out-slot, ``edge_id_t`` = that form's slot -> edge map)
    from the packed coefficient rows ``coef [n_dst, 6, W]`` = A, B, Gmin, Gmax, min u, max u:
    ``grad_u = A + B u + Gmin [u == min u] + Gmax [u == max u]`` per slot."""
    _require_device(rowptr_t, col_t, edge_id_t, p_src, edge_attr, wc, coef)
    lib = _lib.load()
    W = p_src.size(1)
    mask = _pna_mask(stats)
    p_src = _strided_rows(p_src, 'p_src', W)
    n_src = rowptr_t.numel() - 1
    if p_src.size(0) != n_src:
        raise ValueError(f"'p_src' needs {n_src} rows")
    if coef.dtype != torch.float32 or coef.dim() != 3 or tuple(coef.shape[1:]) != (6, W):
        raise ValueError(f"'coef' must be a float32 [n_dst, 6, {W}] tensor (got {coef.dtype} "
                         f"{tuple(coef.shape)})")
    coef = coef.contiguous()
    edge_attr, wc, De = _pna_edge(edge_attr, wc, W, col_t.numel())
    edge_id_t = _edge_id(edge_id_t, rowptr_t, col_t)
    want_grad_edge_attr = bool(want_grad_edge_attr) and De > 0
    dev = p_src.device
    if n_src == 0 or col_t.numel() == 0:
        return (torch.zeros(n_src, W, dtype=torch.float32, device=dev),
                torch.zeros_like(edge_attr) if want_grad_edge_attr else None,
                None if wc is None else torch.zeros_like(wc))
    grad_p = torch.empty(n_src, W, dtype=torch.float32, device=dev)
    grad_edge = torch.empty_like(edge_attr) if want_grad_edge_attr else None
    grad_wc = torch.empty_like(wc) if wc is not None else None
    g = _csr(rowptr_t, col_t, n_src, hub)
    ws, ws_bytes = _workspace(lib.pygamd_pna_workspace_bytes, (g.n_chunks, W, De), dev,
                              g.n_chunks > 0 or De > 0)
    with _timed({'kind': 'pna', 'op': 'backward', 'n_rows': n_src, 'E': col_t.numel(), 'W': W,
                 'De': De, 'stats': mask, 'ld': _ld(p_src), 'n_hub': g.n_hub,
                 'n_chunks': g.n_chunks, 'grad_edge_attr': want_grad_edge_attr}, p_src):
        check(lib.pygamd_pna_backward(
            ctypes.byref(g), _p(edge_id_t), _p(p_src), _ld(p_src), _p(edge_attr), _p(wc),
            _p(coef), coef.size(0), W, De, mask, _p(grad_p), _p(grad_edge), _p(grad_wc), _p(ws),
            ws_bytes, _stream(p_src)), 'pna_backward')
    return grad_p, grad_edge, grad_wc


# ---- GENConv's softmax aggregation (csrc/gen.hip) --------------------------------------------------
GEN_EDGE_NONE, GEN_EDGE_WIDE, GEN_EDGE_LINEAR = (_lib.CONSTANTS['PYGAMD_GEN_EDGE_' + m]
                                                 for m in ('NONE', 'WIDE', 'LINEAR'))


def gen_supported(F: int, De: int = 0) -> bool:
    """The kernel pair serves ``F <= 512`` and, with ``lin_edge`` (``De >= 1``), ``De <= 32`` and
    ``F * De <= 4096``; ``De = 0`` for edge features of width ``F`` or none."""
    return bool(_lib.load().pygamd_gen_supported(int(F), int(De)))


def _gen_edge(edge_attr: Optional[Tensor], weight: Optional[Tensor], bias: Optional[Tensor],
              F: int, E: int):
    """(mode, edge_attr, weight, bias, De) checked; everything None without an edge term."""
    if edge_attr is None:
        if weight is not None or bias is not None:
            raise ValueError("'weight' and 'bias' need 'edge_attr'")
        return GEN_EDGE_NONE, None, None, None, 0
    edge_attr, weight, bias, De = _gine_edge(edge_attr, weight, bias, F, E)
    return (GEN_EDGE_LINEAR if De else GEN_EDGE_WIDE), edge_attr, weight, bias, De


def _gen_t(t: Tensor, F: int) -> Tensor:
    if t.dtype != torch.float32 or t.numel() not in (1, F):
        raise ValueError(f"'t' must hold 1 or {F} float32 values (got {t.dtype} "
                         f"{tuple(t.shape)})")
    return t.reshape(-1).contiguous()


def gen_forward(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], x_src: Tensor,
                edge_attr: Optional[Tensor], weight: Optional[Tensor], bias: Optional[Tensor],
                t: Tensor, *, eps_msg: float = 1e-7, want_s2: bool = False, hub=None):
    """``(out [n_rows, F], saved [2 | 3, n_rows, F])`` on a by-destination handle: ``out[i] =
    sum_k alpha_k m_k`` with ``m_k = relu(x_src[col[k]] + e_k) + eps_msg`` and ``alpha`` the softmax
    of ``t * m`` over the slots of ``i`` PER COLUMN; ``e_k`` is 0 (``edge_attr=None``),
    ``edge_attr[edge_id[k]]`` (width ``F``) or ``weight @ edge_attr[edge_id[k]] + bias``.  ``t`` is
    a device tensor of 1 or ``F`` values.  ``saved`` holds the running maximum ``M``, ``1 / (L +
    1e-16)`` and, with ``want_s2``, ``sum_k alpha m^2``.  Rows without slots are exactly 0.
    ``x_src`` may be a column block of a wider tensor (its row stride is passed)."""
    _require_device(rowptr, col, edge_id, x_src, edge_attr, weight, bias, t)
    lib = _lib.load()
    if x_src.dim() != 2:
        raise ValueError("'x_src' must be two-dimensional")
    F = x_src.size(1)
    x_src = _strided_rows(x_src, 'x_src', F)
    n_rows = rowptr.numel() - 1
    mode, edge_attr, weight, bias, De = _gen_edge(edge_attr, weight, bias, F, col.numel())
    t = _gen_t(t, F)
    edge_id = _edge_id(edge_id, rowptr, col)
    dev = x_src.device
    planes = 3 if want_s2 else 2
    if n_rows == 0 or col.numel() == 0:  # no slot anywhere: zeros, nothing to launch
        return (torch.zeros(n_rows, F, dtype=torch.float32, device=dev),
                torch.zeros(planes, n_rows, F, dtype=torch.float32, device=dev))
    out = torch.empty(n_rows, F, dtype=torch.float32, device=dev)
    saved = torch.empty(planes, n_rows, F, dtype=torch.float32, device=dev)
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_gen_workspace_bytes, (g.n_chunks, F, 0), dev,
                              g.n_chunks > 0)
    with _timed({'kind': 'gen', 'op': 'forward', 'n_rows': n_rows, 'E': col.numel(), 'F': F,
                 'De': De, 'ld': _ld(x_src), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': False, 'grad_t': bool(want_s2)}, x_src):
        check(lib.pygamd_gen_forward(
            ctypes.byref(g), _p(edge_id), _p(x_src), _ld(x_src), mode, _p(edge_attr), _p(weight),
            _p(bias), _p(t), t.numel(), float(eps_msg), x_src.size(0), F, De, int(want_s2),
            _p(out), _p(saved), _p(ws), ws_bytes, _stream(x_src)), 'gen_forward')
    return out, saved


def gen_backward(rowptr_t: Tensor, col_t: Tensor, edge_id_t: Optional[Tensor], x_src: Tensor,
                 edge_attr: Optional[Tensor], weight: Optional[Tensor], bias: Optional[Tensor],
                 t: Tensor, coef: Tensor, *, eps_msg: float = 1e-7, semi_grad: bool = False,
                 want_grad_edge_attr: bool = True, grad_t: bool = False, hub=None):
    """``(grad_x_src [n_src, F], grad_edge_attr | None, grad_weight | None, grad_bias | None)`` on
    the by-SOURCE handle (``col_t`` = the destination of every out-slot, ``edge_id_t`` = that
    form's slot -> edge map) from the packed rows ``coef [n_dst, 3, F]`` = ``M``, ``grad_out / (L +
    1e-16)``, ``out`` (``semi_grad``: ``[n_dst, 2, F]`` without ``out``).  ``grad_edge_attr`` comes
    in the caller's edge order.  ``grad_t`` only marks the timing record: the gradient of ``t`` is
    the caller's reduction."""
    _require_device(rowptr_t, col_t, edge_id_t, x_src, edge_attr, weight, bias, t, coef)
    lib = _lib.load()
    F = x_src.size(1)
    x_src = _strided_rows(x_src, 'x_src', F)
    n_src = rowptr_t.numel() - 1
    if x_src.size(0) != n_src:
        raise ValueError(f"'x_src' needs {n_src} rows")
    planes = 2 if semi_grad else 3
    if coef.dtype != torch.float32 or coef.dim() != 3 or tuple(coef.shape[1:]) != (planes, F):
        raise ValueError(f"'coef' must be a float32 [n_dst, {planes}, {F}] tensor (got "
                         f"{coef.dtype} {tuple(coef.shape)})")
    coef = coef.contiguous()
    mode, edge_attr, weight, bias, De = _gen_edge(edge_attr, weight, bias, F, col_t.numel())
    t = _gen_t(t, F)
    edge_id_t = _edge_id(edge_id_t, rowptr_t, col_t, 'edge_id_t')
    want_grad_edge_attr = bool(want_grad_edge_attr) and mode != GEN_EDGE_NONE
    dev = x_src.device
    if n_src == 0 or col_t.numel() == 0:
        return (torch.zeros(n_src, F, dtype=torch.float32, device=dev),
                torch.zeros_like(edge_attr) if want_grad_edge_attr else None,
                None if weight is None else torch.zeros_like(weight),
                None if bias is None else torch.zeros_like(bias))
    grad_x = torch.empty(n_src, F, dtype=torch.float32, device=dev)
    grad_edge = torch.empty_like(edge_attr) if want_grad_edge_attr else None
    grad_w = torch.empty_like(weight) if weight is not None else None
    grad_b = torch.empty_like(bias) if bias is not None else None
    g = _csr(rowptr_t, col_t, n_src, hub)
    ws, ws_bytes = _workspace(lib.pygamd_gen_workspace_bytes, (g.n_chunks, F, De), dev,
                              g.n_chunks > 0 or De > 0)
    with _timed({'kind': 'gen', 'op': 'backward', 'n_rows': n_src, 'E': col_t.numel(), 'F': F,
                 'De': De, 'ld': _ld(x_src), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': want_grad_edge_attr, 'grad_t': bool(grad_t)}, x_src):
        check(lib.pygamd_gen_backward(
            ctypes.byref(g), _p(edge_id_t), _p(x_src), _ld(x_src), mode, _p(edge_attr),
            _p(weight), _p(bias), _p(t), t.numel(), float(eps_msg), int(bool(semi_grad)),
            _p(coef), coef.size(0), F, De, int(want_grad_edge_attr), _p(grad_x), _p(grad_edge),
            _p(grad_w), _p(grad_b), _p(ws), ws_bytes, _stream(x_src)), 'gen_backward')
    return grad_x, grad_edge, grad_w, grad_b


# ---- ResGatedGraphConv's gated sum (csrc/resgated.hip) ----------------------------------------------
def resgated_supported(F: int, De: int = 0) -> bool:
    """The kernels serve ``F <= 512`` and, with ``edge_dim`` (``De >= 1``), ``De <= 32`` and
    ``F * De <= 2048`` (two edge matrices share the registers gine.hip gives one)."""
    return bool(_lib.load().pygamd_resgated_supported(int(F), int(De)))


def _resgated_args(k: Tensor, qv: Tensor, edge_attr: Optional[Tensor], weight: Optional[Tensor],
                   n_dst: int, E: int):
    """(k, qv, edge_attr, weight, F, De) checked: ``k [>= n_dst, F]`` and the packed ``qv [n_src,
    2F]`` with their row strides, ``weight [2, F, De]`` = ``Wg``, then ``Wv``; both edge arguments
    None without an edge term (``De = 0``)."""
    if k.dim() != 2:
        raise ValueError("'k' must be two-dimensional")
    F = k.size(1)
    k, qv = _strided_rows(k, 'k', F), _strided_rows(qv, 'qv', 2 * F)
    if k.size(0) < n_dst:
        raise ValueError(f"'k' needs at least {n_dst} rows")
    if (edge_attr is None) != (weight is None):
        raise ValueError("'edge_attr' and 'weight' come together")
    if weight is None:
        return k, qv, None, None, F, 0
    edge_attr = _edge_rows(edge_attr, E)
    De = edge_attr.size(1)
    if weight.dtype != torch.float32 or tuple(weight.shape) != (2, F, De) or De < 1:
        raise ValueError(f"'weight' must be float32 [2, {F}, {De}] (got {weight.dtype} "
                         f"{tuple(weight.shape)})")
    return k, qv, edge_attr, weight.contiguous(), F, De


def resgated_forward(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], k: Tensor,
                     qv: Tensor, edge_attr: Optional[Tensor] = None,
                     weight: Optional[Tensor] = None, *, hub=None) -> Tensor:
    """``out [n_rows, F] = sum_k sigmoid(z_k) * u_k`` on a by-destination handle with ``z_k =
    k[i] + qv[col[k], :F] + weight[0] @ a_k`` and ``u_k = qv[col[k], F:] + weight[1] @ a_k``, ``a_k =
    edge_attr[edge_id[k]]`` (``edge_attr=None``: no edge terms).  Rows without slots are exactly
    0.  ``k`` and ``qv`` may be column blocks of wider tensors (their row strides are passed);
    ``edge_attr`` stays in the caller's edge order."""
    _require_device(rowptr, col, edge_id, k, qv, edge_attr, weight)
    lib = _lib.load()
    n_rows = rowptr.numel() - 1
    k, qv, edge_attr, weight, F, De = _resgated_args(k, qv, edge_attr, weight, n_rows,
                                                     col.numel())
    edge_id = _edge_id(edge_id, rowptr, col)
    dev = k.device
    if n_rows == 0 or col.numel() == 0:  # no slot anywhere: zeros, nothing to launch
        return torch.zeros(n_rows, F, dtype=torch.float32, device=dev)
    out = torch.empty(n_rows, F, dtype=torch.float32, device=dev)
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_resgated_workspace_bytes, (g.n_chunks, F, 0), dev,
                              g.n_chunks > 0)
    with _timed({'kind': 'resgated', 'op': 'forward', 'n_rows': n_rows, 'E': col.numel(), 'F': F,
                 'De': De, 'ld': _ld(qv), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': False}, k):
        check(lib.pygamd_resgated_forward(
            ctypes.byref(g), _p(edge_id), _p(k), _ld(k), _p(qv), _ld(qv), _p(edge_attr),
            _p(weight), qv.size(0), F, De, _p(out), _p(ws), ws_bytes, _stream(k)),
            'resgated_forward')
    return out


def resgated_backward_dst(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], k: Tensor,
                          qv: Tensor, edge_attr: Optional[Tensor], weight: Optional[Tensor],
                          grad_out: Tensor, *, want_grad_edge_attr: bool = True, hub=None):
    """``(grad_k [rows of k, F], grad_edge_attr | None, grad_weight [2, F, De] | None)`` on the
    forward's by-destination handle: ``grad_k[i] = sum_k g u s (1 - s)`` with ``s = sigmoid(z)``
    recomputed, and with an edge term ``grad_edge_attr[k] = weight[0]^T (g u s (1 - s)) +
    weight[1]^T (g s)`` in the caller's edge order and the gradients of both matrices from
    per-workgroup partials reduced in workgroup order."""
    _require_device(rowptr, col, edge_id, k, qv, edge_attr, weight, grad_out)
    lib = _lib.load()
    n_rows = rowptr.numel() - 1
    k, qv, edge_attr, weight, F, De = _resgated_args(k, qv, edge_attr, weight, n_rows,
                                                     col.numel())
    grad_out = _strided_rows(grad_out, 'grad_out', F)
    if grad_out.size(0) != n_rows:
        raise ValueError(f"'grad_out' needs {n_rows} rows")
    edge_id = _edge_id(edge_id, rowptr, col)
    want_grad_edge_attr = bool(want_grad_edge_attr) and De > 0
    dev = k.device
    if n_rows == 0 or col.numel() == 0:
        return (torch.zeros(k.size(0), F, dtype=torch.float32, device=dev),
                torch.zeros_like(edge_attr) if want_grad_edge_attr else None,
                None if weight is None else torch.zeros_like(weight))
    grad_k = _grad_rows(k.size(0), n_rows, F, dev)
    grad_edge = torch.empty_like(edge_attr) if want_grad_edge_attr else None
    grad_w = torch.empty_like(weight) if weight is not None else None
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_resgated_workspace_bytes, (g.n_chunks, F, De), dev,
                              g.n_chunks > 0 or De > 0)
    with _timed({'kind': 'resgated', 'op': 'backward_dst', 'n_rows': n_rows, 'E': col.numel(),
                 'F': F, 'De': De, 'ld': _ld(qv), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': want_grad_edge_attr}, k):
        check(lib.pygamd_resgated_backward_dst(
            ctypes.byref(g), _p(edge_id), _p(k), _ld(k), _p(qv), _ld(qv), _p(edge_attr),
            _p(weight), _p(grad_out), _ld(grad_out), qv.size(0), F, De, _p(grad_k),
            _p(grad_edge), _p(grad_w), _p(ws), ws_bytes, _stream(k)), 'resgated_backward_dst')
    return grad_k, grad_edge, grad_w


def resgated_backward_src(rowptr_t: Tensor, col_t: Tensor, edge_id_t: Optional[Tensor], k: Tensor,
                          qv: Tensor, edge_attr: Optional[Tensor], weight: Optional[Tensor],
                          grad_out: Tensor, *, hub=None) -> Tensor:
    """The packed ``grad_qv [n_src, 2F] = [sum g u s (1 - s) | sum g s]`` on the by-SOURCE handle
    (``col_t`` = the destination of every out-slot, ``edge_id_t`` = that form's slot -> edge
    map).  ``k`` and ``grad_out`` are gathered per slot, each at its own row stride: two tensors
    in place, or the two halves of one packed ``[n_dst, 2F]`` plane."""
    _require_device(rowptr_t, col_t, edge_id_t, k, qv, edge_attr, weight, grad_out)
    lib = _lib.load()
    n_src = rowptr_t.numel() - 1
    k, qv, edge_attr, weight, F, De = _resgated_args(k, qv, edge_attr, weight, 0, col_t.numel())
    if qv.size(0) != n_src:
        raise ValueError(f"'qv' needs {n_src} rows")
    grad_out = _strided_rows(grad_out, 'grad_out', F)
    n_dst = grad_out.size(0)
    if k.size(0) < n_dst:
        raise ValueError(f"'k' needs at least {n_dst} rows")
    edge_id_t = _edge_id(edge_id_t, rowptr_t, col_t, 'edge_id_t')
    dev = k.device
    if n_src == 0 or col_t.numel() == 0:
        return torch.zeros(n_src, 2 * F, dtype=torch.float32, device=dev)
    grad_qv = torch.empty(n_src, 2 * F, dtype=torch.float32, device=dev)
    g = _csr(rowptr_t, col_t, n_src, hub)
    ws, ws_bytes = _workspace(lib.pygamd_resgated_workspace_bytes, (g.n_chunks, F, 0), dev,
                              g.n_chunks > 0)
    with _timed({'kind': 'resgated', 'op': 'backward_src', 'n_rows': n_src, 'E': col_t.numel(),
                 'F': F, 'De': De, 'ld': _ld(k), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': False}, k):
        check(lib.pygamd_resgated_backward_src(
            ctypes.byref(g), _p(edge_id_t), _p(k), _ld(k), _p(qv), _ld(qv), _p(edge_attr),
            _p(weight), _p(grad_out), _ld(grad_out), n_dst, F, De, _p(grad_qv), _p(ws), ws_bytes,
            _stream(k)), 'resgated_backward_src')
    return grad_qv


# ---- CGConv's gated softplus sum (csrc/cg.hip) ------------------------------------------------------
def cg_supported(F: int, De: int = 0) -> bool:
    """The kernels serve ``F <= 512``; the raw-feature edge mode (``De >= 1``: both edge matrices
    in registers) additionally needs ``De <= 32`` and ``F * De <= 2048``.  Past that a caller
    passes the dense product ``edge_terms [E, 2F]`` instead (``De = 0``)."""
    return bool(_lib.load().pygamd_cg_supported(int(F), int(De)))


def _cg_args(p: Tensor, q: Tensor, edge_attr: Optional[Tensor], weight: Optional[Tensor],
             n_dst: int, E: int):
    """(p, q, mode, edge_attr, weight, F, De) checked: the packed ``p [>= n_dst, 2F]`` and ``q
    [n_src, 2F]`` with their row strides; ``edge_attr [E, De]`` with ``weight [2, F, De]`` (raw
    features, the two matrices in registers), ``edge_attr [E, 2F]`` alone (the dense edge terms)
    or neither."""
    if p.dim() != 2 or p.size(1) % 2:
        raise ValueError("'p' must be a two-dimensional [n, 2F] tensor")
    F = p.size(1) // 2
    p, q = _strided_rows(p, 'p', 2 * F), _strided_rows(q, 'q', 2 * F)
    if p.size(0) < n_dst:
        raise ValueError(f"'p' needs at least {n_dst} rows")
    if edge_attr is None:
        if weight is not None:
            raise ValueError("'weight' comes with 'edge_attr'")
        return p, q, GEN_EDGE_NONE, None, None, F, 0
    edge_attr = _edge_rows(edge_attr, E)
    if weight is None:
        if edge_attr.size(1) != 2 * F:
            raise ValueError(f"without 'weight', 'edge_attr' holds the edge terms [{E}, {2 * F}] "
                             f"(got {tuple(edge_attr.shape)})")
        return p, q, GEN_EDGE_WIDE, edge_attr, None, F, 0
    De = edge_attr.size(1)
    if weight.dtype != torch.float32 or tuple(weight.shape) != (2, F, De) or De < 1:
        raise ValueError(f"'weight' must be float32 [2, {F}, {De}] (got {weight.dtype} "
                         f"{tuple(weight.shape)})")
    return p, q, GEN_EDGE_LINEAR, edge_attr, weight.contiguous(), F, De


def _cg_plane(out: Optional[Tensor], rows: int, n_rows: int, F: int, device, name: str) -> Tensor:
    """the ``[rows, 2F]`` gradient a backward launch writes: the caller's column block of a wider
    plane (rows beyond ``n_rows`` are the caller's to zero) or a fresh tensor"""
    if out is None:
        return _grad_rows(rows, n_rows, 2 * F, device)
    if (out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (rows, 2 * F)
            or (out.numel() > 0 and (out.stride(1) != 1 or out.stride(0) < 2 * F))):
        raise ValueError(f"'{name}' must be a float32 [{rows}, {2 * F}] tensor with unit column "
                         f"stride")
    return out


def _cg_workspace(lib, n_chunks: int, F: int, De: int, device):
    # (no query of its own: the cg entry points take resgated's workspace, include/pyg_amd.h)
    return _workspace(lib.pygamd_resgated_workspace_bytes, (n_chunks, F, De), device,
                      n_chunks > 0 or De > 0)


def cg_forward(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], p: Tensor, q: Tensor,
               edge_attr: Optional[Tensor] = None, weight: Optional[Tensor] = None, *,
               residual: Optional[Tensor] = None, mean: bool = False, hub=None) -> Tensor:
    """``out [n_rows, F] = epilogue(sum_k sigmoid(zf_k) * softplus(zs_k))`` on a by-destination
    handle with ``[zf_k | zs_k] = p[i] + q[col[k]] + (edge terms of edge_id[k])``; the edge modes
    are :func:`_cg_args`'s.  ``mean`` divides by the row's slot count, ``residual [>= n_rows, F]``
    is added after that; a row without slots is exactly its residual (or 0).  ``p``, ``q`` and
    ``residual`` may be column blocks of wider tensors."""
    _require_device(rowptr, col, edge_id, p, q, edge_attr, weight, residual)
    lib = _lib.load()
    n_rows = rowptr.numel() - 1
    p, q, mode, edge_attr, weight, F, De = _cg_args(p, q, edge_attr, weight, n_rows, col.numel())
    if residual is not None:
        residual = _strided_rows(residual, 'residual', F)
        if residual.size(0) < n_rows:
            raise ValueError(f"'residual' needs at least {n_rows} rows")
    edge_id = _edge_id(edge_id, rowptr, col)
    dev = p.device
    if n_rows == 0 or col.numel() == 0:  # no slot anywhere: the epilogue alone, nothing to launch
        if residual is None:
            return torch.zeros(n_rows, F, dtype=torch.float32, device=dev)
        return residual[:n_rows].clone(memory_format=torch.contiguous_format)
    out = torch.empty(n_rows, F, dtype=torch.float32, device=dev)
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _cg_workspace(lib, g.n_chunks, F, 0, dev)
    with _timed({'kind': 'cg', 'op': 'forward', 'n_rows': n_rows, 'E': col.numel(), 'F': F,
                 'De': De, 'mode': mode, 'ld': _ld(q), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': False}, p):
        check(lib.pygamd_cg_forward(
            ctypes.byref(g), _p(edge_id), _p(p), _ld(p), _p(q), _ld(q), mode, _p(edge_attr),
            _p(weight), _p(residual), 0 if residual is None else _ld(residual), int(bool(mean)),
            q.size(0), F, De, _p(out), _p(ws), ws_bytes, _stream(p)), 'cg_forward')
    return out


def cg_backward_dst(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], p: Tensor, q: Tensor,
                    edge_attr: Optional[Tensor], weight: Optional[Tensor], grad_out: Tensor, *,
                    mean: bool = False, want_grad_edge: bool = True,
                    out: Optional[Tensor] = None, hub=None):
    """``(grad_p [rows of p, 2F], grad_edge | None, grad_weight [2, F, De] | None)`` on the
    forward's by-destination handle: ``grad_p[i] = [sum gzf | sum gzs]`` with both activations
    recomputed.  ``grad_edge`` is ``grad_edge_attr [E, De]`` with raw features and the per-slot
    ``[gzf | gzs]``, the gradient of the edge terms ``[E, 2F]``, with dense ones, in the caller's
    edge order.  ``out``: the ``[rows of p, 2F]`` column block of a wider plane to write ``grad_p``
    into (its rows past ``n_rows`` are left alone)."""
    _require_device(rowptr, col, edge_id, p, q, edge_attr, weight, grad_out, out)
    lib = _lib.load()
    n_rows = rowptr.numel() - 1
    p, q, mode, edge_attr, weight, F, De = _cg_args(p, q, edge_attr, weight, n_rows, col.numel())
    grad_out = _strided_rows(grad_out, 'grad_out', F)
    if grad_out.size(0) != n_rows:
        raise ValueError(f"'grad_out' needs {n_rows} rows")
    edge_id = _edge_id(edge_id, rowptr, col)
    want_grad_edge = bool(want_grad_edge) and mode != GEN_EDGE_NONE
    dev = p.device
    grad_p = _cg_plane(out, p.size(0), n_rows, F, dev, 'out')
    grad_edge = torch.empty_like(edge_attr) if want_grad_edge else None
    grad_w = torch.empty_like(weight) if weight is not None else None
    if n_rows == 0 or col.numel() == 0:
        grad_p[:n_rows].zero_()
        return (grad_p, None if grad_edge is None else grad_edge.zero_(),
                None if grad_w is None else grad_w.zero_())
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _cg_workspace(lib, g.n_chunks, F, De, dev)
    with _timed({'kind': 'cg', 'op': 'backward_dst', 'n_rows': n_rows, 'E': col.numel(), 'F': F,
                 'De': De, 'mode': mode, 'ld': _ld(q), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': want_grad_edge}, p):
        check(lib.pygamd_cg_backward_dst(
            ctypes.byref(g), _p(edge_id), _p(p), _ld(p), _p(q), _ld(q), mode, _p(edge_attr),
            _p(weight), _p(grad_out), _ld(grad_out), int(bool(mean)), q.size(0), F, De,
            _p(grad_p), _ld(grad_p), _p(grad_edge), _p(grad_w), _p(ws), ws_bytes, _stream(p)),
            'cg_backward_dst')
    return grad_p, grad_edge, grad_w


def cg_backward_src(rowptr_t: Tensor, col_t: Tensor, edge_id_t: Optional[Tensor], p: Tensor,
                    q: Tensor, edge_attr: Optional[Tensor], weight: Optional[Tensor],
                    grad_out: Tensor, *, dst_rowptr: Optional[Tensor] = None,
                    out: Optional[Tensor] = None, hub=None) -> Tensor:
    """``grad_q [n_src, 2F] = [sum gzf | sum gzs]`` on the by-SOURCE handle (``col_t`` = the
    destination of every out-slot, ``edge_id_t`` = that form's slot -> edge map).  ``p`` and
    ``grad_out`` are gathered per slot at their own row strides.  ``dst_rowptr``: the
    by-destination ``rowptr`` of a mean aggregation (None: sum).  ``out``: the ``[n_src, 2F]``
    column block of a wider plane to write into."""
    _require_device(rowptr_t, col_t, edge_id_t, p, q, edge_attr, weight, grad_out, dst_rowptr, out)
    lib = _lib.load()
    n_src = rowptr_t.numel() - 1
    p, q, mode, edge_attr, weight, F, De = _cg_args(p, q, edge_attr, weight, 0, col_t.numel())
    if q.size(0) != n_src:
        raise ValueError(f"'q' needs {n_src} rows")
    grad_out = _strided_rows(grad_out, 'grad_out', F)
    n_dst = grad_out.size(0)
    if p.size(0) < n_dst:
        raise ValueError(f"'p' needs at least {n_dst} rows")
    if dst_rowptr is not None:
        if dst_rowptr.dtype != rowptr_t.dtype or dst_rowptr.numel() != n_dst + 1:
            raise ValueError(f"'dst_rowptr' must have the index dtype and {n_dst + 1} entries")
        dst_rowptr = dst_rowptr.contiguous()
    edge_id_t = _edge_id(edge_id_t, rowptr_t, col_t, 'edge_id_t')
    dev = p.device
    grad_q = _cg_plane(out, n_src, n_src, F, dev, 'out')
    if n_src == 0 or col_t.numel() == 0:
        return grad_q.zero_()
    g = _csr(rowptr_t, col_t, n_src, hub)
    ws, ws_bytes = _cg_workspace(lib, g.n_chunks, F, 0, dev)
    with _timed({'kind': 'cg', 'op': 'backward_src', 'n_rows': n_src, 'E': col_t.numel(), 'F': F,
                 'De': De, 'mode': mode, 'ld': _ld(p), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks,
                 'grad_edge_attr': False}, p):
        check(lib.pygamd_cg_backward_src(
            ctypes.byref(g), _p(edge_id_t), _p(p), _ld(p), _p(q), _ld(q), mode, _p(edge_attr),
            _p(weight), _p(grad_out), _ld(grad_out), int(dst_rowptr is not None),
            _p(dst_rowptr), n_dst, F, De, _p(grad_q), _ld(grad_q), _p(ws), ws_bytes, _stream(p)),
            'cg_backward_src')
    return grad_q


# ---- FiLMConv's typed feature modulation (csrc/film.hip) -------------------------------------------
def film_supported(F: int) -> bool:
    """The kernels serve ``1 <= F <= 512``."""
    return bool(_lib.load().pygamd_film_supported(int(F)))


def _film_args(h: Tensor, gb: Tensor, R: int):
    """(h, gb, F) checked: ``h [n_src, R * F]`` and ``gb [>= n_dst, R * 2F]`` (block ``r`` =
    ``[beta_r | gamma_r]``) with their row strides — two tensors or column blocks of one plane."""
    R = int(R)
    if R < 1 or h.dim() != 2 or h.size(1) % R or h.size(1) == 0:
        raise ValueError(f"'h' must be a two-dimensional [n, R * F] tensor with R = {R}")
    F = h.size(1) // R
    return _strided_rows(h, 'h', R * F), _strided_rows(gb, 'gb', 2 * R * F), F


def _film_rel(rel: Tensor, E: int) -> Tensor:
    if rel.dtype != torch.int32 or rel.dim() != 1 or rel.numel() != E:
        raise ValueError(f"'rel' must be an int32 [{E}] tensor (got {rel.dtype} "
                         f"{tuple(rel.shape)})")
    return rel.contiguous()


def _film_scale(scale: Optional[Tensor], E: int) -> Optional[Tensor]:
    if scale is None:
        return None
    if scale.dtype != torch.float32 or scale.dim() != 1 or scale.numel() != E:
        raise ValueError(f"'scale' must be a float32 [{E}] tensor (got {scale.dtype} "
                         f"{tuple(scale.shape)})")
    return scale.contiguous()


def _film_pairs(rowptr: Tensor, pair_rel: Tensor, pair_node: Tensor):
    n = rowptr.numel() - 1
    for name, t in (('pair_rel', pair_rel), ('pair_node', pair_node)):
        if t.dtype != rowptr.dtype or t.dim() != 1 or t.numel() != n:
            raise ValueError(f"'{name}' must have the index dtype and one entry per pair row")
    return pair_rel.contiguous(), pair_node.contiguous()


def _film_plane(out: Tensor, rows: int, width: int, name: str) -> Tensor:
    """the zero-filled ``[rows, width]`` gradient block a backward launch writes into: a tensor of
    the caller's, or a column block of a wider plane"""
    if (out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (rows, width)
            or (out.numel() > 0 and (out.stride(1) != 1 or out.stride(0) < width))):
        raise ValueError(f"'{name}' must be a float32 [{rows}, {width}] tensor with unit column "
                         f"stride")
    return out


def _film_workspace(lib, n_chunks: int, F: int, device):
    # (no query of its own: the film entry points take resgated's workspace, include/pyg_amd.h)
    return _workspace(lib.pygamd_resgated_workspace_bytes, (n_chunks, F, 0), device, n_chunks > 0)


def film_forward(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], rel: Tensor, h: Tensor,
                 gb: Tensor, R: int, *, scale: Optional[Tensor] = None,
                 residual: Optional[Tensor] = None, relu: bool = True, hub=None) -> Tensor:
    """``out [n_rows, F] = residual + sum_k scale[e] * act(gamma * h[col[k], rF:(r+1)F] + beta)`` on
    a by-destination handle with ``e = edge_id[k]``, ``r = rel[e]`` (int32, in ``[0, R)``: the
    caller's to guarantee) and ``[beta | gamma] = gb[i, r * 2F:(r + 1) * 2F]``.  ``scale [E]``: the
    per-edge mean normaliser (None: sum).  ``relu=False``: no activation.  A row without slots is
    exactly its residual (or 0).  ``h``, ``gb`` and ``residual`` may be column blocks of wider
    tensors."""
    _require_device(rowptr, col, edge_id, rel, h, gb, scale, residual)
    lib = _lib.load()
    n_rows = rowptr.numel() - 1
    h, gb, F = _film_args(h, gb, R)
    if gb.size(0) < n_rows:
        raise ValueError(f"'gb' needs at least {n_rows} rows")
    E = col.numel()
    rel, scale = _film_rel(rel, E), _film_scale(scale, E)
    if residual is not None:
        residual = _strided_rows(residual, 'residual', F)
        if residual.size(0) < n_rows:
            raise ValueError(f"'residual' needs at least {n_rows} rows")
    edge_id = _edge_id(edge_id, rowptr, col)
    dev = h.device
    if n_rows == 0 or E == 0:  # no slot anywhere: the epilogue alone, nothing to launch
        if residual is None:
            return torch.zeros(n_rows, F, dtype=torch.float32, device=dev)
        return residual[:n_rows].clone(memory_format=torch.contiguous_format)
    out = torch.empty(n_rows, F, dtype=torch.float32, device=dev)
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _film_workspace(lib, g.n_chunks, F, dev)
    with _timed({'kind': 'film', 'op': 'forward', 'n_rows': n_rows, 'E': E, 'F': F, 'R': int(R),
                 'ld': _ld(h), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, h):
        check(lib.pygamd_film_forward(
            ctypes.byref(g), _p(edge_id), _p(rel), _p(h), _ld(h), _p(gb), _ld(gb), _p(scale),
            _p(residual), 0 if residual is None else _ld(residual), int(bool(relu)), h.size(0),
            F, int(R), _p(out), _p(ws), ws_bytes, _stream(h)), 'film_forward')
    return out


def film_backward_dst(rowptr: Tensor, col: Tensor, pair_rel: Tensor, pair_dst: Tensor, h: Tensor,
                      gb: Tensor, R: int, grad_out: Tensor, out: Tensor, *, mean: bool = False,
                      relu: bool = True, hub=None) -> Tensor:
    """Writes ``out[i, r * 2F:(r + 1) * 2F] = [sum gm | sum gm * h]`` (``gm = grad_out[i] *
    act'(pre)``, for ``mean`` divided by the pair row's length) for every row ``p`` of the
    ``(relation, destination)`` pair handle, ``r = pair_rel[p]``, ``i = pair_dst[p]``, ``col`` =
    the sources of its slots.  ``out [rows of gb, R * 2F]`` is the caller's zero-filled plane, or
    a column block of one: blocks of pairs that do not occur are left alone."""
    _require_device(rowptr, col, pair_rel, pair_dst, h, gb, grad_out, out)
    lib = _lib.load()
    n_rows = rowptr.numel() - 1
    h, gb, F = _film_args(h, gb, R)
    grad_out = _strided_rows(grad_out, 'grad_out', F)
    if gb.size(0) < grad_out.size(0):
        raise ValueError(f"'gb' needs at least {grad_out.size(0)} rows")
    out = _film_plane(out, gb.size(0), 2 * int(R) * F, 'out')
    pair_rel, pair_dst = _film_pairs(rowptr, pair_rel, pair_dst)
    if n_rows == 0 or col.numel() == 0:
        return out
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _film_workspace(lib, g.n_chunks, F, h.device)
    with _timed({'kind': 'film', 'op': 'backward_dst', 'n_rows': n_rows, 'E': col.numel(), 'F': F,
                 'R': int(R), 'ld': _ld(h), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, h):
        check(lib.pygamd_film_backward_dst(
            ctypes.byref(g), _p(pair_rel), _p(pair_dst), _p(h), _ld(h), _p(gb), _ld(gb),
            _p(grad_out), _ld(grad_out), int(bool(relu)), int(bool(mean)), h.size(0), F, int(R),
            _p(out), _ld(out), _p(ws), ws_bytes, _stream(h)), 'film_backward_dst')
    return out


def film_backward_src(rowptr_t: Tensor, col_t: Tensor, edge_id_t: Optional[Tensor],
                      pair_rel: Tensor, pair_src: Tensor, h: Tensor, gb: Tensor, R: int,
                      grad_out: Tensor, out: Tensor, *, scale: Optional[Tensor] = None,
                      relu: bool = True, hub=None) -> Tensor:
    """Writes ``out[j, r * F:(r + 1) * F] = sum scale[e] * grad_out[i] * act'(pre) * gamma_{r,i}``
    for every row ``p`` of the ``(relation, source)`` pair handle of the flipped graph, ``r =
    pair_rel[p]``, ``j = pair_src[p]``, ``col_t`` = the destinations of its slots, ``edge_id_t`` =
    that handle's slot -> edge map (for ``scale``).  ``out [n_src, R * F]`` is the caller's
    zero-filled plane, or a column block of one."""
    _require_device(rowptr_t, col_t, edge_id_t, pair_rel, pair_src, h, gb, scale, grad_out, out)
    lib = _lib.load()
    n_rows = rowptr_t.numel() - 1
    h, gb, F = _film_args(h, gb, R)
    grad_out = _strided_rows(grad_out, 'grad_out', F)
    n_dst = grad_out.size(0)
    if gb.size(0) < n_dst:
        raise ValueError(f"'gb' needs at least {n_dst} rows")
    out = _film_plane(out, h.size(0), int(R) * F, 'out')
    pair_rel, pair_src = _film_pairs(rowptr_t, pair_rel, pair_src)
    scale = _film_scale(scale, col_t.numel())
    edge_id_t = _edge_id(edge_id_t, rowptr_t, col_t, 'edge_id_t')
    if n_rows == 0 or col_t.numel() == 0:
        return out
    g = _csr(rowptr_t, col_t, n_rows, hub)
    ws, ws_bytes = _film_workspace(lib, g.n_chunks, F, h.device)
    with _timed({'kind': 'film', 'op': 'backward_src', 'n_rows': n_rows, 'E': col_t.numel(),
                 'F': F, 'R': int(R), 'ld': _ld(gb), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks},
                h):
        check(lib.pygamd_film_backward_src(
            ctypes.byref(g), _p(edge_id_t), _p(pair_rel), _p(pair_src), _p(h), _ld(h), _p(gb),
            _ld(gb), _p(scale), _p(grad_out), _ld(grad_out), int(bool(relu)), n_dst, F, int(R),
            _p(out), _ld(out), _p(ws), ws_bytes, _stream(h)), 'film_backward_src')
    return out


# ---- RGATConv's additive relational attention (csrc/rgat.hip) --------------------------------------
def rgat_supported(H: int, C: int) -> bool:
    """The one-pass kernels serve this head layout (H * C <= 512, H <= 64)."""
    return bool(_lib.load().pygamd_rgat_supported(int(H), int(C)))


# (no workspace query of its own: the rgat entry points take han's workspace, include/pyg_amd.h)
def _rgat_planes(p: Tensor, qi: Tensor, kj: Tensor, R: int, H: int, C: int):
    """``P [n, R * H * C]``, ``QI`` and ``KJ [n, R * H]`` with their row strides: three tensors or
    the column blocks of one packed plane"""
    return (_strided_rows(p, 'p', R * H * C), _strided_rows(qi, 'qi', R * H),
            _strided_rows(kj, 'kj', R * H))


def _rgat_bias(b: Optional[Tensor], E: int, H: int) -> Optional[Tensor]:
    if b is None:
        return None
    if b.dtype != torch.float32 or tuple(b.shape) != (E, H):
        raise ValueError(f"'b' must be a float32 [{E}, {H}] tensor (got {b.dtype} "
                         f"{tuple(b.shape)})")
    return b.contiguous()


def _rgat_slots(rel: Tensor, b: Optional[Tensor], E: int, H: int):
    return _film_rel(rel, E), _rgat_bias(b, E, H)


def rgat_forward(rowptr: Tensor, col: Tensor, rel: Tensor, p: Tensor, qi: Tensor, kj: Tensor,
                 b: Optional[Tensor], R: int, H: int, C: int, slope: float, *,
                 pair_stats: Optional[Tensor] = None, hub=None):
    """``(alpha [nnz, H] in slot order, out [n_rows, H * C])`` of RGAT's additive attention on a
    by-destination handle: ``rel`` (int32, per SLOT, in ``[0, R)``: the caller's to guarantee, as
    the range of ``col``), ``p [n_src, R * H * C]``, ``qi [>= n_rows, R * H]``, ``kj [n_src, R *
    H]`` (column blocks of wider tensors are read in place), ``b [nnz, H]`` the optional score
    bias in slot order.  ``pair_stats`` None: the softmax across all relations of a destination;
    the ``[n_rows, R, 2 H]`` of :func:`rgat_pair_stats`: within every relation."""
    _require_device(rowptr, col, rel, p, qi, kj, b, pair_stats)
    lib = _lib.load()
    R, H, C = int(R), int(H), int(C)
    p, qi, kj = _rgat_planes(p, qi, kj, R, H, C)
    n_rows, E = rowptr.numel() - 1, col.numel()
    if qi.size(0) < n_rows or kj.size(0) != p.size(0):
        raise ValueError(f"'qi' needs at least {n_rows} rows and 'kj' the rows of 'p'")
    rel, b = _rgat_slots(rel, b, E, H)
    if pair_stats is not None and (pair_stats.dtype != torch.float32
                                   or not pair_stats.is_contiguous()
                                   or pair_stats.numel() != n_rows * R * 2 * H):
        raise ValueError(f"'pair_stats' must be a contiguous float32 [{n_rows}, {R}, {2 * H}]")
    alpha = torch.empty(E, H, dtype=torch.float32, device=p.device)
    out = torch.empty(n_rows, H * C, dtype=torch.float32, device=p.device)
    if E == 0 or n_rows == 0:  # no edges: every row is empty
        return alpha, out.zero_()
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_han_workspace_bytes, (g.n_chunks, H, C), p.device,
                              g.n_chunks > 0)
    with _timed({'kind': 'rgat', 'op': 'forward', 'n_rows': n_rows, 'E': E, 'H': H, 'C': C,
                 'R': R, 'ld': _ld(p), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, p):
        check(lib.pygamd_rgat_forward(
            ctypes.byref(g), _p(rel), _p(p), _ld(p), _p(qi), _ld(qi), _p(kj), _ld(kj), _p(b),
            _p(pair_stats), p.size(0), H, C, R, float(slope), _p(alpha), _p(out), _p(ws),
            ws_bytes, _stream(p)), 'rgat_forward')
    return alpha, out


def rgat_backward_dst(rowptr: Tensor, col: Tensor, rel: Tensor, p: Tensor, qi: Tensor, kj: Tensor,
                      b: Optional[Tensor], alpha: Tensor, grad_out: Tensor, out: Tensor, R: int,
                      H: int, C: int, slope: float, *, within: bool = False, hub=None) -> Tensor:
    """``grad_s [nnz, H]`` in slot order (also the gradient of ``b``) on the forward's handle;
    ``within``: the raw ``d alpha`` that :func:`rgat_pair_finish` turns into ``grad_s``."""
    _require_device(rowptr, col, rel, p, qi, kj, b, alpha, grad_out, out)
    lib = _lib.load()
    R, H, C = int(R), int(H), int(C)
    p, qi, kj = _rgat_planes(p, qi, kj, R, H, C)
    n_rows, E = rowptr.numel() - 1, col.numel()
    grad_out, out = _dense_rows(grad_out, 'grad_out', H * C), _dense_rows(out, 'out', H * C)
    if (qi.size(0) < n_rows or kj.size(0) != p.size(0) or out.size(0) != n_rows
            or grad_out.size(0) != n_rows or tuple(alpha.shape) != (E, H)):
        raise ValueError(f"'qi', 'out' and 'grad_out' need the {n_rows} rows of the handle, "
                         f"'alpha' one row per slot")
    rel, b = _rgat_slots(rel, b, E, H)
    alpha = alpha.contiguous()
    grad_s = torch.empty_like(alpha)
    if E == 0 or n_rows == 0:
        return grad_s
    g = _csr(rowptr, col, n_rows, hub)
    with _timed({'kind': 'rgat', 'op': 'backward_dst', 'n_rows': n_rows, 'E': E, 'H': H, 'C': C,
                 'R': R, 'ld': _ld(p), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, p):
        check(lib.pygamd_rgat_backward_dst(
            ctypes.byref(g), _p(rel), _p(p), _ld(p), _p(qi), _ld(qi), _p(kj), _ld(kj), _p(b),
            _p(alpha), _p(grad_out), _p(out), p.size(0), H, C, R, float(slope),
            int(bool(within)), _p(grad_s), _stream(p)), 'rgat_backward_dst')
    return grad_s


def _rgat_pair_call(rowptr, col, slot_map, pair_rel, pair_dst, qi, kj, b, alpha, R, H, slope,
                    grad_s, stats, grad_qi, op):
    _require_device(rowptr, col, slot_map, pair_rel, pair_dst, qi, kj, b, alpha, grad_s, stats,
                    grad_qi)
    lib = _lib.load()
    R, H = int(R), int(H)
    n_rows, E = rowptr.numel() - 1, col.numel()
    qi, kj = _strided_rows(qi, 'qi', R * H), _strided_rows(kj, 'kj', R * H)
    pair_rel, pair_dst = _film_pairs(rowptr, pair_rel, pair_dst)
    if slot_map.dtype != rowptr.dtype or slot_map.numel() != E:
        raise ValueError("'slot_map' must have the index dtype and one entry per slot")
    slot_map = slot_map.contiguous()
    b = _rgat_bias(b, E, H)
    if n_rows == 0 or E == 0:
        return
    g = _csr(rowptr, col, n_rows, None)   # (every pair row whole)
    with _timed({'kind': 'rgat', 'op': op, 'n_rows': n_rows, 'E': E, 'H': H, 'R': R}, qi):
        check(lib.pygamd_rgat_pair_scalar(
            ctypes.byref(g), _p(slot_map), _p(pair_rel), _p(pair_dst), _p(qi), _ld(qi), _p(kj),
            _ld(kj), _p(b), _p(alpha), kj.size(0), H, R, float(slope), _p(grad_s), _p(stats),
            _p(grad_qi), 0 if grad_qi is None else _ld(grad_qi), _stream(qi)), 'rgat_' + op)


def rgat_pair_stats(rowptr: Tensor, col: Tensor, slot_map: Tensor, pair_rel: Tensor,
                    pair_dst: Tensor, qi: Tensor, kj: Tensor, b: Optional[Tensor], n_dst: int,
                    R: int, H: int, slope: float) -> Tensor:
    """The within-relation normaliser ``[n_dst, R, 2 H]`` = per ``(destination, relation)`` pair
    the (maximum ``[H]``, ``1 / (sum + 1e-16) [H]``) of its scores, from one scalar launch over the
    ``(relation, destination)`` pair rows; pairs that do not occur stay uninitialised (and are
    never read)."""
    stats = torch.empty(int(n_dst), int(R), 2 * int(H), dtype=torch.float32, device=qi.device)
    if qi.size(0) < n_dst:
        raise ValueError(f"'qi' needs at least {n_dst} rows")
    _rgat_pair_call(rowptr, col, slot_map, pair_rel, pair_dst, qi, kj, b, None, R, H, slope, None,
                    stats, None, 'pair_stats')
    return stats


def rgat_pair_finish(rowptr: Tensor, col: Tensor, slot_map: Tensor, pair_rel: Tensor,
                     pair_dst: Tensor, qi: Tensor, kj: Tensor, b: Optional[Tensor], alpha: Tensor,
                     grad_s: Tensor, R: int, H: int, slope: float, grad_qi: Tensor) -> None:
    """Within-relation backward over the ``(relation, destination)`` pair rows: ``grad_s`` (the
    raw ``d alpha`` of :func:`rgat_backward_dst` with ``within``) becomes ``alpha (d alpha - D) *
    leaky_relu'`` in place, ``D`` the pair's ``sum alpha * d alpha``, and ``grad_qi[i, r * H:(r +
    1) * H] = sum grad_s`` (the caller's zero-filled plane, or a column block of one)."""
    E = col.numel()
    if (tuple(alpha.shape) != (E, H) or tuple(grad_s.shape) != (E, H)
            or not alpha.is_contiguous() or not grad_s.is_contiguous()):
        raise ValueError(f"'alpha' and 'grad_s' must be contiguous [{E}, {H}]")
    grad_qi = _film_plane(grad_qi, grad_qi.size(0), int(R) * int(H), 'grad_qi')
    if grad_qi.size(0) != qi.size(0):
        raise ValueError("'grad_qi' needs the rows of 'qi'")
    _rgat_pair_call(rowptr, col, slot_map, pair_rel, pair_dst, qi, kj, b, alpha, R, H, slope,
                    grad_s, None, grad_qi, 'pair_finish')


def rgat_backward_src(rowptr: Tensor, col: Tensor, slot_map: Tensor, pair_rel: Tensor,
                      pair_node: Tensor, alpha: Tensor, grad_s: Tensor,
                      grad_out: Optional[Tensor], R: int, H: int, C: int, grad_a: Tensor,
                      grad_p: Optional[Tensor] = None, *, hub=None) -> None:
    """Over the ``(relation, node)`` pair rows of a pair handle (``col`` = the other endpoint,
    ``slot_map`` = pair slot -> by-destination slot): ``grad_a[node, r * H:(r + 1) * H] = sum
    grad_s`` and, with ``grad_p``, ``grad_p[node, r * H * C:(r + 1) * H * C] = sum alpha *
    grad_out[col]``.  Both are the caller's zero-filled planes, or column blocks of one: blocks of
    pairs that do not occur are left alone."""
    _require_device(rowptr, col, slot_map, pair_rel, pair_node, alpha, grad_s, grad_out, grad_a,
                    grad_p)
    lib = _lib.load()
    R, H, C = int(R), int(H), int(C)
    n_rows, E = rowptr.numel() - 1, col.numel()
    pair_rel, pair_node = _film_pairs(rowptr, pair_rel, pair_node)
    if slot_map.dtype != rowptr.dtype or slot_map.numel() != E:
        raise ValueError("'slot_map' must have the index dtype and one entry per slot")
    slot_map = slot_map.contiguous()
    if tuple(alpha.shape) != (E, H) or tuple(grad_s.shape) != (E, H):
        raise ValueError(f"'alpha' and 'grad_s' must be [{E}, {H}]")
    alpha, grad_s = alpha.contiguous(), grad_s.contiguous()
    grad_a = _film_plane(grad_a, grad_a.size(0), R * H, 'grad_a')
    n_other = 0
    if grad_p is not None:
        grad_p = _film_plane(grad_p, grad_a.size(0), R * H * C, 'grad_p')
        grad_out = _dense_rows(grad_out, 'grad_out', H * C)
        n_other = grad_out.size(0)
    if n_rows == 0 or E == 0:
        return
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_han_workspace_bytes, (g.n_chunks, H, C), alpha.device,
                              g.n_chunks > 0)
    with _timed({'kind': 'rgat', 'op': 'backward_src', 'n_rows': n_rows, 'E': E, 'H': H, 'C': C,
                 'R': R, 'rows': grad_p is not None, 'n_hub': g.n_hub, 'n_chunks': g.n_chunks},
                alpha):
        check(lib.pygamd_rgat_backward_src(
            ctypes.byref(g), _p(slot_map), _p(pair_rel), _p(pair_node), _p(alpha), _p(grad_s),
            _p(grad_out) if grad_p is not None else None, n_other, H, C, R, _p(grad_a),
            _ld(grad_a), _p(grad_p), 0 if grad_p is None else _ld(grad_p), _p(ws), ws_bytes,
            _stream(alpha)), 'rgat_backward_src')


# ---- mixture messages, aggregate first (csrc/mixture.hip) ------------------------------------------
def mixture_supported(F: int, K: int) -> bool:
    """The kernels serve rows of ``1 <= F <= 512`` floats and ``1 <= K <= 256`` coefficients per
    edge."""
    return bool(_lib.load().pygamd_mixture_supported(int(F), int(K)))


def _mixture_coef(coef: Tensor, E: int, name: str = 'coef') -> Tensor:
    if coef.dtype != torch.float32 or coef.dim() != 2 or coef.size(0) != E or coef.size(1) < 1:
        raise ValueError(f"'{name}' must be a float32 [{E}, K] tensor (got {coef.dtype} "
                         f"{tuple(coef.shape)})")
    return coef.contiguous()


def mixture_expand(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], x: Tensor,
                   coef: Tensor, *, hub=None) -> Tensor:
    """``Z [n_rows, K * F]`` with ``Z[r, k * F + f] = sum_{slots s of r} coef[edge_id[s], k] *
    x[col[s], f]`` over a sorted handle: the forward's by destination, or the transposed one with
    ``x := grad_out`` for the gradient of ``x``.  ``x`` may be a column block of a wider tensor
    (its row stride is passed); ``coef [E, K]`` stays in the caller's edge order (``edge_id=None``:
    it follows the slots).  Rows without slots are exactly 0."""
    _require_device(rowptr, col, edge_id, x, coef)
    lib = _lib.load()
    n_rows = rowptr.numel() - 1
    if x.dim() != 2:
        raise ValueError("'x' must be two-dimensional")
    F = x.size(1)
    x = _strided_rows(x, 'x', F)
    coef = _mixture_coef(coef, col.numel())
    K = coef.size(1)
    edge_id = _edge_id(edge_id, rowptr, col)
    dev = x.device
    if n_rows == 0 or col.numel() == 0:  # no slot anywhere: zeros, nothing to launch
        return torch.zeros(n_rows, K * F, dtype=torch.float32, device=dev)
    z = torch.empty(n_rows, K * F, dtype=torch.float32, device=dev)
    g = _csr(rowptr, col, n_rows, hub)
    ws, ws_bytes = _workspace(lib.pygamd_mixture_workspace_bytes, (g.n_chunks, F, K), dev,
                              g.n_chunks > 0)
    with _timed({'kind': 'mixture', 'op': 'expand', 'n_rows': n_rows, 'E': col.numel(), 'F': F,
                 'K': K, 'ld': _ld(x), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, x):
        check(lib.pygamd_mixture_expand(
            ctypes.byref(g), _p(edge_id), _p(x), _ld(x), _p(coef), x.size(0), F, K, _p(z), _p(ws),
            ws_bytes, _stream(x)), 'mixture_expand')
    return z


def mixture_coef_grad(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], wide: Tensor,
                      x: Tensor, *, hub=None) -> Tensor:
    """``grad_coef [E, K]`` with ``grad_coef[edge_id[s], k] = <wide[r, k * F : (k + 1) * F],
    x[col[s], :]>`` for every slot ``s`` of every row ``r`` of the by-destination handle; ``wide
    [n_rows, K * F]`` is contiguous, ``x`` may be a column block."""
    _require_device(rowptr, col, edge_id, wide, x)
    lib = _lib.load()
    n_rows = rowptr.numel() - 1
    if x.dim() != 2:
        raise ValueError("'x' must be two-dimensional")
    F = x.size(1)
    x = _strided_rows(x, 'x', F)
    if (wide.dtype != torch.float32 or wide.dim() != 2 or wide.size(0) != n_rows or F < 1
            or wide.size(1) < F or wide.size(1) % F):
        raise ValueError(f"'wide' must be a float32 [{n_rows}, K * {F}] tensor (got {wide.dtype} "
                         f"{tuple(wide.shape)})")
    wide = wide.contiguous()
    K = wide.size(1) // F
    edge_id = _edge_id(edge_id, rowptr, col)
    grad = torch.empty(col.numel(), K, dtype=torch.float32, device=x.device)
    if n_rows == 0 or col.numel() == 0:
        return grad
    g = _csr(rowptr, col, n_rows, hub)
    with _timed({'kind': 'mixture', 'op': 'coef_grad', 'n_rows': n_rows, 'E': col.numel(), 'F': F,
                 'K': K, 'ld': _ld(x), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, x):
        check(lib.pygamd_mixture_coef_grad(
            ctypes.byref(g), _p(edge_id), _p(wide), _p(x), _ld(x), x.size(0), F, K, _p(grad),
            _stream(x)), 'mixture_coef_grad')
    return grad


# ---- per-graph normalisation (csrc/graph_norm.hip) -------------------------------------------------
# The hub plan over a by-graph pointer: a graph of more than GRAPH_NORM_THRESHOLD nodes is walked as
# chunks of GRAPH_NORM_CHUNK nodes, one wave each (profiles/graph_norm.md).
GRAPH_NORM_THRESHOLD = 256
GRAPH_NORM_CHUNK = 128
GRAPH_NORM_BLOCKS = _lib.CONSTANTS['PYGAMD_GRAPH_NORM_BLOCKS']
NORM_MODES = {'channel': _lib.CONSTANTS['PYGAMD_NORM_CHANNEL'],
              'graph': _lib.CONSTANTS['PYGAMD_NORM_GRAPH']}


def graph_norm_supported(F: int) -> bool:
    """The per-graph normalisation kernels serve rows of ``1 <= F <= 512`` floats."""
    return bool(_lib.load().pygamd_graph_norm_supported(int(F)))


def graph_norm_workspace_bytes(n_chunks: int, n_hub: int, F: int, backward: bool) -> int:
    """The workspace formula include/pyg_amd.h states for ``pygamd_graph_norm_*`` (there is no
    query in the C ABI): the chunks' partial sums and, backward, the hub graphs' coefficients and
    the workgroups' partials of the parameter gradients."""
    if backward:
        return 4 * F * (2 * n_chunks + 3 * n_hub + 3 * GRAPH_NORM_BLOCKS)
    return 8 * F * n_chunks


def graph_norm_plan(ptr: Tensor) -> HubPlan:
    """The hub plan of a by-graph pointer at this kernel's threshold and chunk."""
    return hub_plan(ptr, GRAPH_NORM_THRESHOLD, GRAPH_NORM_CHUNK)


def _norm_handle(ptr: Tensor, hub: Optional[HubPlan]) -> Csr:
    """``pygamd_csr`` of a by-graph pointer: no column array, the plan's own threshold and chunk"""
    if hub is None:
        hub = no_hubs(GRAPH_NORM_THRESHOLD, GRAPH_NORM_CHUNK)
    rows, cptr, n_hub, n_chunks, threshold, chunk = hub
    g = Csr(rowptr=ptr.data_ptr(), col=None, idx_dtype=_idx_dtype(ptr), n_rows=ptr.numel() - 1,
            hub_rows=None if rows is None else rows.data_ptr(),
            hub_chunk_ptr=None if cptr is None else cptr.data_ptr(), n_hub=n_hub,
            n_chunks=n_chunks, hub_threshold=threshold, hub_chunk=chunk)
    g._keep = (ptr, hub)
    return g


def _norm_param(t: Optional[Tensor], F: int, name: str) -> Optional[Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32 or tuple(t.shape) != (F, ):
        raise ValueError(f"'{name}' must be a float32 [{F}] tensor (got {t.dtype} "
                         f"{tuple(t.shape)})")
    return t.contiguous()


def _norm_mode(mode: str, mean_scale, std_eps: bool) -> int:
    if mode not in NORM_MODES:
        raise ValueError(f"'mode' must be 'channel' or 'graph' (got {mode!r})")
    if mode == 'graph' and mean_scale is not None:
        raise ValueError("'mean_scale' belongs to mode='channel'")
    if mode == 'channel' and std_eps:
        raise ValueError("'std_eps' belongs to mode='graph'")
    return NORM_MODES[mode]


def graph_norm_forward(ptr: Tensor, x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                       mean_scale: Optional[Tensor], eps: float, mode: str, *,
                       std_eps: bool = False, hub: Optional[HubPlan] = None):
    """``(y [N, F], mean, rstd)`` of GraphNorm (``mode='channel'``: statistics per graph and column,
    ``mean`` / ``rstd [B, F]``) or of LayerNorm over whole graphs (``mode='graph'``: ``[B]``) for
    the graphs ``ptr [B + 1]`` of the rows of ``x``, which may be a column block of a wider tensor;
    ``std_eps``: divide by ``sqrt(var) + eps``.  ``hub``: :func:`graph_norm_plan` of ``ptr``."""
    _require_device(ptr, x, weight, bias, mean_scale)
    lib = _lib.load()
    if x.dim() != 2:
        raise ValueError("'x' must be two-dimensional")
    N, F = x.shape
    x = _strided_rows(x, 'x', F)
    weight, bias = _norm_param(weight, F, 'weight'), _norm_param(bias, F, 'bias')
    mean_scale = _norm_param(mean_scale, F, 'mean_scale')
    m = _norm_mode(mode, mean_scale, std_eps)
    B = ptr.numel() - 1
    dev = x.device
    y = torch.empty(N, F, dtype=torch.float32, device=dev)
    stats = (B, F) if mode == 'channel' else (B, )
    if B <= 0 or F == 0 or N == 0:   # no row anywhere: nothing to launch
        return y, x.new_zeros(stats), x.new_zeros(stats)
    mean = torch.empty(stats, dtype=torch.float32, device=dev)
    rstd = torch.empty(stats, dtype=torch.float32, device=dev)
    g = _norm_handle(ptr, hub)
    ws_bytes = graph_norm_workspace_bytes(g.n_chunks, g.n_hub, F, False)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    with _timed({'kind': 'graph_norm', 'op': 'forward', 'mode': mode, 'B': B, 'N': N, 'F': F,
                 'ld': _ld(x), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, x):
        check(lib.pygamd_graph_norm_forward(
            ctypes.byref(g), m, _p(x), _ld(x), N, F, _p(weight), _p(bias), _p(mean_scale),
            float(eps), int(bool(std_eps)), _p(y), F, _p(mean), _p(rstd), _p(ws), ws_bytes,
            _stream(x)), 'graph_norm_forward')
    return y, mean, rstd


def graph_norm_backward(ptr: Tensor, x: Tensor, grad_y: Tensor, mean: Tensor, rstd: Tensor,
                        weight: Optional[Tensor], mean_scale: Optional[Tensor], eps: float,
                        mode: str, *, std_eps: bool = False, hub: Optional[HubPlan] = None,
                        want_weight: bool = False, want_bias: bool = False,
                        want_mean_scale: bool = False):
    """``(grad_x [N, F], grad_weight, grad_bias, grad_mean_scale)`` from the forward's inputs and
    its saved ``mean`` and ``rstd``; a parameter gradient that is not wanted is None."""
    _require_device(ptr, x, grad_y, mean, rstd, weight, mean_scale)
    lib = _lib.load()
    if x.dim() != 2:
        raise ValueError("'x' must be two-dimensional")
    N, F = x.shape
    x, grad_y = _strided_rows(x, 'x', F), _strided_rows(grad_y, 'grad_y', F)
    if grad_y.size(0) != N:
        raise ValueError(f"'grad_y' needs the {N} rows of 'x'")
    weight, mean_scale = _norm_param(weight, F, 'weight'), _norm_param(mean_scale, F, 'mean_scale')
    m = _norm_mode(mode, mean_scale, std_eps)
    if want_mean_scale and mode != 'channel':
        raise ValueError("'grad_mean_scale' belongs to mode='channel'")
    B = ptr.numel() - 1
    stats = (B, F) if mode == 'channel' else (B, )
    for t, name in ((mean, 'mean'), (rstd, 'rstd')):
        if t.dtype != torch.float32 or tuple(t.shape) != stats or not t.is_contiguous():
            raise ValueError(f"'{name}' must be the forward's contiguous float32 {stats} tensor")
    dev = x.device
    grad_x = torch.empty(N, F, dtype=torch.float32, device=dev)
    nothing = B <= 0 or F == 0 or N == 0
    alloc = torch.zeros if nothing else torch.empty
    g_w = alloc(F, dtype=torch.float32, device=dev) if want_weight else None
    g_b = alloc(F, dtype=torch.float32, device=dev) if want_bias else None
    g_ms = alloc(F, dtype=torch.float32, device=dev) if want_mean_scale else None
    if nothing:
        return grad_x, g_w, g_b, g_ms
    g = _norm_handle(ptr, hub)
    ws_bytes = graph_norm_workspace_bytes(g.n_chunks, g.n_hub, F, True)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with _timed({'kind': 'graph_norm', 'op': 'backward', 'mode': mode, 'B': B, 'N': N, 'F': F,
                 'ld': _ld(x), 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, x):
        check(lib.pygamd_graph_norm_backward(
            ctypes.byref(g), m, _p(x), _ld(x), _p(grad_y), _ld(grad_y), N, F, _p(weight),
            _p(mean_scale), float(eps), int(bool(std_eps)), _p(mean), _p(rstd), _p(grad_x), F,
            _p(g_w), _p(g_b), _p(g_ms), _p(ws), ws_bytes, _stream(x)), 'graph_norm_backward')
    return grad_x, g_w, g_b, g_ms


# ---- one propagation step with its combination as the epilogue (csrc/hop.hip) ----------------------
def _hop_plane(t: Optional[Tensor], name: str, n_rows: int, F: int) -> Optional[Tensor]:
    if t is None:
        return None
    t = _strided_rows(t, name, F)
    if t.size(0) < n_rows:
        raise ValueError(f"'{name}' needs at least {n_rows} rows (got {t.size(0)})")
    return t


def hop(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], w: Optional[Tensor], x: Tensor,
        a: float = 1.0, *, y: Optional[Tensor] = None, b: float = 0.0,
        z: Optional[Tensor] = None, c: float = 0.0, out: Optional[Tensor] = None,
        want_out: bool = True, sum: Optional[Tensor] = None, d: float = 1.0,
        sum_init: bool = False, hub: Optional[HubPlan] = None) -> Optional[Tensor]:
    """``out [n_rows, F] = a * sum_k w[edge_id[k]] x[col[k]]  (+ b y)  (+ c z)`` over the rows of
    the handle and, with ``sum``, ``sum = (0 if sum_init else sum) + d * out`` in the same launch.
    ``w`` (one value per edge, in the caller's edge order through ``edge_id``; None: 1), ``y``,
    ``z`` may be None; every plane may be a column block of a wider tensor (its row stride is
    passed) and is read or written in place.  ``out`` may be given (it may be ``y`` or ``z``, not
    ``x`` or ``sum``); ``want_out=False`` with ``sum`` writes the sum alone and returns None."""
    _require_device(rowptr, col, edge_id, w, x, y, z, out, sum)
    lib = _lib.load()
    if x.dim() != 2:
        raise ValueError("'x' must be two-dimensional")
    F = x.size(1)
    if F < 1:
        raise ValueError("'x' needs at least one column")
    x = _strided_rows(x, 'x', F)
    n_rows = rowptr.numel() - 1
    y, z = _hop_plane(y, 'y', n_rows, F), _hop_plane(z, 'z', n_rows, F)
    if w is not None:
        if w.dtype != torch.float32 or w.dim() != 1:
            raise ValueError(f"'w' must be a one-dimensional float32 tensor (got {w.dtype} "
                             f"{tuple(w.shape)})")
        if edge_id is None and w.numel() != col.numel():
            raise ValueError("'w' needs one value per slot")
        w = w.contiguous()
    edge_id = _edge_id(edge_id, rowptr, col) if w is not None else None
    for name, t in (('out', out), ('sum', sum)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.size(1) != F
                              or t.size(0) < n_rows or t.stride(1) != 1 or t.stride(0) < F):
            raise ValueError(f"'{name}' must be a float32 [>= {n_rows}, {F}] tensor with unit "
                             f"column stride")
    if not want_out and sum is None:
        raise ValueError("nothing to compute: neither 'out' nor 'sum' is wanted")
    if out is None and want_out:
        out = torch.empty(n_rows, F, dtype=torch.float32, device=x.device)
    if not want_out:
        out = None
    if n_rows == 0:
        return out
    if col.numel() == 0:  # no slots: every row is its epilogue; the launch reads no slot
        col, w, edge_id = rowptr.new_zeros(1), None, None
    g = _csr(rowptr, col, n_rows, hub)
    args = _lib.HopArgs(
        w=_p(w), x=_p(x), ldx=_ld(x), n_src=x.size(0), F=F, a=float(a),
        y=_p(y), ldy=0 if y is None else _ld(y), b=float(b),
        z=_p(z), ldz=0 if z is None else _ld(z), c=float(c),
        out=_p(out), ldo=0 if out is None else _ld(out),
        sum=_p(sum), lds=0 if sum is None else _ld(sum), d=float(d), sum_init=int(bool(sum_init)))
    ws, ws_bytes = _workspace(lib.pygamd_hop_workspace_size, (g.n_chunks, F), x.device,
                              g.n_chunks > 0)
    with _timed({'kind': 'hop', 'n_rows': n_rows, 'E': col.numel(), 'F': F, 'ld': _ld(x),
                 'w': w is not None, 'y': y is not None, 'z': z is not None,
                 'sum': sum is not None, 'n_hub': g.n_hub, 'n_chunks': g.n_chunks}, x):
        check(lib.pygamd_hop(ctypes.byref(g), _p(edge_id), ctypes.byref(args), _p(ws), ws_bytes,
                             _stream(x)), 'hop')
    return out


# ---- dense feature transform (fp32 MFMA GEMM, csrc/gemm.hip) -------------------------------------
def _nt_workspace(lib, M: int, n_out: int, k_red: int, device):
    """Partial-tile slabs of a launch split over its reduction (few row tiles: sampled blocks,
    Cora-sized inputs); ``(None, 0)`` when the rows alone fill the chip."""
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_linear_nt_workspace_bytes(M, n_out, k_red, ctypes.byref(nbytes)))
    if nbytes.value == 0:
        return None, 0
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device), nbytes.value


def linear_forward(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, relu: bool = False,
                   out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """``act(x @ w.T + bias)`` for row-strided fp32 ``x [M, K]``, ``w [N, K]``; ``out`` may be a
    row-strided view (e.g. one half of an ``[agg | x]`` buffer)."""
    _require_device(x, w, bias, out)
    C = _compiled.ops()
    if C is not None and _plain(x, w) and x.size(1) == w.size(1) \
            and (out is None or (out.dtype == torch.float32 and out.shape == (x.size(0), w.size(0))
                                 and (w.size(0) <= 1 or out.stride(1) == 1))):
        if out is None:
            out = torch.empty(x.size(0), w.size(0), dtype=torch.float32, device=x.device)
        with _timed({'kind': 'gemm', 'op': 'forward', 'M': x.size(0), 'N': w.size(0),
                     'K': x.size(1)}, x):
            C.linear_forward(x, w, bias, relu, out, accumulate)
        return out
    lib = _lib.load()
    x2, w2 = _f32_rows(x, 'x'), _f32_rows(w, 'weight')
    M, K = x2.shape
    N = w2.size(0)
    if w2.size(1) != K:
        raise ValueError(f"'x' has {K} columns but 'weight' expects {w2.size(1)}")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    elif out.shape != (M, N) or out.dtype != torch.float32 or (N > 1 and out.stride(1) != 1):
        raise ValueError("'out' must be a float32 [M, N] tensor with unit inner stride")
    if bias is not None:
        bias = bias.contiguous()
    ws, ws_bytes = _nt_workspace(lib, M, N, K, x.device)
    with _timed({'kind': 'gemm', 'op': 'forward', 'M': M, 'N': N, 'K': K}, x):
        check(lib.pygamd_linear_forward(_p(x2), _ld(x2), _p(w2), _ld(w2), _p(bias), M, K, N,
                                        int(relu), int(accumulate), _p(out), _ld(out), _p(ws),
                                        ws_bytes, _stream(x)), 'linear_forward')
    return out


def relu_bits_like(n_rows: int, width: int, device) -> Tensor:
    """Storage for a ReLU mask with one bit per element (``pygamd_spmm_args.relu_bits``): int32
    ``[ceil(n_rows / 32), ceil(width / 32), 32]`` — tiles of 32 rows x 32 columns, word
    ``[r >> 5, c >> 5, r & 31]`` holds the 32 columns of row ``r`` in its bits ``c & 31``."""
    return torch.empty((n_rows + 31) // 32, (width + 31) // 32, 32, dtype=torch.int32,
                       device=device)


def pack_relu_bits(act: Tensor) -> Tensor:
    """``act > 0`` in the layout of :func:`relu_bits_like` (host-side helper for tests / callers
    that did not get the bits from ``sage_layer_forward``)."""
    n, f = act.shape
    rt, w = (n + 31) // 32, (f + 31) // 32
    pos = torch.zeros(rt * 32, w * 32, dtype=torch.int64, device=act.device)
    pos[:n, :f] = (act > 0).to(torch.int64)
    weights = (1 << torch.arange(32, dtype=torch.int64, device=act.device))
    words = (pos.view(rt, 32, w, 32) * weights).sum(-1)          # [tile, row in tile, block]
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)  # two's complement int32
    return words.permute(0, 2, 1).contiguous().to(torch.int32)


def _check_bits(bits: Optional[Tensor], n_rows: int, width: int):
    if bits is None:
        return
    if (bits.dtype != torch.int32 or bits.dim() != 3 or bits.size(0) < (n_rows + 31) // 32
            or bits.size(1) < (width + 31) // 32 or bits.size(2) != 32
            or not bits.is_contiguous()):
        raise ValueError(f"'relu_bits' must be a contiguous int32 [>= {(n_rows + 31) // 32}, >= "
                         f"{(width + 31) // 32}, 32] (see relu_bits_like), got {bits.dtype} "
                         f"{tuple(bits.shape)}")


def sage_layer_forward_supported(F: int, Fo: int, reduce: str) -> bool:
    return bool(_lib.load().pygamd_sage_layer_forward_supported(F, Fo, REDUCE_IDS[reduce]))


# schedule of the one-kernel layer: 0 / None = the production entry point (arithmetic per
# set_gemm_mode); 1..6 = include/pyg_amd_lab.h (1 = production fp32 schedule with probe bits,
# 2 = streamed gather phase, 3 / 4 = persistent producer / consumer waves with 4 / 8 transform
# waves, 5 / 6 = the production split / fp32 kernels whatever the mode); the env switch exists for
# A/B timing on the device
SAGE_FUSED_VARIANT = int(os.environ.get('PYGAMD_FUSED_VARIANT', '0'))
SAGE_FUSED_PROBE = 0  # scripts/fused_probe.py: skip the gather (1) / MFMA (2) loop of the kernel
# `save_agg` of sage_layer_forward: `agg` already holds the aggregated rows (PYGAMD_AGG_GIVEN)
AGG_GIVEN = _lib.AGG_GIVEN


def sage_layer_forward(rowptr: Tensor, col: Tensor, x_gather: Tensor, x_root: Tensor, w: Tensor,
                       bias: Optional[Tensor], reduce: str, relu: bool, agg: Tensor, out: Tensor,
                       hub=None, save_agg=True, relu_bits: Optional[Tensor] = None,
                       mask_bits: Optional[Tensor] = None, row_scale: Optional[Tensor] = None,
                       out_scaled: Optional[Tensor] = None, variant: Optional[int] = None,
                       gather_width: Optional[int] = None,
                       compressed_out: Optional[Tensor] = None,
                       rowend: Optional[Tensor] = None) -> Tensor:
    """``out = act([aggr(x_gather) | x_root] @ w.T + bias)`` in ONE kernel (csrc/sage_fused.hip);
    ``agg`` ([n_rows, F] view, may be a half of a wider buffer) receives the aggregated rows when
    ``save_agg`` (hub rows always).  ``save_agg=AGG_GIVEN``: ``agg`` already holds them (left there
    by a ``save_agg=True`` launch on the same graph and ``x_gather``) and is read instead of the
    gather — same results bit for bit, no index or source row is touched.  ``relu_bits`` (from :func:`relu_bits_like`, needs
    ``relu``) receives ``out > 0`` as one bit per element (see :func:`relu_bits_like`).
    ``mask_bits`` (same layout): ``out`` is zeroed where its bit is clear — with the transposed
    graph, the degree-scaled gradient rows as ``x_gather``, the unscaled ones as ``x_root`` and
    ``w = [W_l^T | W_r^T]`` the launch is the layer's INPUT GRADIENT (dgrad GEMM + transposed
    aggregation + ReLU backward in one pass).  ``out_scaled`` receives ``out * row_scale[:, None]``
    as a second output (what the next such launch gathers).  ``gather_width=F``: ``x_gather`` is
    an int32 block of compressed rows (:func:`rows_compress`) of ``F`` columns; ``compressed_out``
    (int32 ``[n_rows, compressed_pitch(Fo)]``) receives ``out`` once more in that layout."""
    _require_device(rowptr, col, x_gather, x_root, w, bias, agg, out, relu_bits, mask_bits,
                    row_scale, out_scaled, compressed_out)
    variant = SAGE_FUSED_VARIANT if variant is None else variant
    given = not isinstance(save_agg, bool) and int(save_agg) == AGG_GIVEN
    save_agg = AGG_GIVEN if given else int(bool(save_agg))
    if given:
        if gather_width is not None:
            raise ValueError("'save_agg=AGG_GIVEN' reads dense aggregated rows: not with a "
                             "compressed 'x_gather'")
        hub = None  # (no hub pre-pass: the rows of `agg` are final)
    lab = bool(variant or SAGE_FUSED_PROBE)  # a laboratory schedule / probe: libpyg_amd_lab.so
    C = None if lab else _compiled.ops()
    if (C is not None and gather_width is None and compressed_out is None and rowend is None
            and _plain(x_gather, x_root, w, agg, out, out_scaled)):
        n_rows, F, Fo = rowptr.numel() - 1, x_gather.size(1), w.size(0)
        ok = (x_root.shape == (n_rows, F) and w.size(1) == 2 * F and agg.shape == (n_rows, F)
              and out.shape == (n_rows, Fo)
              and (out_scaled is None or (row_scale is not None and row_scale.numel() == n_rows
                                          and row_scale.dtype == torch.float32
                                          and out_scaled.shape == (n_rows, Fo)
                                          and (Fo <= 1 or out_scaled.stride(1) == 1))))
        if ok:
            _check_bits(relu_bits, n_rows, Fo)
            _check_bits(mask_bits, n_rows, Fo)
            hub = _hub6(hub)
            with _timed({'n_rows': n_rows, 'n_src': x_gather.size(0),
                         'nnz': 0 if given else col.numel(), 'F': F,
                         'reduce': reduce, 'idx_bytes': rowptr.element_size(), 'weighted': False,
                         'src_scale': False, 'accumulate': False, 'n_hub': hub.n_hub,
                         'fused_gemm': {'Fo': Fo, 'K': 2 * F, 'save_agg': bool(save_agg),
                                        'backward': mask_bits is not None,
                                        'scaled_copy': out_scaled is not None}}, x_gather):
                if given:  # (its own operator: `agg` is an input there, see torch_binding.cpp)
                    C.sage_layer_given(rowptr, x_root, w, bias, REDUCE_IDS[reduce], relu, agg,
                                       out, relu_bits, mask_bits, row_scale, out_scaled)
                else:
                    C.sage_layer_fused(
                        rowptr, col, x_gather, x_root, w, bias, REDUCE_IDS[reduce], relu, agg,
                        out, *hub, save_agg, relu_bits, mask_bits, row_scale, out_scaled)
            return out
    lib = _lib.load_lab() if lab else _lib.load()
    xr, w2 = _f32_rows(x_root, 'x_root'), _f32_rows(w, 'weight')
    if gather_width is None:
        xg = _f32_rows(x_gather, 'x')
        F = xg.size(1)
    else:
        _check_compressed(x_gather, gather_width, 'x_gather')
        xg, F = x_gather, gather_width
    n_rows, Fo = rowptr.numel() - 1, w2.size(0)
    if rowend is not None:  # rows own fixed slot blocks [rowptr[r], rowend[r]) (sampled batches)
        _require_device(rowend)
        n_rows = xr.size(0)
        if rowend.dtype != rowptr.dtype or not rowend.is_contiguous() \
                or rowend.numel() < n_rows or rowptr.numel() < n_rows:
            raise ValueError("'rowend' needs the dtype of 'rowptr' and one entry per row")
    if xr.shape != (n_rows, F) or w2.size(1) != 2 * F or agg.shape != (n_rows, F) \
            or out.shape != (n_rows, Fo):
        raise ValueError('shape mismatch in sage_layer_forward')
    a = SpmmArgs()
    a.rowptr, a.col = rowptr.data_ptr(), col.data_ptr()
    if rowend is not None:
        a.rowend = rowend.data_ptr()
    a.x, a.out = xg.data_ptr(), agg.data_ptr()
    a.n_rows, a.n_src, a.F = n_rows, xg.size(0), F
    a.ldx, a.ldo = _ld(xg), _ld(agg)
    a.idx_dtype, a.reduce = _idx_dtype(rowptr), REDUCE_IDS[reduce]
    a.w_heads, a.head_dim = 1, F
    if gather_width is not None:
        a.x_format = _lib.X_COMPRESSED
    _hub_args(a, hub)
    if bias is not None:
        bias = bias.contiguous()
    _check_bits(relu_bits, n_rows, Fo)
    _check_bits(mask_bits, n_rows, Fo)
    f = _lib.SageFusedArgs()
    f.x_root, f.ld_root = xr.data_ptr(), _ld(xr)
    f.w, f.ldw = w2.data_ptr(), _ld(w2)
    f.bias = 0 if bias is None else bias.data_ptr()
    f.Fo, f.relu, f.save_agg = Fo, int(relu), save_agg
    f.y, f.ldy = out.data_ptr(), _ld(out)
    if relu_bits is not None:
        f.relu_bits_out, f.ld_bits_out = relu_bits.data_ptr(), relu_bits.size(1)
    if mask_bits is not None:
        f.mask_bits, f.ld_mask_bits = mask_bits.data_ptr(), mask_bits.size(1)
    if out_scaled is not None:
        if row_scale is None or row_scale.numel() != n_rows or row_scale.dtype != torch.float32:
            raise ValueError("'out_scaled' needs a float32 'row_scale' with one entry per row")
        if out_scaled.shape != (n_rows, Fo) or out_scaled.dtype != torch.float32 \
                or (Fo > 1 and out_scaled.stride(1) != 1):
            raise ValueError("'out_scaled' must be a float32 [n_rows, Fo] tensor with unit inner "
                             "stride")
        row_scale = row_scale.contiguous()
        f.row_scale = row_scale.data_ptr()
        f.y_scaled, f.ldy_scaled = out_scaled.data_ptr(), _ld(out_scaled)
    if compressed_out is not None:
        _check_compressed(compressed_out, Fo, 'compressed_out')
        if compressed_out.size(0) != n_rows or Fo % 32 != 0:
            raise ValueError("'compressed_out' needs one row per output row and Fo % 32 == 0")
        f.compressed_out, f.ld_compressed = compressed_out.data_ptr(), _ld(compressed_out)
    sink = timing_sink
    if sink is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(xg.device))
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_sage_layer_fused_workspace_bytes(ctypes.byref(a), ctypes.byref(f),
                                                      ctypes.byref(nbytes)))
    ws_bytes = nbytes.value
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xg.device) if ws_bytes else None
    if lab:
        check(lib.pygamd_lab_sage_layer_fused(ctypes.byref(a), ctypes.byref(f), variant or 1,
                                              SAGE_FUSED_PROBE, _p(ws), ws_bytes, _stream(xg)),
              'sage_layer_forward (lab schedule)')
    else:
        check(lib.pygamd_sage_layer_fused(ctypes.byref(a), ctypes.byref(f), _p(ws), ws_bytes,
                                          _stream(xg)), 'sage_layer_forward')
    if sink is not None:
        ev1.record(torch.cuda.current_stream(xg.device))
        sink.append(({'n_rows': n_rows, 'n_src': xg.size(0),
                      'nnz': 0 if given else col.numel(), 'F': F,
                      'reduce': reduce, 'idx_bytes': rowptr.element_size(), 'weighted': False,
                      'src_scale': False, 'accumulate': False, 'n_hub': a.n_hub,
                      'compressed_src': gather_width is not None,
                      'fused_gemm': {'Fo': Fo, 'K': 2 * F, 'save_agg': bool(save_agg),
                                     'backward': mask_bits is not None,
                                     'scaled_copy': out_scaled is not None,
                                     'compressed_out': compressed_out is not None}}, ev0, ev1))
    return out


def cross_entropy_rows(logits: Tensor, target: Tensor, index: Optional[Tensor] = None):
    """``(loss, grad_rows)`` of ``F.cross_entropy(logits[index], target[index])`` (``index`` None: all
    rows; mean reduction) from ONE pass over the selected rows (``pygamd_cross_entropy_step``):
    ``loss`` a float32 scalar, ``grad_rows`` ``[B, C]`` = ``d loss / d logits[index]``.  ``target``
    holds one int64 label per row of ``logits``.  A label outside ``[0, C)`` / an index outside the
    rows is flagged (``PYGAMD_CHECK_INDEX``) and contributes neither loss nor gradient."""
    _require_device(logits, target, index)
    x = _f32_rows(logits, 'logits')
    N, C = x.shape
    if target.dtype != torch.int64 or target.dim() != 1 or target.numel() != N \
            or not target.is_contiguous():
        raise ValueError(f"'target' must hold one contiguous int64 label per row of 'logits' "
                         f"({N}), got {target.dtype} {tuple(target.shape)}")
    if index is not None and (index.dtype != torch.int64 or index.dim() != 1
                              or not index.is_contiguous()):
        raise ValueError("'index' must be a contiguous 1-D int64 tensor")
    B = N if index is None else index.numel()
    if B == 0 or C == 0:
        raise ValueError('cross_entropy_rows needs at least one row and one class')
    lib = _lib.load()
    grad = torch.empty(B, C, dtype=torch.float32, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_cross_entropy_step_workspace_bytes(B, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
    ring, slot, err = _index_flag(x.device, True)
    check(lib.pygamd_cross_entropy_step(_p(x), _ld(x), _p(index), N, B, C, _p(target), _p(index),
                                        _p(grad), C, _p(loss), _p(ws), nbytes.value, _p(err),
                                        None, _stream(x)), 'cross_entropy_rows')
    _index_flag_done(ring, slot, err, "cross_entropy: a target outside [0, C) (or an 'index' "
                     "entry outside the rows of the logits)", C, target)
    return loss, grad


def set_gemm_mode(mode: str) -> str:
    """Arithmetic of the dense transform kernels (``pygamd_set_gemm_mode``): ``'fp32'`` (default:
    the fp32 matrix instruction, bitwise an fmaf chain) or ``'split'`` (operands as three bf16
    terms each, six bf16 matrix products with fp32 accumulation: fp32-level accuracy, ~2.5 x the
    matrix rate).  Returns the previous mode."""
    lib = _lib.load()
    if mode not in _lib.GEMM_MODES:
        raise ValueError(f"mode must be one of {sorted(_lib.GEMM_MODES)}, got '{mode}'")
    prev = get_gemm_mode()
    for each in _lib.loaded():  # (the laboratory build keeps its own copy of the switch)
        check(each.pygamd_set_gemm_mode(_lib.GEMM_MODES[mode]), 'set_gemm_mode')
    return prev


def lab_set_wgrad_variant(variant: int) -> None:
    """LAB (include/pyg_amd_lab.h, libpyg_amd_lab.so): 0 = production split weight gradient
    (operands split once on their way into LDS), 1 = round 3's in-register schedule, further
    values = timing probes.  While a variant is selected EVERY call of this module goes to the
    laboratory library (a superset build of the product library) through ctypes; 0 switches back
    to the product library.  Tests and probes only."""
    check(_lib.load_lab().pygamd_lab_set_wgrad_variant(int(variant)), 'lab_set_wgrad_variant')
    _lib.use_lab(int(variant) != 0)


def get_gemm_mode() -> str:
    code = _lib.load().pygamd_get_gemm_mode()
    return next(k for k, v in _lib.GEMM_MODES.items() if v == code)


def linear_dgrad(g: Tensor, w_t: Tensor, row_scale: Optional[Tensor] = None, n_scaled: int = 0,
                 out: Optional[Tensor] = None, accumulate: bool = False,
                 relu_mask: Optional[Tensor] = None, relu_bits: Optional[Tensor] = None,
                 out_scaled: Optional[Tensor] = None) -> Tensor:
    """``g [M, N] @ w [N, K]`` with the weight handed over transposed (``w_t [K, N]``); columns
    ``[0, n_scaled)`` of the result are multiplied by ``row_scale[row]``; where ``relu_mask [M, K]``
    (a ReLU output) is not positive the result is 0 (that ReLU's backward as the epilogue);
    ``relu_bits`` is the same mask as one bit per element (:func:`relu_bits_like`).
    ``out_scaled [M, K]`` receives ``result * row_scale[:, None]`` (all columns) as a second
    output of the same pass."""
    _require_device(g, w_t, row_scale, out, relu_mask, relu_bits, out_scaled)
    if relu_mask is not None and relu_bits is not None:
        raise ValueError("pass at most one of 'relu_mask' / 'relu_bits'")
    C = _compiled.ops()
    if C is not None and _plain(g, w_t, relu_mask, out, out_scaled) \
            and g.size(1) == w_t.size(1):
        M, K = g.size(0), w_t.size(0)
        ok = ((out is None or (out.shape == (M, K) and (K <= 1 or out.stride(1) == 1)))
              and (relu_mask is None or tuple(relu_mask.shape) == (M, K))
              and (out_scaled is None or (row_scale is not None and not accumulate
                                          and out_scaled.shape == (M, K)
                                          and (K <= 1 or out_scaled.stride(1) == 1))))
        if ok:
            _check_bits(relu_bits, M, K)
            if out is None:
                out = torch.empty(M, K, dtype=torch.float32, device=g.device)
            with _timed({'kind': 'gemm', 'op': 'dgrad', 'M': M, 'N': K, 'K': g.size(1)}, g):
                C.linear_dgrad(g, w_t, row_scale, n_scaled, out, accumulate, relu_mask,
                               relu_bits, out_scaled)
            return out
    lib = _lib.load()
    g2, w2 = _f32_rows(g, 'grad'), _f32_rows(w_t, 'weight_t')
    M, N = g2.shape
    K = w2.size(0)
    if w2.size(1) != N:
        raise ValueError(f"'grad' has {N} columns but 'weight_t' expects {w2.size(1)}")
    if out is None:
        out = torch.empty(M, K, dtype=torch.float32, device=g.device)
    if row_scale is not None:
        row_scale = row_scale.contiguous()
    if out_scaled is not None:
        if row_scale is None or accumulate:
            raise ValueError("'out_scaled' needs 'row_scale' and no 'accumulate'")
        if out_scaled.shape != (M, K) or out_scaled.dtype != torch.float32 \
                or (K > 1 and out_scaled.stride(1) != 1):
            raise ValueError("'out_scaled' must be a float32 [M, K] tensor with unit inner stride")
    m2 = None
    _check_bits(relu_bits, M, K)
    if relu_mask is not None:
        m2 = _f32_rows(relu_mask, 'relu_mask')
        if tuple(m2.shape) != (M, K):
            raise ValueError(f"'relu_mask' must be [{M}, {K}], got {tuple(m2.shape)}")
    ws, ws_bytes = _nt_workspace(lib, M, K, N, g.device)
    with _timed({'kind': 'gemm', 'op': 'dgrad', 'M': M, 'N': K, 'K': N}, g):
        check(lib.pygamd_linear_dgrad2(_p(g2), _ld(g2), _p(w2), _ld(w2), _p(row_scale),
                                       n_scaled if row_scale is not None else 0, M, N, K,
                                       int(accumulate), _p(m2), _ld(m2) if m2 is not None else 0,
                                       _p(relu_bits),
                                       relu_bits.size(1) if relu_bits is not None else 0,
                                       _p(out), _ld(out), _p(out_scaled),
                                       _ld(out_scaled) if out_scaled is not None else 0,
                                       _p(ws), ws_bytes, _stream(g)), 'linear_dgrad')
    return out


def linear_wgrad(g: Tensor, x: Tensor, out: Optional[Tensor] = None,
                 accumulate: bool = False, wgs_per_cu: int = 0, bias_grad: bool = False,
                 x2: Optional[Tensor] = None, bias_out: Optional[Tensor] = None):
    """``g [M, N].T @ x [M, K]`` -> ``[N, K]`` (deterministic split reduction over M).
    ``wgs_per_cu=1`` halves the launch's footprint (for running under a bandwidth-bound kernel
    on another stream).  ``bias_grad=True`` also returns ``g.sum(0)`` — taken from the same pass
    over ``g`` — as ``(grad_w, grad_b)``.  ``x2`` (``[M, K2]``): the gradient against
    ``[x | x2]`` -> ``[N, K + K2]`` without concatenating the two.  ``bias_out`` (contiguous
    float32 ``[N]``, with ``bias_grad``): where the bias gradient is written (e.g. its slot of a
    flat gradient buffer) instead of a fresh tensor."""
    _require_device(g, x, out, x2, bias_out)
    if bias_out is not None and (not bias_grad or bias_out.dtype != torch.float32
                                 or bias_out.shape != (g.size(1), )
                                 or not bias_out.is_contiguous()):
        raise ValueError("'bias_out' needs bias_grad=True and a contiguous float32 [N] tensor")
    C = _compiled.ops()
    if C is not None and _plain(g, x, x2, out) and x.size(0) == g.size(0) \
            and (x2 is None or (x2.size(0) == g.size(0) and x.size(1) > 0 and x2.size(1) > 0)):
        N, K = g.size(1), x.size(1) + (0 if x2 is None else x2.size(1))
        if K > 0 and (out is None or (out.shape == (N, K) and (K <= 1 or out.stride(1) == 1))):
            if out is None:
                out = torch.empty(N, K, dtype=torch.float32, device=g.device)
            gb = None
            if bias_grad:
                gb = bias_out if bias_out is not None else \
                    torch.empty(N, dtype=torch.float32, device=g.device)
            with _timed({'kind': 'gemm', 'op': 'wgrad', 'M': g.size(0), 'N': N, 'K': K,
                         'x2': x2 is not None}, g):
                C.linear_wgrad(g, x, out, accumulate, wgs_per_cu, gb, x2)
            return (out, gb) if bias_grad else out
    lib = _lib.load()
    second = None if x2 is None else _f32_rows(x2, 'x2')
    g2, first = _f32_rows(g, 'grad'), _f32_rows(x, 'x')
    M, N = g2.shape
    K1 = first.size(1)
    K2 = 0 if second is None else second.size(1)
    K = K1 + K2
    if first.size(0) != M or (second is not None and second.size(0) != M):
        raise ValueError(f"'grad' has {M} rows but 'x' has {first.size(0)}"
                         + ('' if second is None else f" and 'x2' {second.size(0)}"))
    if second is not None and (K1 == 0 or K2 == 0):
        raise ValueError("both operands of a two-operand weight gradient need columns")
    if out is None:
        out = torch.empty(N, K, dtype=torch.float32, device=g.device)
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_linear_wgrad_workspace_bytes(M, N, K, ctypes.byref(nbytes)))
    ws = torch.empty(max(nbytes.value, 4), dtype=torch.uint8, device=g.device)
    gb = None
    if bias_grad:
        if K == 0:  # no weight tile passes over g
            cs = colsum(g2)
            return out, (cs if bias_out is None else bias_out.copy_(cs))
        gb = bias_out if bias_out is not None else \
            torch.empty(N, dtype=torch.float32, device=g.device)
    with _timed({'kind': 'gemm', 'op': 'wgrad', 'M': M, 'N': N, 'K': K,
                 'x2': second is not None}, g):
        check(lib.pygamd_linear_wgrad2(_p(g2), _ld(g2), _p(first), _ld(first), K1, _p(second),
                                       _ld(second) if second is not None else 0, K2, M, N,
                                       int(accumulate), int(wgs_per_cu), _p(out), _ld(out),
                                       _p(gb), _p(ws), nbytes.value, _stream(g)), 'linear_wgrad')
    return (out, gb) if bias_grad else out


# ---- segment_matmul (grouped GEMM, fp32 MFMA) ---------------------------------------------------
_segmm_plans = {}


WGRAD_CHUNK_ROWS = 2048


def segmm_plan(ptr_host: tuple, device, blocks: int = 1):
    """(tiles int32 [T,3], T, wgrad chunks int32 [C,3], C) on `device` for a host pointer tuple;
    cached.  Tiles cover every non-empty segment in 64-row pieces, chunks in 2048-row pieces.
    With ``blocks`` > 1 every piece is listed once per column block, as group
    ``segment * blocks + b`` (the block-diagonal layout of ``pygamd_segment_matmul``)."""
    key = (ptr_host, str(device), blocks)
    hit = _segmm_plans.get(key)
    if hit is not None:
        return hit
    tm = _lib.load().pygamd_segment_matmul_tile_rows()

    def pieces(step):
        out = []
        for g in range(len(ptr_host) - 1):
            a, b = ptr_host[g], ptr_host[g + 1]
            for r in range(a, b, step):
                for blk in range(blocks):
                    out.append((g * blocks + blk, r, min(step, b - r)))
        return out

    tiles, chunks = pieces(tm), pieces(WGRAD_CHUNK_ROWS)
    t = torch.tensor(tiles, dtype=torch.int32).reshape(-1, 3).to(device)
    c = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 3).to(device)
    if len(_segmm_plans) > 32:
        _segmm_plans.pop(next(iter(_segmm_plans)))
    _segmm_plans[key] = (t, len(tiles), c, len(chunks))
    return _segmm_plans[key]


def _row_index(rows: Optional[Tensor], name: str) -> Optional[Tensor]:
    if rows is None:
        return None
    if rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"'{name}' must be a one-dimensional int32 / int64 tensor")
    return rows.to(torch.int64).contiguous()


def segment_matmul(x: Tensor, w: Tensor, plan, transpose_w: bool = False,
                   blocks: int = 1, x_rows: Optional[Tensor] = None) -> Tensor:
    """out[seg] = x[seg] @ W[g]  (or @ W[g]^T when transpose_w) — W is [G, K, N] contiguous.
    ``blocks`` > 1: x is [S, blocks*K], W is [segments*blocks, K, N], out is [S, blocks*N].
    ``x_rows`` [S]: operand row s is ``x[x_rows[s]]`` (gathered inside the kernel)."""
    _require_device(x, w, x_rows)
    x_rows = _row_index(x_rows, 'x_rows')
    lib = _lib.load()
    tiles, n_tiles = plan[0], plan[1]
    x2 = _f32_rows(x, 'x')
    w = w.contiguous()
    if transpose_w:
        w = w.transpose(1, 2)
    G, K, N = w.shape
    # the bf16 term planes of the weights (split arithmetic, K <= 128: csrc/segmm.hip)
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_segment_matmul_workspace_bytes(G, K, N, ctypes.byref(nbytes)))
    split = nbytes.value > 0 and get_gemm_mode() == 'split'
    if transpose_w and not split:
        # the general kernel streams weight rows with coalesced 128-byte loads: materialise W^T
        # (the split kernel's pre-pass reads the transposed view where it lies)
        w = w.contiguous()
    seg_stride, sk, sn = w.stride()
    if x2.size(1) != blocks * K:
        raise ValueError(f"'inputs' has {x2.size(1)} columns but the weights expect "
                         f"{blocks * K}")
    n_out = x2.size(0) if x_rows is None else x_rows.numel()
    out = torch.empty(n_out, blocks * N, dtype=torch.float32, device=x.device)
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device) if split else None
    check(lib.pygamd_segment_matmul(_p(x2), _ld(x2), _p(x_rows), _p(w), seg_stride, sk, sn, G,
                                    _p(tiles),
                                    n_tiles, K, N, blocks, _p(out), _ld(out), _p(ws),
                                    0 if ws is None else nbytes.value, _stream(x)),
          'segment_matmul')
    return out


def segment_matmul_wgrad(x: Tensor, g: Tensor, plan, n_seg: int, blocks: int = 1,
                         g_rows: Optional[Tensor] = None) -> Tensor:
    """grad_W[g] = x[seg]^T @ grad[seg] -> [G, K, N]  (G = n_seg groups incl. blocks).
    ``g_rows`` [S]: gradient row s is ``g[g_rows[s]]`` (gathered inside the kernel)."""
    _require_device(x, g, g_rows)
    g_rows = _row_index(g_rows, 'g_rows')
    lib = _lib.load()
    x2, g2 = _f32_rows(x, 'x'), _f32_rows(g, 'grad')
    K, N = x2.size(1) // blocks, g2.size(1) // blocks
    gw = torch.empty(n_seg, K, N, dtype=torch.float32, device=x.device)
    check(lib.pygamd_segment_matmul_wgrad(_p(x2), _ld(x2), _p(g2), _ld(g2), _p(g_rows),
                                          _p(plan[2]), plan[3],
                                          n_seg, K, N, blocks, _p(gw), _stream(x)),
          'segment_matmul_wgrad')
    return gw


# ---- neighbour sampling (one hop) ---------------------------------------------------------------
def sample_neighbors(colptr: Tensor, row: Tensor, frontier: Tensor, offsets: Tensor, total: int,
                     max_per_node: int, seed: int, zero_fill: bool = False,
                     replace: bool = False, salt_position: bool = False,
                     seed_dev: Optional[Tensor] = None, weight: Optional[Tensor] = None,
                     window: Optional[Tuple[Tensor, Tensor]] = None):
    """(src_global, dst_pos_in_frontier, csc_slot) for the sampled in-edges of `frontier`.
    ``total`` sizes the outputs; ``zero_fill`` for a static capacity larger than what the hop
    really samples (the tail then holds 0 = a valid node / slot id).  ``replace``: draws with
    replacement (``offsets`` from :func:`sample_counts` with the same flag).  ``salt_position``:
    the draws of a node also depend on its position in ``frontier`` (disjoint sampling: the same
    node in two trees draws independently).  ``seed_dev`` (int64 [1] on the device) is added to
    ``seed`` on the device (a captured graph bumps it between replays).  ``weight`` (fp32 [E] in
    CSC slot order, finite, >= 0): draws in proportion to edge weight
    (``pygamd_sample_neighbors_weighted``).  ``window``: the ``(lo, hi)`` of
    :func:`sample_temporal_window`; the same draws on the slots ``[lo, hi)`` in place of the
    node's column (``pygamd_sample_neighbors_temporal``), so a window that is the whole column
    gives the column's edges bit for bit."""
    _require_device(colptr, row, frontier, offsets, weight, *(window or ()))
    if weight is not None and (weight.dtype != torch.float32 or not weight.is_contiguous()
                               or weight.numel() != row.numel()):
        raise ValueError("'weight' must be a contiguous float32 tensor with one entry per edge")
    if weight is not None and window is not None:
        raise ValueError("weighted draws on a window are not supported")
    lib = _lib.load()
    alloc = torch.zeros if zero_fill else torch.empty
    src = alloc(total, dtype=colptr.dtype, device=colptr.device)
    dstpos = alloc(total, dtype=colptr.dtype, device=colptr.device)
    slot = alloc(total, dtype=colptr.dtype, device=colptr.device)
    # the arguments every draw entry point ends with
    tail = (_p(offsets), max_per_node, seed & 0xFFFFFFFFFFFFFFFF,
            int(replace) | (2 if salt_position else 0), _p(seed_dev), _p(src), _p(dstpos),
            _p(slot), _stream(colptr))
    if total > 0 and weight is not None:
        check(lib.pygamd_sample_neighbors_weighted(
            _p(colptr), _p(row), _idx_dtype(colptr), _p(weight), _p(frontier), frontier.numel(),
            *tail), 'sample_neighbors_weighted')
    elif total > 0 and window is not None:
        check(lib.pygamd_sample_neighbors_temporal(
            _p(row), _idx_dtype(row), _p(frontier), frontier.numel(), _p(window[0]),
            _p(window[1]), *tail), 'sample_neighbors_temporal')
    elif total > 0:
        check(lib.pygamd_sample_neighbors(_p(colptr), _p(row), _idx_dtype(colptr), _p(frontier),
                                          frontier.numel(), *tail), 'sample_neighbors')
    return src, dstpos, slot


def gather_scatter_add(x: Tensor, gather_idx: Tensor, scatter_idx: Tensor, n_out: int,
                       scale: Optional[Tensor] = None, w: Optional[Tensor] = None,
                       out: Optional[Tensor] = None, n_valid: Optional[Tensor] = None) -> Tensor:
    """out[scatter_idx[e]] += scale[gather_idx[e]] * w[e] * x[gather_idx[e]]; ``out`` defaults to
    zeros, or accumulates into the given (row-strided) buffer.  ``n_valid`` (int64 [1], device):
    only that many leading entries of the fixed-capacity edge list are real."""
    _require_device(x, gather_idx, scatter_idx, scale, w, out)
    C = _compiled.ops()
    if C is not None and _plain(x, out) and gather_idx.dtype in (torch.int32, torch.int64) \
            and (out is None or (out.size(1) == x.size(1) and (x.size(1) <= 1 or out.stride(1) == 1))):
        if out is None:
            out = torch.zeros(n_out, x.size(1), dtype=torch.float32, device=x.device)
        C.gather_scatter_add(x, gather_idx, scatter_idx, scale, w, out, n_valid)
        return out
    lib = _lib.load()
    x2 = _f32_rows(x, 'x')
    F = x2.size(1)
    if out is None:
        out = torch.zeros(n_out, F, dtype=torch.float32, device=x.device)
    gi, si = gather_idx.contiguous(), scatter_idx.contiguous()
    if scale is not None:
        scale = scale.contiguous()
    if w is not None:
        w = w.contiguous()
    check(lib.pygamd_gather_scatter_add(_p(x2), _ld(x2), _p(gi), _p(si), _idx_dtype(gi),
                                        _p(scale), _p(w), gi.numel(), _p(n_valid), F, _p(out),
                                        _ld(out), _stream(x)), 'gather_scatter_add')
    return out


# ---- GAT node terms ----------------------------------------------------------------------------
def head_dot_forward(x: Tensor, att_a: Tensor, att_b: Optional[Tensor], H: int, C: int):
    """(a, b) with a[n,h] = <x[n,h,:], att_a[h,:]>; x is [N, H*C]."""
    _require_device(x, att_a, att_b)
    lib = _lib.load()
    x2 = _f32_rows(x, 'x')
    n = x2.size(0)
    att_a = att_a.contiguous()
    out_a = torch.empty(n, H, dtype=torch.float32, device=x.device)
    out_b = None
    if att_b is not None:
        att_b = att_b.contiguous()
        out_b = torch.empty(n, H, dtype=torch.float32, device=x.device)
    check(lib.pygamd_head_dot_forward(_p(x2), _ld(x2), _p(att_a), _p(att_b), n, H, C, _p(out_a),
                                      _p(out_b), _stream(x)), 'head_dot_forward')
    return out_a, out_b


def head_dot_backward(x: Tensor, att_a: Tensor, att_b: Optional[Tensor], grad_a: Tensor,
                      grad_b: Optional[Tensor], H: int, C: int, need_grad_x: bool,
                      accumulate_into: Optional[Tensor] = None):
    """``accumulate_into`` ([n, H*C], unit inner stride): the input gradient is ADDED to it (the
    gradient of the same x through the aggregation) instead of going to a fresh tensor."""
    _require_device(x, att_a, att_b, grad_a, grad_b, accumulate_into)
    lib = _lib.load()
    x2 = _f32_rows(x, 'x')
    n = x2.size(0)
    att_a, grad_a = att_a.contiguous(), grad_a.contiguous()
    g_att_a = torch.empty(H * C, dtype=torch.float32, device=x.device)
    g_att_b = None
    if att_b is not None:
        att_b, grad_b = att_b.contiguous(), grad_b.contiguous()
        g_att_b = torch.empty(H * C, dtype=torch.float32, device=x.device)
    if accumulate_into is not None:
        grad_x = _f32_rows(accumulate_into, 'accumulate_into')
        if grad_x is not accumulate_into or grad_x.shape != (n, H * C):
            raise ValueError("'accumulate_into' must be [n, H * C] float32 with unit inner stride")
    else:
        grad_x = torch.empty(n, H * C, dtype=torch.float32, device=x.device) \
            if need_grad_x else None
    check(lib.pygamd_head_dot_backward(_p(x2), _ld(x2), _p(att_a), _p(att_b), _p(grad_a),
                                       _p(grad_b), n, H, C, _p(grad_x),
                                       _ld(grad_x) if grad_x is not None else 0,
                                       1 if accumulate_into is not None else 0, _p(g_att_a),
                                       _p(g_att_b), _stream(x)), 'head_dot_backward')
    return grad_x, g_att_a, g_att_b


def sample_counts(colptr: Tensor, frontier: Tensor, k: int,
                  n_valid: Optional[Tensor] = None, replace: bool = False) -> Tensor:
    """min(deg, k) per frontier entry (``replace`` with ``k >= 0``: k wherever deg > 0); entries
    past the device-side count ``n_valid`` (int64 [1]) of a fixed-capacity frontier get 0."""
    _require_device(colptr, frontier, n_valid)
    lib = _lib.load()
    cnt = torch.empty_like(frontier)
    check(lib.pygamd_sample_counts(_p(colptr), _idx_dtype(colptr), _p(frontier),
                                   frontier.numel(), k, int(replace and k >= 0), _p(n_valid),
                                   _p(cnt), _stream(colptr)),
          'sample_counts')
    return cnt


def sample_temporal_window(colptr: Tensor, row: Tensor, time: Tensor, frontier: Tensor,
                           frontier_time: Tensor, k: int, edge_level: bool = False,
                           replace: bool = False, last: bool = False,
                           n_valid: Optional[Tensor] = None):
    """(lo, hi, cnt) per frontier entry (``pygamd_sample_temporal_window``): the eligible window
    ``[s, hi)`` of the node's time-sorted column (time key <= ``frontier_time``, int64 [F]), narrowed
    to its last ``k`` slots for ``last`` (``k >= 0``), and :func:`sample_counts`' rule on it.
    ``time``: int64 node times ``[N]``, or edge times ``[E]`` in CSC slot order with
    ``edge_level``."""
    _require_device(colptr, row, time, frontier, frontier_time, n_valid)
    if time.dtype != torch.int64 or frontier_time.dtype != torch.int64:
        raise ValueError("'time' and 'frontier_time' must be int64")
    if frontier_time.numel() != frontier.numel():
        raise ValueError("'frontier_time' needs one entry per frontier node")
    time, frontier_time = time.contiguous(), frontier_time.contiguous()
    lib = _lib.load()
    lo = torch.empty_like(frontier)
    hi = torch.empty_like(frontier)
    cnt = torch.empty_like(frontier)
    check(lib.pygamd_sample_temporal_window(
        _p(colptr), _p(row), _idx_dtype(colptr), _p(time), int(edge_level), _p(frontier),
        _p(frontier_time), frontier.numel(), k, int(replace and k >= 0), int(last), _p(n_valid),
        _p(lo), _p(hi), _p(cnt), _stream(colptr)), 'sample_temporal_window')
    return lo, hi, cnt


def _relabel_assign(src_global: Tensor, local_map: Tensor, total: Optional[Tensor] = None,
                    base=0, zero_fill: bool = False):
    """Phases 0-2 of ``pygamd_relabel`` and the scan between them: the sources not yet in
    ``local_map`` get the local ids ``base``, ``base + 1``, ... in order of first appearance.
    ``total`` (int64 [1], device): only that many entries of ``src_global`` are real (a static
    capacity); ``base``: a host int, or int64 [1] on the device.  Returns ``(new_nodes, n_new)`` at
    the capacity ``len(src_global)`` (entries past the count are unwritten, 0 with ``zero_fill``)
    with ``n_new`` int64 [1] on the device.  No host read."""
    lib = _lib.load()
    m = src_global.numel()
    dt, st, dev = _idx_dtype(src_global), _stream(src_global), src_global.device
    new_nodes = (torch.zeros if zero_fill else torch.empty)(m, dtype=src_global.dtype, device=dev)
    if m == 0:
        return new_nodes, torch.zeros(1, dtype=torch.int64, device=dev)
    base_dev = base if isinstance(base, Tensor) else None
    check(lib.pygamd_relabel(0, _p(src_global), dt, m, _p(total), _p(local_map), None, 0, None,
                             None, st))
    flag = torch.empty(m, dtype=torch.int64, device=dev)
    check(lib.pygamd_relabel(1, _p(src_global), dt, m, _p(total), _p(local_map), _p(flag), 0,
                             None, None, st))
    scan = cumsum(flag, out=flag)
    check(lib.pygamd_relabel(2, _p(src_global), dt, m, _p(total), _p(local_map), _p(scan),
                             0 if base_dev is not None else base, _p(base_dev), _p(new_nodes), st))
    return new_nodes, scan[-1:]


def relabel_new_nodes(src_global: Tensor, local_map: Tensor, base: int):
    """Assigns local ids base, base+1, ... to the sources not yet in `local_map` (order of first
    appearance) and returns (new_nodes, row_local).  One host sync (the number of new nodes)."""
    _require_device(src_global, local_map)
    if src_global.numel() == 0:
        return src_global.new_empty(0), src_global.new_empty(0)
    new_nodes, n_new = _relabel_assign(src_global, local_map, None, base)
    rows = relabel_lookup(src_global, None, local_map)
    return new_nodes[:int(n_new)], rows  # host sync: sizes the next hop (the frontier)


def relabel_new_nodes_padded(src_global: Tensor, total: Tensor, local_map: Tensor, base: Tensor):
    """The same WITHOUT a host sync: ``src_global`` has the hop's static capacity, ``total`` (int64
    [1], device) of its entries are real, ``base`` (int64 [1], device) nodes are in the batch so
    far.  Returns (new_nodes [capacity] zero-padded, row_local [capacity] zero-padded, n_new int64
    [1] on the device)."""
    _require_device(src_global, total, local_map, base)
    new_nodes, n_new = _relabel_assign(src_global, local_map, total, base, zero_fill=True)
    return new_nodes, relabel_lookup(src_global, total, local_map), n_new


def sample_negatives(n: int, num_nodes: int, seed: int, device, dtype=torch.int64,
                     cdf: Optional[Tensor] = None, node_time: Optional[Tensor] = None,
                     bound: Optional[Tensor] = None, fallback: int = 0,
                     seed_dev: Optional[Tensor] = None) -> Tensor:
    """``n`` negative node ids (``pygamd_sample_negatives``): uniform over ``[0, num_nodes)``, or
    in proportion to weight given their fp64 inclusive ``cdf`` ``[num_nodes]``; with ``node_time``
    (int64 ``[num_nodes]``) draw ``j`` is accepted iff ``node_time[c] <= bound[j % len(bound)]``
    (int64), up to 6 candidates, then ``fallback``."""
    if dtype not in (torch.int32, torch.int64):
        raise ValueError(f"negatives are int32 or int64 node ids (got {dtype})")
    if n < 0:
        raise ValueError(f"the number of negatives must be non-negative (got {n})")
    if n > 0 and num_nodes <= 0:
        raise ValueError('negatives need a graph with at least one node')
    if cdf is not None and (cdf.dtype != torch.float64 or cdf.dim() != 1
                            or cdf.numel() != num_nodes):
        raise ValueError(f"'cdf' must be a one-dimensional float64 tensor with {num_nodes} "
                         f"entries")
    if (node_time is None) != (bound is None):
        raise ValueError("'node_time' and 'bound' go together")
    if node_time is not None:
        if node_time.dtype != torch.int64 or node_time.numel() != num_nodes:
            raise ValueError(f"'node_time' must be int64 with {num_nodes} entries")
        if bound.dtype != torch.int64 or bound.dim() != 1 or (n > 0 and bound.numel() == 0):
            raise ValueError("'bound' must be a non-empty one-dimensional int64 tensor")
        if not 0 <= fallback < num_nodes:
            raise ValueError(f"'fallback' must be a node id in [0, {num_nodes})")
        node_time, bound = node_time.contiguous(), bound.contiguous()
    out = torch.empty(n, dtype=dtype, device=device)
    _require_device(out, cdf, node_time, bound, seed_dev)
    if n == 0:
        return out
    lib = _lib.load()
    check(lib.pygamd_sample_negatives(
        n, num_nodes, seed & 0xFFFFFFFFFFFFFFFF, _p(seed_dev), _p(cdf), _p(node_time), _p(bound),
        0 if bound is None else bound.numel(), int(fallback), _idx_dtype(out), _p(out),
        _stream(out)), 'sample_negatives')
    return out


def unique_inverse(keys: Tensor, max_value: Optional[int] = None, count_on_device: bool = False):
    """``torch.unique(keys, return_inverse=True)`` of non-negative int32 / int64 ids (sorted; the
    inverse is int64): :func:`index_sort` (``max_value`` bounds its passes), then
    ``pygamd_unique_inverse``.  One host read, the number of distinct keys.
    ``count_on_device``: no host read; returns ``(uniq, inverse, n_unique)`` with ``uniq`` at its
    capacity ``len(keys)`` (entries past the count are unwritten) and ``n_unique`` int64 ``[1]`` on
    the device, for a caller that reads the count together with other values."""
    _require_device(keys)
    if keys.dim() != 1:
        raise ValueError("'keys' must be one-dimensional")
    _idx_dtype(keys)
    n = keys.numel()
    if n == 0:
        empty = (keys.new_empty(0), torch.empty(0, dtype=torch.int64, device=keys.device))
        return empty + (torch.zeros(1, dtype=torch.int64, device=keys.device), ) \
            if count_on_device else empty
    sorted_k, perm = index_sort(keys, max_value)
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    check(lib.pygamd_cumsum_workspace_bytes(_lib.IDX_I64, n, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=keys.device)
    rank = torch.empty(n, dtype=torch.int64, device=keys.device)
    uniq = torch.empty_like(sorted_k)
    inverse = torch.empty(n, dtype=torch.int64, device=keys.device)
    n_unique = torch.empty(1, dtype=torch.int64, device=keys.device)
    check(lib.pygamd_unique_inverse(_p(sorted_k), _p(perm), _idx_dtype(keys), n, _p(rank), _p(ws),
                                    nbytes.value, _p(uniq), _p(inverse), _p(n_unique),
                                    _stream(keys)), 'unique_inverse')
    if count_on_device:
        return uniq, inverse, n_unique
    return uniq[:int(n_unique)], inverse  # host read: sizes the seed block


# ---- heterogeneous sampling: the typed layer over one stacked CSC -----------------------------------
def _i64_host(values):
    """A host int64 array for the small per-type tables of the hetero entry points."""
    arr = (ctypes.c_int64 * max(len(values), 1))(*values)
    return arr


LINK_NEG_MODES = {None: _lib.CONSTANTS['PYGAMD_LINK_NEG_NONE'],
                  'none': _lib.CONSTANTS['PYGAMD_LINK_NEG_NONE'],
                  'binary': _lib.CONSTANTS['PYGAMD_LINK_NEG_BINARY'],
                  'triplet': _lib.CONSTANTS['PYGAMD_LINK_NEG_TRIPLET']}


def hetero_link_seeds(src: Tensor, dst: Tensor, num_neg: int, mode, seed: int, endpoints,
                      link_time: Optional[Tensor] = None
                      ) -> Tuple[Tensor, Optional[Tensor]]:
    """``pygamd_hetero_link_seeds``: the typed seed block of a heterogeneous edge batch in one
    launch.  ``src`` / ``dst``: the typed local endpoints ``[P]`` of the positive links (device,
    one index dtype); ``mode``: ``None`` / ``'binary'`` / ``'triplet'``; ``endpoints``: two dicts
    (source, destination) with ``num_nodes``, ``node_base`` and optionally ``cdf`` (fp64
    ``[num_nodes]``), ``node_time`` (int64 ``[num_nodes]``, that type's slice) and ``fallback``.
    Returns ``(seeds, seed_time)``: the global ids ``[n_src + n_dst]`` (source block first,
    positives then negatives; the negative in slot ``P + j`` of endpoint ``e`` is
    :func:`sample_negatives`' draw ``j`` for the seed ``seed * 2 + e``), and, with ``link_time``
    (int64 ``[P]``), the int64 time ``link_time[j % P]`` of every slot (else ``None``)."""
    if mode not in LINK_NEG_MODES:
        raise ValueError(f"'mode' must be None, 'binary' or 'triplet' (got {mode!r})")
    m = LINK_NEG_MODES[mode]
    if src.dim() != 1 or dst.dim() != 1 or src.numel() != dst.numel() or src.dtype != dst.dtype:
        raise ValueError("'src' and 'dst' must be one-dimensional, of one length and one dtype")
    dt = _idx_dtype(src)
    P = src.numel()
    if num_neg < 0 or (num_neg > 0 and (m == 0 or P == 0)):
        raise ValueError(f"'num_neg' must be non-negative, and zero without a negative-sampling "
                         f"mode or without positive links (got {num_neg})")
    if len(endpoints) != 2:
        raise ValueError("'endpoints' describes the source and the destination endpoint")
    if link_time is not None and (link_time.dtype != torch.int64 or link_time.dim() != 1
                                  or link_time.numel() != P):
        raise ValueError(f"'link_time' must be a one-dimensional int64 tensor with {P} entries")
    table, cdfs, times = [], [], []
    for e, ep in enumerate(endpoints):
        n, base = int(ep['num_nodes']), int(ep['node_base'])
        cdf, node_time = ep.get('cdf'), ep.get('node_time')
        fallback = int(ep.get('fallback') or 0)
        draws = num_neg > 0 and (m == 1 or (m == 2 and e == 1))
        if n < 0 or base < 0:
            raise ValueError("'num_nodes' and 'node_base' must be non-negative")
        if draws and n <= 0:
            raise ValueError('negatives need a node type with at least one node')
        if src.dtype == torch.int32 and base + n > 2 ** 31 - 1:
            raise ValueError('int32 seeds: the global ids of the endpoint type do not fit')
        if cdf is not None and (cdf.dtype != torch.float64 or cdf.dim() != 1
                                or cdf.numel() != n):
            raise ValueError(f"'cdf' must be a one-dimensional float64 tensor with {n} entries")
        if node_time is not None:
            if link_time is None:
                raise ValueError("'node_time' bounds the negatives by 'link_time', which is "
                                 "missing")
            if node_time.dtype != torch.int64 or node_time.dim() != 1 or node_time.numel() != n \
                    or not node_time.is_contiguous():
                raise ValueError(f"'node_time' must be contiguous int64 with {n} entries")
            if not 0 <= fallback < n:
                raise ValueError(f"'fallback' must be a node id in [0, {n})")
        table += [n, base, fallback]
        cdfs.append(None if cdf is None else cdf.contiguous())
        times.append(node_time)
    _require_device(src, dst, link_time, *cdfs, *times)
    n_src = P + (num_neg if m == 1 else 0)
    n_dst = P + (num_neg if m >= 1 else 0)
    seeds = torch.empty(n_src + n_dst, dtype=src.dtype, device=src.device)
    seed_time = None if link_time is None else \
        torch.empty(n_src + n_dst, dtype=torch.int64, device=src.device)
    if P == 0:
        return seeds, seed_time
    src, dst = src.contiguous(), dst.contiguous()
    link_time = None if link_time is None else link_time.contiguous()
    check(_lib.load().pygamd_hetero_link_seeds(
        _p(src), _p(dst), dt, P, int(num_neg), m, _p(link_time), _i64_host(table), _p(cdfs[0]),
        _p(cdfs[1]), _p(times[0]), _p(times[1]), seed & 0xFFFFFFFFFFFFFFFF, _p(seeds),
        _p(seed_time), _stream(seeds)), 'hetero_link_seeds')
    return seeds, seed_time


def _hop_tables(item_begin, et_table):
    """The ``item_begin, et_table, n_et`` arguments of the typed hop entry points as host arrays
    (``et_table``: rows ``(frontier_off, col_off, dst_local, k)`` per edge type)."""
    return (_i64_host(item_begin), _i64_host([int(v) for r in et_table for v in r]),
            len(et_table))


def hetero_sample_counts(colptr: Tensor, frontier: Tensor, item_begin, et_table,
                         replace: bool = False) -> Tensor:
    """``pygamd_hetero_sample_counts``: per work item of a hop, ``min(deg, k)`` with the ``k`` of
    the item's edge type (see ``include/pyg_amd.h``).  ``item_begin``: host ints ``[n_et + 1]``;
    ``et_table``: rows ``(frontier_off, col_off, dst_local, k)`` per edge type."""
    _require_device(colptr, frontier)
    if frontier.dtype != colptr.dtype:
        raise ValueError("'frontier' must have the graph's index dtype")
    lib = _lib.load()
    n = int(item_begin[-1])
    cnt = torch.empty(n, dtype=colptr.dtype, device=colptr.device)
    check(lib.pygamd_hetero_sample_counts(_p(colptr), _idx_dtype(colptr), _p(frontier),
                                          *_hop_tables(item_begin, et_table), int(replace),
                                          _p(cnt), _stream(colptr)), 'hetero_sample_counts')
    return cnt


def hetero_sample_neighbors(colptr: Tensor, row: Tensor, perm: Tensor, frontier: Tensor,
                            offsets: Tensor, capacity: int, item_begin, et_table, seed: int,
                            replace: bool = False, salt_position: bool = False,
                            want_fpos: bool = False,
                            window: Optional[Tuple[Tensor, Tensor]] = None):
    """``pygamd_hetero_sample_neighbors``: ``(src_global, col_local, edge, fpos)`` of one hop at the
    static ``capacity`` (entries past ``offsets[-1]`` are not written, except ``fpos``, which is
    zero-filled; ``None`` unless ``want_fpos``).  ``window``: the ``(lo, hi)`` of
    :func:`hetero_sample_temporal_window`; the same draws and outputs on the slots ``[lo, hi)`` of
    every item (``pygamd_hetero_sample_neighbors_temporal``)."""
    _require_device(colptr, row, perm, frontier, offsets, *(window or ()))
    lib = _lib.load()
    dt, dev = colptr.dtype, colptr.device
    src = torch.empty(capacity, dtype=dt, device=dev)
    col = torch.empty(capacity, dtype=dt, device=dev)
    edge = torch.empty(capacity, dtype=dt, device=dev)
    fpos = torch.zeros(capacity, dtype=dt, device=dev) if want_fpos else None
    # the arguments both draw entry points end with
    tail = (_p(offsets), *_hop_tables(item_begin, et_table), seed & 0xFFFFFFFFFFFFFFFF,
            int(replace) | (2 if salt_position else 0), _p(src), _p(col), _p(edge), _p(fpos),
            _stream(colptr))
    if capacity > 0 and int(item_begin[-1]) > 0 and window is not None:
        check(lib.pygamd_hetero_sample_neighbors_temporal(
            _p(row), _p(perm), _idx_dtype(row), _p(frontier), _p(window[0]), _p(window[1]),
            *tail), 'hetero_sample_neighbors_temporal')
    elif capacity > 0 and int(item_begin[-1]) > 0:
        check(lib.pygamd_hetero_sample_neighbors(
            _p(colptr), _p(row), _p(perm), _idx_dtype(colptr), _p(frontier), *tail),
            'hetero_sample_neighbors')
    return src, col, edge, fpos


def hetero_sample_temporal_window(colptr: Tensor, row: Tensor, time: Tensor, frontier: Tensor,
                                  frontier_time: Tensor, item_begin, et_table, timed_mask: int,
                                  edge_level: bool = False, replace: bool = False,
                                  last: bool = False):
    """``pygamd_hetero_sample_temporal_window``: ``(lo, hi, cnt)`` per work item of a temporal hop.
    A timed edge type (its bit of ``timed_mask``) gets the prefix of the item's time-sorted column
    with time <= ``frontier_time`` (int64, aligned with ``frontier``), narrowed to its last ``k``
    slots for ``last``; an untimed one its whole column.  ``cnt`` follows
    :func:`hetero_sample_counts`' rule on the window.  ``time``: int64 over the global node ids,
    or over the slots with ``edge_level``."""
    _require_device(colptr, row, time, frontier, frontier_time)
    if frontier.dtype != colptr.dtype:
        raise ValueError("'frontier' must have the graph's index dtype")
    if time.dtype != torch.int64 or frontier_time.dtype != torch.int64:
        raise ValueError("'time' and 'frontier_time' must be int64")
    time, frontier_time = time.contiguous(), frontier_time.contiguous()
    lib = _lib.load()
    n = int(item_begin[-1])
    lo = torch.empty(n, dtype=colptr.dtype, device=colptr.device)
    hi = torch.empty(n, dtype=colptr.dtype, device=colptr.device)
    cnt = torch.empty(n, dtype=colptr.dtype, device=colptr.device)
    check(lib.pygamd_hetero_sample_temporal_window(
        _p(colptr), _p(row), _idx_dtype(colptr), _p(time), int(edge_level), _p(frontier),
        _p(frontier_time), *_hop_tables(item_begin, et_table),
        int(timed_mask), int(replace), int(last), _p(lo), _p(hi), _p(cnt), _stream(colptr)),
        'hetero_sample_temporal_window')
    return lo, hi, cnt


def hetero_split(new_nodes: Tensor, n_new: Tensor, node_base, count_prev, offsets: Optional[Tensor],
                 item_begin, local_map: Optional[Tensor] = None, want_typed: bool = False,
                 aux: Optional[Tensor] = None):
    """``pygamd_hetero_split`` (both phases and the scan between them): the stable partition by
    node type of the hop's new nodes (the first ``n_new`` (int64 [1], device) of ``new_nodes``).
    Returns ``(sorted_global, sorted_local, typed, aux_sorted, stats)``: the type-major buffers,
    the typed local id of every new node (``want_typed``; else ``None``), ``aux`` (int64) in
    type-major order, and the int64 stats ``[n_t + n_et + 1]`` (new nodes per type, then the edge
    boundaries ``offsets[item_begin[e]]``)."""
    _require_device(new_nodes, n_new, offsets, local_map, aux)
    lib = _lib.load()
    m = new_nodes.numel()
    dt, dev = new_nodes.dtype, new_nodes.device
    n_t, n_et = len(node_base) - 1, len(item_begin) - 1
    sorted_global = torch.empty(m, dtype=dt, device=dev)
    sorted_local = torch.empty(m, dtype=dt, device=dev)
    typed = torch.empty(m, dtype=dt, device=dev) if want_typed else None
    aux_sorted = torch.empty(m, dtype=torch.int64, device=dev) if aux is not None else None
    stats = torch.zeros(n_t + n_et + 1, dtype=torch.int64, device=dev)
    if m == 0:
        return sorted_global, sorted_local, typed, aux_sorted, stats
    nb, cp, ib = _i64_host(node_base), _i64_host(count_prev), _i64_host(item_begin)
    flag = torch.empty(n_t * m, dtype=torch.int64, device=dev)
    st = _stream(new_nodes)
    check(lib.pygamd_hetero_split(0, _p(new_nodes), _idx_dtype(new_nodes), m, _p(n_new), nb, cp,
                                  n_t, _p(flag), None, ib, n_et, None, None, None, None, None,
                                  None, None, st), 'hetero_split')
    cumsum(flag, out=flag)
    check(lib.pygamd_hetero_split(1, _p(new_nodes), _idx_dtype(new_nodes), m, _p(n_new), nb, cp,
                                  n_t, _p(flag), _p(offsets), ib, n_et, _p(aux), _p(local_map),
                                  _p(typed), _p(sorted_global), _p(sorted_local), _p(aux_sorted),
                                  _p(stats), st), 'hetero_split')
    return sorted_global, sorted_local, typed, aux_sorted, stats


def relabel_claim_assign(src_global: Tensor, total: Tensor, local_map: Tensor):
    """Phases 0-2 of ``pygamd_relabel`` at a static capacity (``total``: int64 [1] on the device):
    ``(new_nodes [capacity], n_new int64 [1])``, the new sources in order of first appearance;
    ``local_map`` holds their ranks afterwards.  No host read."""
    _require_device(src_global, total, local_map)
    return _relabel_assign(src_global, local_map, total)


def relabel_lookup(src_global: Tensor, total: Optional[Tensor], local_map: Tensor) -> Tensor:
    """Phase 3 of ``pygamd_relabel``: ``local_map[src]`` for the first ``total`` entries (all of
    them for ``None``), 0 after."""
    _require_device(src_global, total, local_map)
    lib = _lib.load()
    out = torch.empty_like(src_global)
    if src_global.numel() > 0:
        check(lib.pygamd_relabel(3, _p(src_global), _idx_dtype(src_global), src_global.numel(),
                                 _p(total), _p(local_map), None, 0, None, _p(out),
                                 _stream(src_global)))
    return out


def edge_key(row: Tensor, col: Tensor, num_nodes: int, by_row: bool) -> Tensor:
    _require_device(row, col)
    lib = _lib.load()
    row, col = row.contiguous(), col.contiguous()
    key = torch.empty(row.numel(), dtype=torch.int64, device=row.device)
    check(lib.pygamd_edge_key(_p(row), _p(col), _idx_dtype(row), row.numel(), num_nodes,
                              int(by_row), _p(key), _stream(row)), 'edge_key')
    return key


def edge_unkey(key_sorted: Tensor, num_nodes: int, by_row: bool, dtype: torch.dtype,
               scan: Optional[Tensor] = None, perm: Optional[Tensor] = None,
               n_out: Optional[int] = None, want_groups: bool = False):
    """(edge_index [2, n_out], gid_orig | None)"""
    _require_device(key_sorted)
    lib = _lib.load()
    E = key_sorted.numel()
    out = torch.empty(2, E if n_out is None else n_out, dtype=dtype, device=key_sorted.device)
    gid = (torch.empty(E, dtype=torch.int64, device=key_sorted.device)
           if (want_groups and scan is not None) else None)
    check(lib.pygamd_edge_unkey(_p(key_sorted), None if scan is None else _p(scan),
                                None if perm is None else _p(perm), E, num_nodes, int(by_row),
                                _idx_dtype(out), _p(out[0]), _p(out[1]),
                                None if gid is None else _p(gid), _stream(key_sorted)),
          'edge_unkey')
    return out, gid


def run_flags(key_sorted: Tensor) -> Tensor:
    _require_device(key_sorted)
    lib = _lib.load()
    flag = torch.empty_like(key_sorted)
    check(lib.pygamd_run_flags(_p(key_sorted), key_sorted.numel(), _p(flag),
                               _stream(key_sorted)), 'run_flags')
    return flag


# ---- heterogeneous layers: every edge type of a HeteroConv in one aggregation ------------------------
MAX_HETERO_TYPES = 64


def _ptr_host(tensors):
    """A host array of device pointers (NULL for None / empty tensors)."""
    vals = [None if (t is None or t.numel() == 0) else t.data_ptr() for t in tensors]
    return (ctypes.c_void_p * max(len(vals), 1))(*vals)


def _hetero_block(t: Tensor, name: str, F: int) -> Tensor:
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.size(1) == F
            and (F <= 1 or t.stride(1) == 1) and (t.size(0) <= 1 or t.stride(0) >= F)):
        raise ValueError(f"'{name}' must hold float32 HIP row blocks [n, {F}] with unit inner "
                         f"stride")
    return t


def hetero_spmm(rowptr: Tensor, col: Tensor, row_begin, xs, outs, means,
                check_bounds: bool = False) -> None:
    """``pygamd_hetero_spmm``: ``outs[et][i] = sum | mean`` of ``xs[et][col[slot]]`` over the slots
    of the stacked row ``row_begin[et] + i`` — every edge type in one launch.  ``row_begin``: host
    ints ``[n_et + 1]``; ``xs[et]``: the ``[n_src, F]`` float32 source matrix of edge type ``et``
    (row-strided views are fine); ``outs[et]``: its ``[rows, F]`` output block, written in place
    (e.g. a column block of a wider matrix); ``means[et]``: mean instead of sum.
    ``check_bounds``: report a source id outside its matrix as ``INDEX_CHECK`` says (the kernel
    reads row 0 for it in every mode); callers that range-checked ``col`` leave it off."""
    _require_device(rowptr, col, *xs, *outs)
    n_et = len(xs)
    if not (len(outs) == len(means) == n_et and len(row_begin) == n_et + 1):
        raise ValueError("'row_begin', 'xs', 'outs' and 'means' disagree about the edge types")
    if n_et > MAX_HETERO_TYPES:
        raise PygAmdError(f'hetero_spmm failed: at most {MAX_HETERO_TYPES} edge types per launch '
                          f'(got {n_et})')
    if col.dtype != rowptr.dtype or rowptr.dim() != 1 or col.dim() != 1:
        raise ValueError("'rowptr' and 'col' must be one-dimensional and of one index dtype")
    if n_et == 0:
        return
    F = xs[0].size(1) if xs[0].dim() == 2 else -1
    n_rows = int(row_begin[-1])
    if rowptr.numel() != n_rows + 1:
        raise ValueError(f"'rowptr' must have {n_rows + 1} entries (got {rowptr.numel()})")
    table = []
    for et in range(n_et):
        x, o = _hetero_block(xs[et], 'xs', F), _hetero_block(outs[et], 'outs', F)
        rows = int(row_begin[et + 1]) - int(row_begin[et])
        if o.size(0) != rows:
            raise ValueError(f"'outs[{et}]' must have {rows} rows (got {o.size(0)})")
        table += [_ld(x), x.size(0), int(bool(means[et])), _ld(o)]
    rowptr, col = rowptr.contiguous(), col.contiguous()
    active = check_bounds and n_rows > 0 and F > 0 and col.numel() > 0
    ring, slot, err = _index_flag(rowptr.device, active)
    check(_lib.load().pygamd_hetero_spmm(
        _p(rowptr), _p(col), _idx_dtype(rowptr), _i64_host([int(v) for v in row_begin]),
        _ptr_host(xs), _ptr_host(outs), _i64_host(table), n_et, F, _p(err), _stream(rowptr)),
        'hetero_spmm')
    if active:
        _hetero_flag_done(ring, slot, err)


def _raise_hetero_out_of_range():
    raise IndexOutOfRange("hetero_spmm: 'col' holds a source id outside [0, n_src) of its edge "
                          "type's source matrix (the kernel read row 0 for it)")


def _hetero_flag_done(ring, slot, err):
    """:func:`_index_flag_done` for :func:`hetero_spmm`: same delivery (async ring / blocking
    read), its own report."""
    if ring is not None:
        ring.publish(slot, 'hetero_spmm', 0, None, report=_raise_hetero_out_of_range)
    elif err is not None and INDEX_CHECK == 'sync' \
            and not torch.cuda.is_current_stream_capturing() and int(err.item()) != 0:
        _raise_hetero_out_of_range()


def hetero_spmm_backward(rowptr_t: Tensor, col_t: Tensor, rowptr: Tensor, row_begin, grads,
                         means, src_begin, grad_xs) -> None:
    """``pygamd_hetero_spmm_backward``: the input gradients of :func:`hetero_spmm` for every source
    node type in one launch, without atomics.  ``rowptr_t`` / ``col_t``: the transposed structure
    over the stacked source nodes (``src_begin``: host ints ``[n_nt + 1]``), whose slots name
    stacked rows; ``grads[et]``: the ``[rows, F]`` gradient of edge type ``et``'s output block;
    ``grad_xs[t]``: the ``[n, F]`` gradient of source node type ``t``, overwritten."""
    _require_device(rowptr_t, col_t, rowptr, *grads, *grad_xs)
    n_et, n_nt = len(grads), len(grad_xs)
    if not (len(means) == n_et and len(row_begin) == n_et + 1 and len(src_begin) == n_nt + 1):
        raise ValueError("'row_begin', 'grads', 'means', 'src_begin' and 'grad_xs' disagree about "
                         "the types")
    if n_et > MAX_HETERO_TYPES or n_nt > MAX_HETERO_TYPES:
        raise PygAmdError(f'hetero_spmm_backward failed: at most {MAX_HETERO_TYPES} edge types and '
                          f'node types per launch (got {n_et}, {n_nt})')
    if not (rowptr_t.dtype == col_t.dtype == rowptr.dtype):
        raise ValueError('the index tensors must share one dtype')
    if n_et == 0 or n_nt == 0:
        return
    F = grads[0].size(1) if grads[0].dim() == 2 else -1
    n_rows, n_src = int(row_begin[-1]), int(src_begin[-1])
    if rowptr.numel() != n_rows + 1 or rowptr_t.numel() != n_src + 1:
        raise ValueError(f"'rowptr' / 'rowptr_t' must have {n_rows + 1} / {n_src + 1} entries")
    table = []
    for et in range(n_et):
        g = _hetero_block(grads[et], 'grads', F)
        rows = int(row_begin[et + 1]) - int(row_begin[et])
        if g.size(0) != rows:
            raise ValueError(f"'grads[{et}]' must have {rows} rows (got {g.size(0)})")
        table += [_ld(g), int(bool(means[et]))]
    lds = []
    for t in range(n_nt):
        gx = _hetero_block(grad_xs[t], 'grad_xs', F)
        rows = int(src_begin[t + 1]) - int(src_begin[t])
        if gx.size(0) != rows:
            raise ValueError(f"'grad_xs[{t}]' must have {rows} rows (got {gx.size(0)})")
        lds.append(_ld(gx))
    check(_lib.load().pygamd_hetero_spmm_backward(
        _p(rowptr_t.contiguous()), _p(col_t.contiguous()), _p(rowptr.contiguous()),
        _idx_dtype(rowptr), _i64_host([int(v) for v in row_begin]), _ptr_host(grads),
        _i64_host(table), n_et, _i64_host([int(v) for v in src_begin]), _ptr_host(grad_xs),
        _i64_host(lds), n_nt, F, _stream(rowptr)), 'hetero_spmm_backward')


# ---- HGTConv: the typed relation transform (csrc/hgt.hip) ----------------------------------------
def hgt_supported(H: int, D: int) -> bool:
    """The relation kernels serve this head layout (H * D <= 512, H <= 64, D <= 128)."""
    return bool(_lib.load().pygamd_hgt_supported(int(H), int(D)))


def _hgt_table(ks, vs, widx, src_type, F: int):
    n_et = len(ks)
    if not (len(vs) == len(widx) == len(src_type) == n_et):
        raise ValueError("'ks', 'vs', 'widx' and 'src_type' disagree about the edge types")
    if n_et > MAX_HETERO_TYPES:
        raise PygAmdError(f'hgt_relation failed: at most {MAX_HETERO_TYPES} edge types per launch '
                          f'(got {n_et})')
    table = []
    for e in range(n_et):
        k, v = _hetero_block(ks[e], 'ks', F), _hetero_block(vs[e], 'vs', F)
        if k.size(0) != v.size(0) or _ld(k) != _ld(v):
            raise ValueError(f"'ks[{e}]' and 'vs[{e}]' need the same rows and row stride")
        table += [_ld(k), k.size(0), int(widx[e]), int(src_type[e])]
    return table


def _hgt_weights(wk: Tensor, wv: Tensor, H: int, D: int) -> int:
    for w in (wk, wv):
        if not (w.is_cuda and w.dtype == torch.float32 and w.dim() == 3 and w.is_contiguous()
                and w.size(1) == D and w.size(2) == D and w.size(0) % H == 0):
            raise ValueError(f"the relation weights must be contiguous float32 [H * T, {D}, {D}] "
                             f"HIP tensors (got {tuple(w.shape)})")
    if wk.shape != wv.shape:
        raise ValueError('the key and value relation weights must have one shape')
    return wk.size(0) // H


def hgt_relation_forward(ks, vs, widx, wk: Tensor, wv: Tensor, H: int, D: int) -> Tensor:
    """``pygamd_hgt_relation_forward``: the packed ``kv [S, 2 * H * D]`` of the stacked source rows
    of every edge type of a call in one launch: ``kv[off[e] + j, 0, h] = ks[e][j, h] @ wk[h * T +
    widx[e]]``, and ``vs`` / ``wv`` in the second half.  ``ks[e]`` / ``vs[e]``: ``[n_e, H * D]``
    float32 row blocks read in place (column blocks of a wider projection are fine)."""
    _require_device(wk, wv, *ks, *vs)
    F = H * D
    T = _hgt_weights(wk, wv, H, D)
    table = _hgt_table(ks, vs, widx, [0] * len(ks), F)
    S = sum(k.size(0) for k in ks)
    kv = torch.empty(S, 2 * F, dtype=torch.float32, device=wk.device)
    if not ks:
        return kv
    with _timed({'kind': 'hgt', 'op': 'relation_forward', 'S': S, 'H': H, 'D': D,
                 'n_et': len(ks)}, wk):
        check(_lib.load().pygamd_hgt_relation_forward(
            _ptr_host(ks), _ptr_host(vs), _i64_host(table), len(ks), _p(wk), _p(wv), T, H, D,
            _p(kv), _stream(wk)), 'hgt_relation_forward')
    return kv


def hgt_relation_backward(ks, vs, widx, src_type, wk: Tensor, wv: Tensor, H: int, D: int,
                          grad_kv: Tensor, grad_ks, grad_vs, weight_grads: bool = True):
    """``pygamd_hgt_relation_backward``: ``grad_ks[t]`` / ``grad_vs[t]`` (``[N_t, H * D]`` row
    blocks of source node type ``t``, e.g. column blocks of one ``[N_t, 3 * H * D]`` buffer) are
    overwritten with the input gradients, summed over the edge types with ``src_type[e] == t`` in
    call order; returns ``(grad_wk, grad_wv)`` (every matrix written) or ``(None, None)``.  No
    atomics: bitwise reproducible."""
    _require_device(wk, wv, grad_kv, *ks, *vs, *grad_ks, *grad_vs)
    lib = _lib.load()
    F = H * D
    T = _hgt_weights(wk, wv, H, D)
    table = _hgt_table(ks, vs, widx, src_type, F)
    S = sum(k.size(0) for k in ks)
    if not (grad_kv.dtype == torch.float32 and grad_kv.shape == (S, 2 * F)):
        raise ValueError(f"'grad_kv' must be float32 [{S}, {2 * F}] (got {tuple(grad_kv.shape)})")
    grad_kv = grad_kv.contiguous()
    if len(grad_ks) != len(grad_vs) or len(grad_ks) > MAX_HETERO_TYPES:
        raise PygAmdError(f'hgt_relation_backward failed: at most {MAX_HETERO_TYPES} node types, '
                          f'one key and one value gradient block each')
    nt_table = []
    for t, (gk, gv) in enumerate(zip(grad_ks, grad_vs)):
        gk, gv = _hetero_block(gk, 'grad_ks', F), _hetero_block(gv, 'grad_vs', F)
        if gk.size(0) != gv.size(0) or _ld(gk) != _ld(gv):
            raise ValueError(f"'grad_ks[{t}]' and 'grad_vs[{t}]' need the same rows and row stride")
        nt_table += [gk.size(0), _ld(gk)]
    grad_wk = grad_wv = ws = None
    ws_bytes = 0
    if not ks:
        for g in list(grad_ks) + list(grad_vs):
            g.zero_()
        return (torch.zeros_like(wk), torch.zeros_like(wv)) if weight_grads else (None, None)
    if weight_grads:
        grad_wk, grad_wv = torch.empty_like(wk), torch.empty_like(wv)
        nbytes = ctypes.c_size_t(0)
        check(lib.pygamd_hgt_workspace_bytes(_i64_host(table), len(ks), H, D,
                                             ctypes.byref(nbytes)), 'hgt_workspace_bytes')
        ws_bytes = nbytes.value
        if ws_bytes:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=wk.device)
    with _timed({'kind': 'hgt', 'op': 'relation_backward', 'S': S, 'H': H, 'D': D,
                 'n_et': len(ks)}, wk):
        check(lib.pygamd_hgt_relation_backward(
            _ptr_host(ks), _ptr_host(vs), _i64_host(table), len(ks), _p(wk), _p(wv), T, H, D,
            _p(grad_kv), _ptr_host(grad_ks), _ptr_host(grad_vs), _i64_host(nt_table),
            len(grad_ks), _p(grad_wk), _p(grad_wv), _p(ws), ws_bytes, _stream(wk)),
            'hgt_relation_backward')
    return grad_wk, grad_wv


# ---- geometric searches (csrc/cluster.hip) -----------------------------------------------------------
KNN_MAX_K = 64        # the running best k sits one slot per lane
CLUSTER_MAX_F = 512


def cluster_supported(F: int, k: int = 1) -> bool:
    """The envelope of ``pygamd_knn`` / ``pygamd_radius`` / ``pygamd_fps``."""
    return 1 <= int(F) <= CLUSTER_MAX_F and 1 <= int(k) <= KNN_MAX_K


def _cluster_rows(t: Tensor, name: str) -> Tensor:
    if t.dim() != 2:
        raise ValueError(f"'{name}' must be two-dimensional (got {t.dim()} dimensions)")
    return _strided_rows(t, name, t.size(1))


def _cluster_ptrs(ptr_x: Tensor, ptr_y: Tensor):
    if ptr_x.dtype != ptr_y.dtype or ptr_x.numel() != ptr_y.numel() or ptr_x.numel() < 1:
        raise ValueError("'ptr_x' and 'ptr_y' need one index dtype and B + 1 entries each")
    return ptr_x.contiguous(), ptr_y.contiguous(), ptr_x.numel() - 1


def knn(x: Tensor, y: Tensor, ptr_x: Tensor, ptr_y: Tensor, k: int, cosine: bool = False,
        exclude_same_index: bool = False) -> Tuple[Tensor, Tensor]:
    """``pygamd_knn``: ``(index [M, k] int64, count [M] int32)`` — for every row of ``y`` the ``k``
    nearest rows of ``x`` of its example, ascending by (distance, index), padded with -1.  ``x`` and
    ``y`` may be column blocks of wider tensors."""
    _require_device(x, y, ptr_x, ptr_y)
    x, y = _cluster_rows(x, 'x'), _cluster_rows(y, 'y')
    if x.size(1) != y.size(1):
        raise ValueError(f"'x' and 'y' differ in width ({x.size(1)} and {y.size(1)})")
    ptr_x, ptr_y, B = _cluster_ptrs(ptr_x, ptr_y)
    N, M, F = x.size(0), y.size(0), x.size(1)
    index = torch.empty(M, int(k), dtype=torch.int64, device=y.device)
    count = torch.empty(M, dtype=torch.int32, device=y.device)
    with _timed({'kind': 'cluster', 'op': 'knn', 'N': N, 'M': M, 'F': F, 'k': int(k), 'B': B}, y):
        check(_lib.load().pygamd_knn(
            _p(x), _ld(x), N, _p(y), _ld(y), M, F, _p(ptr_x), _p(ptr_y), _idx_dtype(ptr_x), B,
            int(k), int(bool(cosine)), int(bool(exclude_same_index)), _p(index), _p(count),
            _stream(y)), 'knn')
    return index, count


def radius(x: Tensor, y: Tensor, ptr_x: Tensor, ptr_y: Tensor, r: float, max_num_neighbors: int,
           exclude_same_index: bool = False) -> Tuple[Tensor, Tensor]:
    """``pygamd_radius``: ``(index [M, max_num_neighbors] int64, count [M] int32)`` — for every row
    of ``y`` the rows of ``x`` of its example with squared distance ``< r * r`` (float32), in
    ascending index, the first ``max_num_neighbors`` of them, padded with -1."""
    _require_device(x, y, ptr_x, ptr_y)
    x, y = _cluster_rows(x, 'x'), _cluster_rows(y, 'y')
    if x.size(1) != y.size(1):
        raise ValueError(f"'x' and 'y' differ in width ({x.size(1)} and {y.size(1)})")
    ptr_x, ptr_y, B = _cluster_ptrs(ptr_x, ptr_y)
    N, M, F = x.size(0), y.size(0), x.size(1)
    cap = int(max_num_neighbors)
    index = torch.empty(M, max(cap, 0), dtype=torch.int64, device=y.device)
    count = torch.empty(M, dtype=torch.int32, device=y.device)
    with _timed({'kind': 'cluster', 'op': 'radius', 'N': N, 'M': M, 'F': F, 'cap': cap, 'B': B},
                y):
        check(_lib.load().pygamd_radius(
            _p(x), _ld(x), N, _p(y), _ld(y), M, F, _p(ptr_x), _p(ptr_y), _idx_dtype(ptr_x), B,
            float(r), cap, int(bool(exclude_same_index)), _p(index), _p(count), _stream(y)),
            'radius')
    return index, count


def fps(x: Tensor, ptr: Tensor, out_ptr: Tensor, start: Tensor, total: int) -> Tensor:
    """``pygamd_fps``: the ``total = out_ptr[-1]`` picks of farthest point sampling, example ``e``
    yielding ``out_ptr[e + 1] - out_ptr[e]`` global row indices in selection order from the global
    row ``start[e]``.  ``ptr``, ``out_ptr`` and ``start`` share one index dtype."""
    _require_device(x, ptr, out_ptr, start)
    x = _cluster_rows(x, 'x')
    B = ptr.numel() - 1
    if not (ptr.dtype == out_ptr.dtype == start.dtype) or out_ptr.numel() != B + 1 \
            or start.numel() != B or B < 0:
        raise ValueError("'ptr' and 'out_ptr' need B + 1 entries, 'start' B, in one index dtype")
    ptr, out_ptr, start = ptr.contiguous(), out_ptr.contiguous(), start.contiguous()
    N, F = x.shape
    lib = _lib.load()
    out = torch.empty(int(total), dtype=torch.int64, device=x.device)
    ws, ws_bytes = _workspace(lib.pygamd_fps_workspace_size, (N, ), x.device)
    with _timed({'kind': 'cluster', 'op': 'fps', 'N': N, 'F': F, 'B': B, 'total': int(total)}, x):
        check(lib.pygamd_fps(_p(x), _ld(x), N, F, _p(ptr), _p(out_ptr), _p(start),
                             _idx_dtype(ptr), B, int(total), _p(out), _p(ws), ws_bytes,
                             _stream(x)), 'fps')
    return out


# ---- hierarchical pooling (csrc/pool.hip) --------------------------------------------------------
# the select kernel's size thresholds: a graph up to TOPK_WAVE_NODES nodes is one wave's, a longer
# one its workgroup's up to TOPK_MAX_NODES; a batch with a longer graph takes the generic route
TOPK_WAVE_NODES = _lib.CONSTANTS['PYGAMD_TOPK_WAVE_NODES']
TOPK_MAX_NODES = _lib.CONSTANTS['PYGAMD_TOPK_MAX_NODES']
TOPK_GROUP = _lib.CONSTANTS['PYGAMD_TOPK_GROUP']


def _i64_vector(t: Tensor, name: str, n: int) -> Tensor:
    if t.dtype != torch.int64 or t.dim() != 1 or t.numel() != n:
        raise ValueError(f"'{name}' must be an int64 vector of {n} entries (got {t.dtype} "
                         f"{tuple(t.shape)})")
    return t.contiguous()


def _f32_vector(t: Tensor, name: str, n: int) -> Tensor:
    if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n:
        raise ValueError(f"'{name}' must be a float32 vector of {n} entries (got {t.dtype} "
                         f"{tuple(t.shape)})")
    return t.contiguous()


def topk_select(score: Tensor, ptr: Tensor, k: Tensor, out_ptr: Tensor, total: int,
                max_nodes: int, want_weight: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """``pygamd_topk_select``: ``(perm [total] int64, weight [total] = score[perm])`` (``weight``
    None unless ``want_weight``) — of every
    graph ``g`` (nodes ``ptr[g] .. ptr[g + 1]``) the first ``min(k[g], n_g)`` nodes by score
    descending, then node index ascending (NaN above every number, ``-0.0 == +0.0``), at the slots
    ``out_ptr[g] ..``.  ``max_nodes``: the largest graph, at most ``TOPK_MAX_NODES``."""
    _require_device(score, ptr, k, out_ptr)
    B = ptr.numel() - 1
    if B < 0 or ptr.dim() != 1:
        raise ValueError("'ptr' needs B + 1 entries")
    score = _f32_vector(score, 'score', score.numel())
    ptr = ptr.contiguous()
    k, out_ptr = _i64_vector(k, 'k', B), _i64_vector(out_ptr, 'out_ptr', B + 1)
    N, M = score.numel(), int(total)
    perm = torch.empty(M, dtype=torch.int64, device=score.device)
    weight = torch.empty(M, dtype=torch.float32, device=score.device) if want_weight else None
    with _timed({'kind': 'pool', 'op': 'topk_select', 'N': N, 'B': B, 'M': M}, score):
        check(_lib.load().pygamd_topk_select(
            _p(score), N, _p(ptr), _idx_dtype(ptr), B, _p(k), _p(out_ptr), M, int(max_nodes),
            _p(perm), _p(weight), _stream(score)), 'topk_select')
    return perm, weight


def _gather_scale_args(x: Tensor, score: Tensor, perm: Tensor):
    _require_device(x, score, perm)
    x = _f32_rows(x, 'x')
    if x.size(1) < 1:
        raise ValueError("'x' needs at least one column")
    score = _f32_vector(score, 'score', x.size(0))
    perm = _i64_vector(perm, 'perm', perm.numel())
    return x, score, perm


def gather_scale_forward(x: Tensor, score: Tensor, perm: Tensor,
                         multiplier: float) -> Tuple[Tensor, Tensor]:
    """``pygamd_gather_scale_forward``: ``(multiplier * (score[perm, None] * x[perm]),
    score[perm])`` in one launch; ``perm`` int64 without duplicates."""
    x, score, perm = _gather_scale_args(x, score, perm)
    N, F, M = x.size(0), x.size(1), perm.numel()
    out = torch.empty(M, F, dtype=torch.float32, device=x.device)
    weight = torch.empty(M, dtype=torch.float32, device=x.device)
    with _timed({'kind': 'pool', 'op': 'gather_scale_forward', 'N': N, 'F': F, 'M': M}, x):
        check(_lib.load().pygamd_gather_scale_forward(
            _p(x), _ld(x), N, F, _p(score), _p(perm), M, float(multiplier), _p(out), F,
            _p(weight), _stream(x)), 'gather_scale_forward')
    return out, weight


def gather_scale_backward(x: Tensor, score: Tensor, perm: Tensor, multiplier: float,
                          grad_out: Tensor, grad_weight: Optional[Tensor], want_x: bool = True,
                          want_score: bool = True):
    """``pygamd_gather_scale_backward``: ``(grad_x [N, F], grad_score [N])`` (None where not
    wanted) from ``grad_out [M, F]`` and the optional ``grad_weight [M]``; the rows outside
    ``perm`` are exactly zero.  Both gradients live in ONE zero-filled buffer: one memset."""
    x, score, perm = _gather_scale_args(x, score, perm)
    N, F, M = x.size(0), x.size(1), perm.numel()
    _require_device(grad_out, grad_weight)
    grad_out = _strided_rows(grad_out, 'grad_out', F)
    if grad_out.size(0) != M:
        raise ValueError(f"'grad_out' must have {M} rows (got {grad_out.size(0)})")
    if grad_weight is not None:
        grad_weight = _f32_vector(grad_weight, 'grad_weight', M)
    buf = torch.zeros(N * (F * bool(want_x) + bool(want_score)), dtype=torch.float32,
                      device=x.device)
    grad_x = buf[:N * F].view(N, F) if want_x else None
    grad_score = buf[buf.numel() - N:] if want_score else None
    with _timed({'kind': 'pool', 'op': 'gather_scale_backward', 'N': N, 'F': F, 'M': M}, x):
        check(_lib.load().pygamd_gather_scale_backward(
            _p(x), _ld(x), N, F, _p(score), _p(perm), M, float(multiplier), _p(grad_out),
            _ld(grad_out), _p(grad_weight), _p(grad_x), F, _p(grad_score), _stream(x)),
            'gather_scale_backward')
    return grad_x, grad_score


def filter_edges(edge_index: Tensor, node_map: Tensor) -> Tuple[Tensor, Tensor]:
    """``pygamd_filter_edges``: ``(edge_index' [2, E'] int64, kept [E'] int64)`` — the edges whose
    two endpoints both map to a non-negative entry of ``node_map [N]`` (int64: the new id or -1),
    relabelled, in the original order, and their edge ids.  The two rows of ``edge_index`` (int32 /
    int64) are read in place at their strides.  The outputs are allocated at ``E`` and narrowed
    after the ONE host read of ``E'``."""
    _require_device(edge_index, node_map)
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"'edge_index' must be [2, E] (got {tuple(edge_index.shape)})")
    node_map = _i64_vector(node_map, 'node_map', node_map.numel())
    E, N = edge_index.size(1), node_map.numel()
    row, col = edge_index[0], edge_index[1]
    if E > 1 and row.stride(0) < 1:   # (a broadcast view)
        row, col = row.contiguous(), col.contiguous()
    stride = max(int(row.stride(0)), 1) if E > 1 else 1
    out = torch.empty(2, E, dtype=torch.int64, device=edge_index.device)
    kept = torch.empty(E, dtype=torch.int64, device=edge_index.device)
    if E == 0:
        return out, kept
    lib = _lib.load()
    total = torch.empty(1, dtype=torch.int64, device=edge_index.device)
    ws, ws_bytes = _workspace(lib.pygamd_filter_edges_workspace_size, (E, ), edge_index.device)
    with _timed({'kind': 'pool', 'op': 'filter_edges', 'E': E, 'N': N}, edge_index):
        check(lib.pygamd_filter_edges(
            _p(row), stride, _p(col), stride, _idx_dtype(edge_index), E, _p(node_map), N,
            _p(out[0]), _p(out[1]), _p(kept), _p(total), _p(ws), ws_bytes, _stream(edge_index)),
            'filter_edges')
    n_kept = int(total.item())
    return out[:, :n_kept], kept[:n_kept]
