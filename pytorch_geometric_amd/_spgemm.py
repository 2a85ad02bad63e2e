"""Host side of the sparse-sparse product ``C = A @ B`` (csrc/spgemm.hip): the route switch, the
test of what the kernels take, and the generic expression (the reference's: ``torch.sparse``).

``PYGAMD_FUSE_SPGEMM`` (read at import): ``0`` / ``1`` start ``GraphUNet.fuse`` and the keyword
``fuse`` of ``EdgeIndex.matmul(EdgeIndex)`` with the kernels off / on.  Unset, they start with
``DEFAULT`` (profiles/spgemm.md)."""
import os
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native

_SWITCH = os.environ.get('PYGAMD_FUSE_SPGEMM')
FUSE_SPGEMM = None if _SWITCH is None else _SWITCH.strip() not in ('', '0')
# the kernels are the one route whose result is fixed bit for bit and whose memory is bounded by
# the long rows' products (profiles/spgemm.md)
DEFAULT = True


def fuse_default() -> bool:
    return DEFAULT if FUSE_SPGEMM is None else FUSE_SPGEMM


def eligible(index: Tensor, N: int, *values: Optional[Tensor]) -> bool:
    """what the kernels take: device tensors, float32 values without a gradient, ``N < 2^31``"""
    if not index.is_cuda or N >= 2 ** 31:
        return False
    return all(v is None or (v.is_cuda and v.dtype == torch.float32 and v.dim() == 1
                             and not v.requires_grad) for v in values)


def generic(row_a: Tensor, col_a: Tensor, val_a: Optional[Tensor], row_b: Tensor, col_b: Tensor,
            val_b: Optional[Tensor], M: int, K: int, N: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``(rowptr_c, col_c, val_c)`` of the product of two COO lists through ``torch.sparse``
    (duplicates are summed, rows ascending, columns ascending per row)."""
    dtype = next((v.dtype for v in (val_a, val_b) if v is not None), torch.float32)

    def coo(row, col, val, size):
        val = torch.ones(row.numel(), dtype=dtype, device=row.device) if val is None else val
        return torch.sparse_coo_tensor(torch.stack([row.long(), col.long()]), val.to(dtype),
                                       size).coalesce()

    out = torch.sparse.mm(coo(row_a, col_a, val_a, (M, K)), coo(row_b, col_b, val_b, (K, N)))
    out = out.coalesce()
    index = out.indices()
    rowptr = torch._convert_indices_from_coo_to_csr(index[0], M).to(row_a.dtype)
    return rowptr, index[1].to(row_a.dtype), out.values()


def ptr2index(rowptr: Tensor, nnz: int) -> Tensor:
    if rowptr.is_cuda:
        return _native.ptr2index(rowptr, nnz)
    rows = torch.arange(rowptr.numel() - 1, dtype=rowptr.dtype)
    return torch.repeat_interleave(rows, rowptr.diff().long(), output_size=nnz)
