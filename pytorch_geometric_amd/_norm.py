"""Host side of the per-graph normalisation layers (``nn.norm.GraphNorm``, ``nn.norm.LayerNorm``
with ``mode='graph'``): the cached by-graph handle of a ``batch`` vector, the route decision and
the generic route.

The fused route (csrc/graph_norm.hip through :class:`_functions.GraphNormFunction`) walks the
graphs of a NON-DECREASING batch vector as contiguous row ranges.  Its handle is ``ptr =
index2ptr(batch)`` plus the hub plan over ``ptr`` at this kernel's threshold and chunk; it is built
once per batch tensor (keyed on identity and ``_version``), together with the verdict on the order
and the one read of ``batch.max()`` that ``batch_size=None`` costs in the reference, so every norm
layer of a step shares it.  ``batch=None`` is one graph of all rows: ``ptr = [0, N]``, a single hub
graph whose plan is known without any read.

The generic route restates the reference's arithmetic (graph_norm.py:72-76, layer_norm.py:82-108)
over this package's ``scatter`` and gather for float32 device tensors and over plain torch for
everything else (host tensors, other dtypes)."""
import weakref
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _native

_LOW = (torch.float16, torch.bfloat16)
MAX_CACHE_ENTRIES = 64


class BatchHandle(NamedTuple):
    ptr: Optional[Tensor]     # [batch_size + 1] at the batch vector's dtype; None: not sorted
    hub: Optional[_native.HubPlan]
    batch_size: int
    is_sorted: bool


_cache = {}
_single = {}


def single_graph_handle(n: int, device) -> BatchHandle:
    """``batch=None``: one graph of ``n`` rows.  The plan of ``ptr = [0, n]`` needs no read."""
    key = (int(n), str(device))
    hit = _single.get(key)
    if hit is not None:
        return hit
    ptr = torch.tensor([0, n], dtype=torch.int64, device=device)
    th, ch = _native.GRAPH_NORM_THRESHOLD, _native.GRAPH_NORM_CHUNK
    if n > th:
        n_chunks = -(-n // ch)
        hub = _native.HubPlan(torch.zeros(1, dtype=torch.int64, device=device),
                              torch.tensor([0, n_chunks], dtype=torch.int64, device=device), 1,
                              n_chunks, th, ch)
    else:
        hub = _native.no_hubs(th, ch)
    if len(_single) >= MAX_CACHE_ENTRIES:
        _single.pop(next(iter(_single)))
    _single[key] = handle = BatchHandle(ptr, hub, 1, True)
    return handle


def _build(batch: Tensor, batch_size: Optional[int]) -> BatchHandle:
    n = batch.numel()
    if n == 0:
        size = 0 if batch_size is None else int(batch_size)
        ptr = torch.zeros(size + 1, dtype=batch.dtype, device=batch.device)
        return BatchHandle(ptr, _native.no_hubs(_native.GRAPH_NORM_THRESHOLD,
                                                _native.GRAPH_NORM_CHUNK), size, True)
    # ONE read: the order's verdict, the first and the largest graph id
    falls = (batch[1:] < batch[:-1]).any().to(batch.dtype)
    unsorted, first, top = torch.stack([falls, batch[0], batch.max()]).tolist()
    size = top + 1 if batch_size is None else int(batch_size)
    if unsorted or first < 0 or top >= size:
        return BatchHandle(None, None, size, False)
    ptr = _native.index2ptr(batch.contiguous(), size)
    return BatchHandle(ptr, _native.graph_norm_plan(ptr), size, True)


def batch_handle(batch: Tensor, batch_size: Optional[int]) -> BatchHandle:
    """The cached :class:`BatchHandle` of a device ``batch`` vector (int32 / int64)."""
    key = (id(batch), None if batch_size is None else int(batch_size))
    hit = _cache.get(key)
    if hit is not None and hit[0]() is batch and hit[1] == batch._version:
        return hit[2]
    handle = _build(batch, batch_size)
    if len(_cache) >= MAX_CACHE_ENTRIES:
        _cache.pop(next(iter(_cache)))

    def _drop(_, key=key, cache=_cache):   # (bound now: module globals are gone at shutdown)
        cache.pop(key, None)

    _cache[key] = (weakref.ref(batch, _drop), batch._version, handle)
    return handle


def clear_cache():
    _cache.clear()
    _single.clear()


def fusable(x: Tensor, batch: Optional[Tensor], fuse: bool) -> bool:
    """The fused route's conditions that need no read: a float device ``x [N, F]`` with ``F <=
    512`` and an int32 / int64 device ``batch`` (or none)."""
    if not (fuse and isinstance(x, Tensor) and x.is_cuda and x.dim() == 2
            and x.dtype in (torch.float32, ) + _LOW and 1 <= x.size(1) <= 512):
        return False
    if batch is None:
        return True
    return (batch.is_cuda and batch.dim() == 1 and batch.numel() == x.size(0)
            and batch.dtype in (torch.int32, torch.int64))


def fused(x: Tensor, batch: Optional[Tensor], batch_size: Optional[int], weight, bias,
          mean_scale, eps: float, mode: str) -> Optional[Tensor]:
    """The fused route, or None when the batch vector turns out not to be sorted.  ``mode``:
    ``'channel'`` (GraphNorm) or ``'graph'`` (LayerNorm over whole graphs)."""
    from ._functions import GraphNormFunction
    if batch is None:
        handle = single_graph_handle(x.size(0), x.device)
    else:
        handle = batch_handle(batch, batch_size)
        if not handle.is_sorted:
            return None
    low = x.dtype if x.dtype in _LOW else None
    with torch.autocast('cuda', enabled=False):
        out = GraphNormFunction.apply(
            x.float(), None if weight is None else weight.float(),
            None if bias is None else bias.float(),
            None if mean_scale is None else mean_scale.float(), handle, float(eps), mode,
            mode == 'graph' and batch is None)
    if low is not None and not torch.is_autocast_enabled():
        out = out.to(low)
    return out


# ---- the generic route -------------------------------------------------------------------------
def _native_rows(x: Tensor, index: Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.float32 and index.is_cuda


def _group_sum(src: Tensor, index: Tensor, size: int) -> Tensor:
    if _native_rows(src, index):
        from .utils import scatter
        return scatter(src, index, 0, size, reduce='sum')
    return src.new_zeros((size, ) + src.shape[1:]).index_add_(0, index.long(), src)


def _group_count(index: Tensor, size: int, like: Tensor) -> Tensor:
    return torch.bincount(index.long(), minlength=size).clamp_(min=1).to(like.dtype)


def _select(src: Tensor, index: Tensor) -> Tensor:
    if _native_rows(src, index):
        from ._functions import GatherFunction
        return GatherFunction.apply(src, index, False)
    return src.index_select(0, index.long())


def _batch_size(batch: Tensor, batch_size: Optional[int]) -> int:
    if batch_size is not None:
        return int(batch_size)
    return int(batch.max()) + 1 if batch.numel() > 0 else 0


def graph_norm_generic(x: Tensor, batch: Optional[Tensor], batch_size: Optional[int],
                       weight: Tensor, bias: Tensor, mean_scale: Tensor, eps: float) -> Tensor:
    """graph_norm.py:65-76 of the reference"""
    if batch is None:
        batch = x.new_zeros(x.size(0), dtype=torch.long)
        batch_size = 1
    size = _batch_size(batch, batch_size)
    count = _group_count(batch, size, x).view(-1, 1)
    mean = _group_sum(x, batch, size) / count
    out = x - _select(mean, batch) * mean_scale
    var = _group_sum(out.pow(2), batch, size) / count
    std = _select((var + eps).sqrt(), batch)
    return weight * out / std + bias


def layer_norm_graph_generic(x: Tensor, batch: Optional[Tensor], batch_size: Optional[int],
                             weight: Optional[Tensor], bias: Optional[Tensor],
                             eps: float) -> Tensor:
    """layer_norm.py:86-108 of the reference, ``mode='graph'``"""
    if batch is None:
        x = x - x.mean()
        out = x / (x.std(unbiased=False) + eps)
    else:
        size = _batch_size(batch, batch_size)
        norm = _group_count(batch, size, x).mul_(x.size(-1)).view(-1, 1)
        mean = _group_sum(x, batch, size).sum(dim=-1, keepdim=True) / norm
        x = x - _select(mean, batch)
        var = _group_sum(x * x, batch, size).sum(dim=-1, keepdim=True) / norm
        out = x / _select((var + eps).sqrt(), batch)
    if weight is not None and bias is not None:
        out = out * weight + bias
    return out
