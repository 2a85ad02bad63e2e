"""The geometric searches of point-cloud models — ``fps``, ``knn``, ``knn_graph``, ``radius``,
``radius_graph`` and ``nearest`` — with the arguments, defaults and output layout of
``torch_geometric.nn.pool`` (torch_geometric/nn/pool/__init__.py:41-375, where each only forwards to
``torch.ops.pyg.*``).

Rules, the same on both routes:

* Examples are the runs of a NON-DECREASING batch vector; a search never leaves its example.  A
  batch vector that decreases somewhere (or holds a negative entry, or one past ``batch_size``)
  raises ``ValueError``.
* The squared L2 distance is ``sum_c (x_c - y_c)^2`` in float32 (float64 inputs: float64), summed in
  the difference form, so a point is at distance exactly 0 from itself.  The cosine distance is
  ``1 - x.y / (|x| |y|)``.
* ``knn``: neighbours come ascending by (distance, index of ``x``); ties go to the smaller index.
  An example with fewer than ``k`` candidates returns what it has.
* ``radius``: a neighbour satisfies ``dist2 < r * r`` STRICTLY, with ``r * r`` formed in float32
  (the device rule of torch_cluster as far as it is known here); neighbours come in ascending index
  and at most ``max_num_neighbors`` are kept, the FIRST ones in index order.
* ``fps``: an example of ``n`` points yields ``math.ceil(ratio * n)`` picks, computed on the host in
  double; every step picks the point not picked yet with the largest minimum distance to the picked
  set, ties to the lowest index, so a cloud with duplicate points goes on at distance 0 without
  ever repeating an index.
* Results on non-finite coordinates are not pinned.

Routes: float32 (half and bfloat16 are widened) device tensors with ``1 <= F <= 512`` (``knn``:
``1 <= k <= 64``) run ``csrc/cluster.hip``.  Everything else — host tensors, other dtypes,
``k > 64``, ``F > 512`` — takes a torch fallback that works example by example in bounded chunks of
query rows and never forms an ``M x N`` matrix over the whole batch.

Host synchronisation on the kernel route: none for ``knn`` / ``knn_graph`` / ``nearest`` / ``fps``
without a batch vector; with one, a single read that brings the example sizes and the validity of
the batch vector together.  ``radius`` / ``radius_graph`` read their data-dependent output size
once, together with that validity; only when a batch vector comes WITHOUT ``batch_size`` do they
need a second read before the launch, for the number of examples (the reference reads
``batch.max()`` on the host at the same point).  ``num_workers`` is accepted and ignored.
"""
import math
from typing import List, Optional, Tuple

import torch
from torch import Tensor

_LOW = (torch.float16, torch.bfloat16)
KERNELS = True           # False: every call takes the torch fallback (measurements, tests)
_CHUNK_ELEMS = 1 << 22   # the fallback's bound on chunk rows x candidates x columns


def _rows(x: Tensor) -> Tensor:
    if x.dim() == 1:
        return x.view(-1, 1)
    return x.reshape(x.size(0), -1) if x.dim() > 2 else x


def _widen(x: Tensor) -> Tensor:
    if x.dtype == torch.float64:
        return x
    return x if x.dtype == torch.float32 else x.float()


def _on_kernel(x: Tensor, y: Tensor, k: int = 1) -> bool:
    from ... import _native
    return (KERNELS and x.is_cuda and y.is_cuda and x.dtype in (torch.float32, ) + _LOW
            and y.dtype in (torch.float32, ) + _LOW and x.size(1) == y.size(1)
            and _native.cluster_supported(x.size(1), k))


class _Examples:
    """The examples of a call: pointer vectors (where the points live), their number, and — after
    at most one host read — the example sizes of both sides."""

    def __init__(self, nx: int, ny: int, batch_x: Optional[Tensor], batch_y: Optional[Tensor],
                 batch_size: Optional[int], device):
        self.device, self.flag, self.sizes = device, None, None
        if batch_x is None and batch_y is None:
            self.B = 1
            ar = torch.arange(2, device=device)           # (no host-to-device copy: no sync)
            self.ptr_x, self.ptr_y = ar * nx, ar * ny
            self.sizes = ([nx], [ny])
            return
        ref = batch_x if batch_x is not None else batch_y
        dtype = ref.dtype if ref.dtype in (torch.int32, torch.int64) else torch.int64
        bx = self._vector(batch_x, nx, dtype, ref.device, 'batch_x')
        by = self._vector(batch_y, ny, dtype, ref.device, 'batch_y')
        if batch_size is None or device.type != 'cuda':
            # the one host read: the batch vectors themselves (sizes, count and validity at once)
            host = torch.cat([bx, by]).cpu()
            hx, hy = host[:nx].long(), host[nx:].long()
            top = -1
            for h in (hx, hy):
                if h.numel() > 0:
                    if bool((h[1:] < h[:-1]).any()) or int(h[0]) < 0:
                        raise ValueError("'batch' must be non-decreasing and non-negative")
                    top = max(top, int(h[-1]))
            if batch_size is not None and top >= int(batch_size):
                raise ValueError(f"'batch' holds the example {top}, 'batch_size' is {batch_size}")
            self.B = max(top + 1 if batch_size is None else int(batch_size), 1)
            self.sizes = (torch.bincount(hx, minlength=self.B).tolist(),
                          torch.bincount(hy, minlength=self.B).tolist())
            if device.type != 'cuda':
                self.ptr_x, self.ptr_y = self._host_ptr(self.sizes[0]), self._host_ptr(self.sizes[1])
                return
        else:
            self.B = max(int(batch_size), 1)
            bad = []
            for b in (bx, by):
                if b.numel() > 0:
                    bad += [(b[1:] < b[:-1]).any(), b[0] < 0, b[-1] >= self.B]
            self.flag = torch.stack(bad).any() if bad else None
        from ... import _native
        self.ptr_x = _native.index2ptr(bx.to(device), self.B)
        self.ptr_y = _native.index2ptr(by.to(device), self.B)

    @staticmethod
    def _vector(b, n, dtype, device, name):
        if b is None:
            return torch.zeros(n, dtype=dtype, device=device)
        if b.dim() != 1 or b.numel() != n:
            raise ValueError(f"'{name}' needs one entry per point ({n}), got {tuple(b.shape)}")
        return b.to(dtype)

    @staticmethod
    def _host_ptr(sizes: List[int]) -> Tensor:
        return torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)

    def check(self, *more: Tensor) -> List[int]:
        """Raise for an invalid batch vector; ONE host read that also brings ``more`` (integer
        device scalars / vectors), returned as a flat list."""
        if self.flag is None and not more:
            return []
        parts = [self.flag.view(1).long()] if self.flag is not None else []
        vals = torch.cat(parts + [m.reshape(-1).long() for m in more]).tolist()
        if self.flag is not None:
            if vals[0]:
                raise ValueError("'batch' must be non-decreasing, non-negative and below "
                                 "'batch_size'")
            self.flag, vals = None, vals[1:]
        return vals

    def example_sizes(self) -> Tuple[List[int], List[int]]:
        if self.sizes is None:
            vals = self.check(self.ptr_x, self.ptr_y)
            px, py = vals[:self.B + 1], vals[self.B + 1:]
            self.sizes = ([px[i + 1] - px[i] for i in range(self.B)],
                          [py[i + 1] - py[i] for i in range(self.B)])
        return self.sizes


def _compact(index: Tensor, count: Tensor, total: int, width: int) -> Tuple[Tensor, Tensor]:
    """``(row, col)`` of the first ``count[q]`` entries of every row of a padded ``[M, width]``
    table, ``total`` of them in all — no host read."""
    M = index.size(0)
    rows = torch.arange(M, device=index.device)
    if total == M * width:
        return rows[:, None].expand(M, width).reshape(-1), index.reshape(-1)
    count = count.long()
    row = torch.repeat_interleave(rows, count, output_size=total)
    first = count.cumsum(0) - count
    pos = torch.arange(total, device=index.device) - first[row]
    return row, index[row, pos]


def _dist(xe: Tensor, yc: Tensor, cosine: bool) -> Tensor:
    """``[c, n]`` distances of the query rows ``yc`` to the candidate rows ``xe``."""
    if cosine:
        dot = (yc[:, None, :] * xe[None, :, :]).sum(-1)
        return 1 - dot / ((yc * yc).sum(-1).sqrt()[:, None] * (xe * xe).sum(-1).sqrt()[None, :])
    diff = yc[:, None, :] - xe[None, :, :]
    return (diff * diff).sum(-1)


def _chunks(n_query: int, n_cand: int, F: int):
    step = max(1, _CHUNK_ELEMS // max(n_cand * max(F, 1), 1))
    for c0 in range(0, n_query, step):
        yield c0, min(c0 + step, n_query)


def _fallback_search(x: Tensor, y: Tensor, ex: _Examples, exclude: bool, select):
    """Example by example, in chunks of query rows: ``select(dist [c, n]) -> (local row, local
    col)`` of the kept pairs, in output order."""
    x, y = _widen(x), _widen(y)
    if x.dtype != y.dtype:
        x, y = x.double(), y.double()
    sx, sy = ex.example_sizes()
    rows, cols = [], []
    xb = yb = 0
    for nx, ny in zip(sx, sy):
        if nx > 0 and ny > 0:
            xe = x[xb:xb + nx]
            for c0, c1 in _chunks(ny, nx, x.size(1)):
                d = _dist(xe, y[yb + c0:yb + c1], select.cosine)
                if exclude:   # the candidate whose global row index is the query's
                    own = torch.arange(yb + c0, yb + c1, device=d.device) - xb
                    hit = (own >= 0) & (own < nx)
                    keep = torch.ones_like(d, dtype=torch.bool)
                    keep[hit.nonzero().view(-1), own[hit]] = False
                else:
                    keep = None
                r, c = select(d, keep)
                rows.append(r + (yb + c0))
                cols.append(c + xb)
        xb, yb = xb + nx, yb + ny
    if not rows:
        empty = torch.empty(0, dtype=torch.int64, device=y.device)
        return empty, empty.clone()
    return torch.cat(rows), torch.cat(cols)


class _SelectK:
    def __init__(self, k: int, cosine: bool):
        self.k, self.cosine = k, cosine

    def __call__(self, d: Tensor, keep: Optional[Tensor]):
        # a stable sort pins the (distance, index) order that topk leaves open among ties
        order = torch.sort(d, dim=1, stable=True).indices
        if keep is not None:
            kept = keep.gather(1, order)
            # stable again: kept entries first, their (distance, index) order unchanged
            order = order.gather(1, torch.sort((~kept).to(torch.int8), dim=1, stable=True).indices)
            n = keep.sum(1)
        else:
            n = torch.full((d.size(0), ), d.size(1), dtype=torch.int64, device=d.device)
        cnt = n.clamp(max=self.k)
        width = min(self.k, d.size(1))
        take = torch.arange(width, device=d.device)[None, :] < cnt[:, None]
        r = torch.arange(d.size(0), device=d.device)[:, None].expand(-1, width)
        return r[take], order[:, :width][take]


class _SelectRadius:
    cosine = False

    def __init__(self, r: float, cap: int):
        self.r2 = float(torch.tensor(float(r), dtype=torch.float32).square())
        self.cap = cap

    def __call__(self, d: Tensor, keep: Optional[Tensor]):
        inside = d < self.r2
        if keep is not None:
            inside &= keep
        inside &= inside.cumsum(1) <= self.cap
        r, c = inside.nonzero(as_tuple=True)   # row-major: by query, ascending index
        return r, c


def _knn_pairs(x: Tensor, y: Tensor, k: int, batch_x, batch_y, cosine: bool,
               batch_size: Optional[int], exclude: bool) -> Tuple[Tensor, Tensor]:
    x, y = _rows(x), _rows(y)
    k = int(k)
    if k < 1:
        raise ValueError(f"'k' must be positive (got {k})")
    if x.size(1) != y.size(1):
        raise ValueError(f"'x' and 'y' differ in width ({x.size(1)} and {y.size(1)})")
    if batch_x is not None and batch_x.device != x.device:
        batch_x = batch_x.to(x.device)
    if batch_y is not None and batch_y.device != y.device:
        batch_y = batch_y.to(y.device)
    ex = _Examples(x.size(0), y.size(0), batch_x, batch_y, batch_size, y.device)
    if not _on_kernel(x, y, k):
        return _fallback_search(x, y, ex, exclude, _SelectK(k, cosine))
    from ... import _native
    sx, sy = ex.example_sizes()
    drop = 1 if exclude else 0
    total = sum(ny * min(k, max(nx - drop, 0)) for nx, ny in zip(sx, sy))
    index, count = _native.knn(_widen(x), _widen(y), ex.ptr_x, ex.ptr_y, k, cosine, exclude)
    return _compact(index, count, total, k)


def knn(x: Tensor, y: Tensor, k: int, batch_x: Optional[Tensor] = None,
        batch_y: Optional[Tensor] = None, cosine: bool = False, num_workers: int = 1,
        batch_size: Optional[int] = None) -> Tensor:
    r"""For each row of ``y`` the ``k`` nearest rows of ``x`` of the same example: ``[2, E]`` with the
    ``y`` index in row 0 and the ``x`` index in row 1, sorted by ``y`` and, per ``y``, ascending by
    (distance, ``x`` index)."""
    row, col = _knn_pairs(x, y, k, batch_x, batch_y, cosine, batch_size, False)
    return torch.stack([row, col])


def knn_graph(x: Tensor, k: int, batch: Optional[Tensor] = None, loop: bool = False,
              flow: str = 'source_to_target', cosine: bool = False, num_workers: int = 1,
              batch_size: Optional[int] = None) -> Tensor:
    r"""The edges to the ``k`` nearest points of every point.  ``loop=False`` excludes the point
    itself BY INDEX inside the search.  The reference asks for ``k + 1`` neighbours and masks
    ``row != col``; the two agree whenever a point is among its own ``k + 1`` nearest, which holds
    for every input without duplicate points."""
    assert flow in ['source_to_target', 'target_to_source']
    row, col = _knn_pairs(x, x, k, batch, batch, cosine, batch_size, not loop)
    return torch.stack([col, row] if flow == 'source_to_target' else [row, col])


def nearest(x: Tensor, y: Tensor, batch_x: Optional[Tensor] = None,
            batch_y: Optional[Tensor] = None) -> Tensor:
    r"""For each row of ``x`` the nearest row of ``y`` of the same example (``knn`` with ``k = 1``,
    roles as in torch_cluster's ``nearest``): ``[x.size(0)]`` indices into ``y``."""
    row, col = _knn_pairs(y, x, 1, batch_y, batch_x, False, None, False)
    out = torch.full((_rows(x).size(0), ), -1, dtype=torch.int64, device=x.device)
    out[row] = col
    return out


def _radius_pairs(x: Tensor, y: Tensor, r: float, batch_x, batch_y, max_num_neighbors: int,
                  batch_size: Optional[int], exclude: bool) -> Tuple[Tensor, Tensor]:
    x, y = _rows(x), _rows(y)
    cap = int(max_num_neighbors)
    if cap < 1:
        raise ValueError(f"'max_num_neighbors' must be positive (got {cap})")
    if not float(r) >= 0:
        raise ValueError(f"'r' must be non-negative (got {r})")
    if x.size(1) != y.size(1):
        raise ValueError(f"'x' and 'y' differ in width ({x.size(1)} and {y.size(1)})")
    if batch_x is not None and batch_x.device != x.device:
        batch_x = batch_x.to(x.device)
    if batch_y is not None and batch_y.device != y.device:
        batch_y = batch_y.to(y.device)
    ex = _Examples(x.size(0), y.size(0), batch_x, batch_y, batch_size, y.device)
    if not _on_kernel(x, y):
        return _fallback_search(x, y, ex, exclude, _SelectRadius(r, cap))
    from ... import _native
    index, count = _native.radius(_widen(x), _widen(y), ex.ptr_x, ex.ptr_y, float(r), cap, exclude)
    total = ex.check(count.sum())[0]   # the one read: the output size, with the batch's validity
    return _compact(index, count, total, cap)


def radius(x: Tensor, y: Tensor, r: float, batch_x: Optional[Tensor] = None,
           batch_y: Optional[Tensor] = None, max_num_neighbors: int = 32, num_workers: int = 1,
           batch_size: Optional[int] = None) -> Tensor:
    r"""For each row of ``y`` the rows of ``x`` of the same example with ``|x - y|^2 < r * r``
    (strict, ``r * r`` in float32), ascending by ``x`` index, at most ``max_num_neighbors`` — the
    first ones in index order: ``[2, E]``, the ``y`` index in row 0, the ``x`` index in row 1."""
    row, col = _radius_pairs(x, y, r, batch_x, batch_y, max_num_neighbors, batch_size, False)
    return torch.stack([row, col])


def radius_graph(x: Tensor, r: float, batch: Optional[Tensor] = None, loop: bool = False,
                 max_num_neighbors: int = 32, flow: str = 'source_to_target',
                 num_workers: int = 1, batch_size: Optional[int] = None) -> Tensor:
    r"""The edges to all points within distance ``r`` (the rule of :func:`radius`);
    ``loop=False`` leaves the point itself out by index, before the cap is applied."""
    assert flow in ['source_to_target', 'target_to_source']
    row, col = _radius_pairs(x, x, r, batch, batch, max_num_neighbors, batch_size, not loop)
    return torch.stack([col, row] if flow == 'source_to_target' else [row, col])


def _fps_host(x: Tensor, sizes: List[int], picks: List[int], start: Tensor) -> Tensor:
    x = _widen(x)
    out = []
    base = 0
    for e, (n, m) in enumerate(zip(sizes, picks)):
        if m > 0:
            pts = x[base:base + n]
            md = torch.full((n, ), float('inf'), dtype=pts.dtype, device=x.device)
            last = start[e] - base
            chosen = torch.empty(m, dtype=torch.int64, device=x.device)
            for it in range(m):
                chosen[it] = last
                if it + 1 == m:
                    break
                diff = pts - pts[last]
                md = torch.minimum(md, (diff * diff).sum(-1))
                md[last] = -1                      # never again: duplicates go on at distance 0
                # the first (lowest) index among the maxima
                last = (md == md.max()).to(torch.uint8).argmax(dim=0)
            out.append(chosen + base)
        base += n
    if not out:
        return torch.empty(0, dtype=torch.int64, device=x.device)
    return torch.cat(out)


def fps(x: Tensor, batch: Optional[Tensor] = None, ratio: float = 0.5,
        random_start: bool = True, batch_size: Optional[int] = None) -> Tensor:
    r"""Farthest point sampling: the global row indices of the picks, grouped by example, in
    selection order.  An example of ``n`` points yields ``math.ceil(ratio * n)`` picks (host
    arithmetic in double; ``0 < ratio <= 1``).  The first pick is row 0 of the example for
    ``random_start=False``, otherwise drawn with ``torch.randint`` under torch's generator of the
    device ``x`` lives on."""
    src = _rows(x)
    ratio = float(ratio)
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"'ratio' must lie in (0, 1] (got {ratio})")
    N, dev = src.size(0), src.device
    if batch is not None and batch.device != dev:
        batch = batch.to(dev)
    ex = _Examples(N, 0, batch, None if batch is None else batch[:0], batch_size, dev)
    sizes = ex.example_sizes()[0]
    picks = [math.ceil(ratio * n) for n in sizes]
    total = sum(picks)
    ptr = ex.ptr_x
    # the same double arithmetic where the pointer lives (no host-to-device copy)
    per = torch.ceil(ratio * (ptr[1:] - ptr[:-1]).double()).to(ptr.dtype)
    out_ptr = torch.cat([per.new_zeros(1), per.cumsum(0).to(ptr.dtype)])
    start = ptr[:-1]
    if random_start:
        span = (ptr[1:] - ptr[:-1]).clamp(min=1)
        draw = torch.randint(0, 1 << 30, (len(sizes), ), device=dev).to(ptr.dtype)
        start = start + draw % span
    if total == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    if not _on_kernel(src, src):
        return _fps_host(src, sizes, picks, start)
    from ... import _native
    return _native.fps(_widen(src), ptr, out_ptr, start.contiguous(), total)


__all__ = ['fps', 'knn', 'knn_graph', 'radius', 'radius_graph', 'nearest']
