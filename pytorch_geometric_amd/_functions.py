"""Autograd glue: each ``torch.autograd.Function`` pairs one forward HIP kernel with the HIP kernels
of its backward.  Formulas follow the reference's CPU path (see the docstrings for file:line)."""
import collections
import os
from typing import Optional

import torch
from torch import Tensor
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native, _onepass
from ._onepass import Slots, _rows, pna_coefficients  # noqa: F401 (kept importable from here)
from .edge_index import EdgeIndex


def _shaped(out2d: Tensor, shape) -> Tensor:
    """The freshly allocated 2-D kernel output under its public shape WITHOUT making it a view:
    autograd forbids in-place edits of views returned by a custom Function, and the reference does
    edit such outputs in place (``deg.pow_(-0.5)`` on a ``scatter`` result, gcn_conv.py:109)."""
    shape = tuple(shape)
    if tuple(out2d.shape) == shape:
        return out2d
    assert out2d.is_contiguous() and out2d._base is None
    return out2d.new_empty(0).set_(out2d.untyped_storage(), out2d.storage_offset(), shape)


class SpmmFunction(Function):
    r"""``out[i] = reduce_{(j -> i)} w_e * x[j]`` on an :class:`EdgeIndex` handle.

    Forward = fused gather/message/reduce of ``MessagePassing.propagate``
    (nn/conv/message_passing.py:421-563; utils/_spmm.py:12-136).  Backward w.r.t. ``x`` = the same
    kernel on the transposed handle (edge_index.py:1849-1900); w.r.t. ``w`` = SDDMM
    (edge_index.py:1903-1922).  ``w_order``: 'coo' (``w[e]`` follows ``edge_index`` order) or
    'slot' (``w`` follows the by-destination slot order, e.g. GAT's alpha).
    """

    @staticmethod
    def forward(ctx, x: Tensor, w: Optional[Tensor], graph: EdgeIndex, reduce: str,
                w_order: str):
        fwd = graph.by_dst()
        if x.size(0) != graph.num_src_nodes:
            raise ValueError(f"'x' has {x.size(0)} rows but the graph has "
                             f"{graph.num_src_nodes} source nodes")
        ctx.graph, ctx.reduce, ctx.w_order = graph, reduce, w_order
        ctx.x_shape = x.shape
        x2 = _rows(x)
        if reduce in ('min', 'max'):
            if w is not None:
                raise NotImplementedError("edge weights are not supported for min/max")
            # the forward also leaves, per output, WHICH slot attained the extremum (int32) or a
            # "split" mark: the backward then needs no edge pass for the unique extrema
            save = ctx.needs_input_grad[0] and not torch.are_deterministic_algorithms_enabled()
            if save:
                out, arg32 = _native.spmm_csr(fwd.ptr, fwd.idx, x2, reduce, n_rows=fwd.n_rows,
                                              hub=fwd.hub, save_arg32=True)
            else:
                out, arg32 = _native.spmm_csr(fwd.ptr, fwd.idx, x2, reduce, n_rows=fwd.n_rows,
                                              hub=fwd.hub), None
            # (the RETURNED tensor is saved, not its 2-D alias: autograd's version check then sees an
            # in-place edit of the result between forward and backward)
            res = _shaped(out, (fwd.n_rows, *x.shape[1:]))
            ctx.save_for_backward(x2, res, arg32)
            return res
        else:
            eid = fwd.perm if (w is not None and w_order == 'coo') else None
            out = _native.spmm_csr(fwd.ptr, fwd.idx, x2, reduce, n_rows=fwd.n_rows, eid=eid, w=w,
                                   hub=fwd.hub)
            need_x = w is not None and ctx.needs_input_grad[1]
            ctx.save_for_backward(x2 if need_x else None, w)
        return _shaped(out, (fwd.n_rows, *x.shape[1:]))

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        graph, reduce = ctx.graph, ctx.reduce
        g2 = _rows(grad_out)
        grad_x = grad_w = None
        if reduce in ('min', 'max'):
            x2, out, arg32 = ctx.saved_tensors
            out = _rows(out)
            if ctx.needs_input_grad[0]:
                fwd = graph.by_dst()
                if torch.are_deterministic_algorithms_enabled():
                    # source-driven, no atomics: fixed summation order, ~3.5x slower
                    bwd = graph.by_src()
                    ntie = _native.spmm_tie_count(fwd.ptr, fwd.idx, x2, out, count_self=True)
                    grad_x = _native.spmm_minmax_backward(bwd.ptr, bwd.idx, x2, out, g2, ntie)
                else:
                    grad_x = None
                    if arg32 is not None and not graph.atomic_backward:
                        # cached graph: winners as per-edge bit masks + a source-driven sum over
                        # the transposed CSR instead of N x F scattered atomics
                        grad_x = _native.spmm_minmax_backward_src(
                            fwd, graph.by_src(), graph.src_slot_to_dst_slot(), x2, out, g2, arg32)
                    if grad_x is None:
                        grad_x = _native.spmm_minmax_backward_dst(fwd.ptr, fwd.idx, x2, out, g2,
                                                                  graph.num_src_nodes,
                                                                  arg32=arg32)
                grad_x = grad_x.view(ctx.x_shape)
            return grad_x, None, None, None, None
        x2, w = ctx.saved_tensors
        fwd = graph.by_dst()
        if reduce == 'mean' and w is not None:
            g2 = g2 * fwd.inv_degree().view(-1, 1)
        if ctx.needs_input_grad[0]:
            scale = fwd.inv_degree() if (reduce == 'mean' and w is None) else None
            if graph.atomic_backward and (w is None or w.dim() == 1 or w.size(1) == 1):
                # graph used once (sampled batch): edge-parallel atomics on the COO list
                # instead of sorting by source (one weight per edge: also a single-head GAT)
                w_coo = w if w is None else w.reshape(-1)
                if w is not None and ctx.w_order == 'slot':
                    w_coo = torch.empty_like(w_coo)
                    w_coo[fwd.perm.long()] = w.reshape(-1)
                ei = graph.edge_index
                grad_x = _native.gather_scatter_add(g2, ei[1], ei[0], graph.num_src_nodes,
                                                    scale=scale, w=w_coo)
            else:
                bwd = graph.by_src()
                eid = None
                if w is not None:
                    eid = bwd.perm if ctx.w_order == 'coo' else graph.src_slot_to_dst_slot()
                grad_x = _native.spmm_csr(bwd.ptr, bwd.idx, g2, 'sum', n_rows=bwd.n_rows,
                                          eid=eid, w=w, src_scale=scale, hub=bwd.hub)
            grad_x = grad_x.view(ctx.x_shape)
        if w is not None and ctx.needs_input_grad[1]:
            eid = fwd.perm if ctx.w_order == 'coo' else None
            heads = 1 if w.dim() == 1 else w.size(1)
            grad_w = _native.sddmm_csr(fwd.ptr, fwd.idx, eid, g2, x2, fwd.nnz, heads)
            grad_w = grad_w.view(w.shape)
        return grad_x, grad_w, None, None, None


# ---- large unsorted scatters: sort once, then a segment reduction ---------------------------------
# The atomic scatter kernels move a cache line per 4-byte atomic: at the products shape
# (E = 61.9 M rows of 256 floats) `scatter(msg, edge_index[1])` takes 206 ms = 0.04 of the HBM peak,
# 311 ms for max (profiles/r04_unfused_propagate.md).  One stable radix sort of the index (a few ms,
# cached per index tensor) turns the same call into a gather-SpMM over the sorted groups
# (`col` = the sort permutation): 11.5 ms, deterministic.  Small inputs keep the atomics.
#
# Who takes the sorted route:
#   * an index of >= SORTED_SCATTER_ALWAYS_ROWS entries always: the sort costs a small fraction of
#     what the atomics cost there, even for an index tensor that is never seen again;
#   * a smaller one (>= SORTED_SCATTER_MIN_ROWS) only when the same tensor (identity + version) has
#     been seen before, or when it is a row of an `EdgeIndex` handle — a sampled batch's fresh
#     index keeps the atomics instead of paying a sort it never amortises.
# Building a plan reads nothing back to the host: `pygamd_index_guard` folds every out-of-range
# entry into a sentinel group behind the last real one (skipped, as the atomic kernels skip such
# rows) and raises the launch's error flag, which travels as PYGAMD_CHECK_INDEX says (async: flag
# ring; sync: one blocking read; off: nothing).  The hub split plan (one host read) is added the
# first time a cached plan is REUSED.  Plans are int32 whenever the sizes fit and the cache is
# bounded in BYTES (PYGAMD_SCATTER_PLAN_BYTES, default 1 GiB; a plan at the products shape is
# 0.26 GB), oldest out first; an entry also dies with its index tensor.
SORTED_SCATTER_MIN_ROWS = 1 << 16
SORTED_SCATTER_MIN_ELEMS = 1 << 23
SORTED_SCATTER_ALWAYS_ROWS = 1 << 20
SCATTER_PLAN_CACHE_BYTES = int(os.environ.get('PYGAMD_SCATTER_PLAN_BYTES', str(1 << 30)))
SCATTER_SEEN_ENTRIES = 64
_scatter_plans = collections.OrderedDict()  # key -> [weakref(base), version, plan, nbytes, hub?, oob]
_scatter_seen = collections.OrderedDict()   # key -> (weakref(base), version): met once, no plan
_INT32_MAX = (1 << 31) - 1


def _index_key(index: Tensor, dim_size: int):
    """Identity of an index tensor: the tensor it views (``edge_index[1]`` is a new view object on
    every call) + where in it + its version counter."""
    base = index._base if index._base is not None else index
    return base, (id(base), index.storage_offset(), index.numel(), index.stride(0), index.dtype,
                  int(dim_size))


def _build_scatter_plan(index: Tensor, dim_size: int, oob: list):
    """``oob``: a one-element list the flag ring sets to True when the guard's flag arrives
    raised — a CACHED plan then re-reports its out-of-range entries on every later hit (the
    kernels skip such rows either way; without the marker only the first use would say so)."""
    n = index.numel()
    small = n < _INT32_MAX and dim_size + 1 < _INT32_MAX
    ring, slot, err = _native._index_flag(index.device, True)
    keys = _native.index_guard(index, dim_size, err,
                               dtype=torch.int32 if small else torch.int64)

    def mark():
        oob[0] = True

    _native._index_flag_done(ring, slot, err, 'scatter', dim_size, index, on_flag=mark)
    sorted_keys, perm = _native.index_sort(keys, max_value=dim_size)
    # group `dim_size` = the out-of-range entries: it has a pointer entry and no output row
    ptr = _native.index2ptr(sorted_keys, dim_size + 1)[:dim_size + 1]
    if perm.dtype != ptr.dtype:
        perm = _native.cast_index(perm, ptr.dtype)
    return ptr, perm


def _plan_bytes(ptr: Tensor, perm: Tensor) -> int:
    return ptr.numel() * ptr.element_size() + perm.numel() * perm.element_size()


def _sorted_scatter_plan(index: Tensor, dim_size: int, force: bool = True):
    """(ptr [dim_size + 1], perm [n], hub) for ``index``, or None when the rule above leaves this
    call to the atomic kernels (``force=False`` and a first sighting)."""
    import weakref
    base, key = _index_key(index, dim_size)
    hit = _scatter_plans.get(key)
    if hit is not None and hit[0]() is base and hit[1] == index._version:
        _scatter_plans.move_to_end(key)
        if hit[5][0] and _native.INDEX_CHECK != 'off':  # known bad since an earlier use: say so
            _native._raise_out_of_range(index, dim_size, 'scatter',   # again, at the call
                                        _native._error_style.value)
        if not hit[4]:  # reused: now the hub split pays (one host read, once)
            ptr, perm, _ = hit[2]
            hit[2], hit[4] = (ptr, perm, _native.hub_plan(ptr)), True
        return hit[2]
    if hit is not None:
        _scatter_plans.pop(key, None)
    if not force and not isinstance(base, EdgeIndex):
        seen = _scatter_seen.get(key)
        if seen is None or seen[0]() is not base or seen[1] != index._version:
            _scatter_seen[key] = (weakref.ref(base, lambda _, k=key: _scatter_seen.pop(k, None)),
                                  index._version)
            while len(_scatter_seen) > SCATTER_SEEN_ENTRIES:
                _scatter_seen.popitem(last=False)
            return None
    _scatter_seen.pop(key, None)
    oob = [False]
    ptr, perm = _build_scatter_plan(index, dim_size, oob)
    plan = (ptr, perm, None)
    nbytes = _plan_bytes(ptr, perm)
    if nbytes <= SCATTER_PLAN_CACHE_BYTES:
        held = sum(e[3] for e in _scatter_plans.values())
        while _scatter_plans and held + nbytes > SCATTER_PLAN_CACHE_BYTES:
            held -= _scatter_plans.popitem(last=False)[1][3]
        _scatter_plans[key] = [weakref.ref(base, lambda _, k=key: _scatter_plans.pop(k, None)),
                               index._version, plan, nbytes, False, oob]
    return plan


def _use_sorted_scatter(rows: Tensor, index: Tensor, reduce: str) -> bool:
    return (reduce in ('sum', 'mean', 'min', 'max') and index.numel() >= SORTED_SCATTER_MIN_ROWS
            and rows.numel() >= SORTED_SCATTER_MIN_ELEMS and rows.dtype == torch.float32
            and not torch.cuda.is_current_stream_capturing())


def _scatter_rows_auto(rows: Tensor, index: Tensor, dim_size: int, reduce: str,
                       return_count: bool = False):
    """`_native.scatter_rows` semantics; large inputs through the sorted route."""
    plan = None
    if _use_sorted_scatter(rows, index, reduce):
        plan = _sorted_scatter_plan(index, dim_size,
                                    force=index.numel() >= SORTED_SCATTER_ALWAYS_ROWS)
    if plan is None:
        return _native.scatter_rows(rows, index, dim_size, reduce, return_count=return_count)
    ptr, perm, hub = plan
    out = _native.spmm_csr(ptr, perm, rows, reduce, n_rows=dim_size, hub=hub)
    if return_count:
        return out, (ptr[1:] - ptr[:-1]).to(torch.float32)
    return out


class GatherFunction(Function):
    """``x.index_select(0, index)`` (message_passing.py:263-290); backward = scatter-add."""

    @staticmethod
    def forward(ctx, x: Tensor, index: Tensor, check_bounds: bool):
        ctx.save_for_backward(index)
        ctx.x_shape = x.shape
        out = _native.gather_rows(_rows(x), index, check_bounds)
        return _shaped(out, (index.numel(), *x.shape[1:]))

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        (index,) = ctx.saved_tensors
        g = _scatter_rows_auto(_rows(grad_out), index, ctx.x_shape[0], 'sum')
        return g.view(ctx.x_shape), None, None


class ScatterFunction(Function):
    """``scatter(src, index, 0, dim_size, reduce)`` on an unsorted index (utils/_scatter.py)."""

    @staticmethod
    def forward(ctx, src: Tensor, index: Tensor, dim_size: int, reduce: str):
        s2 = _rows(src)
        ctx.reduce, ctx.src_shape = reduce, src.shape
        if reduce == 'mean':
            out, count = _scatter_rows_auto(s2, index, dim_size, reduce, return_count=True)
            ctx.save_for_backward(index, count)
        elif reduce in ('min', 'max', 'mul'):
            # the RETURNED tensor is what the backward compares against: saving it (not its 2-D
            # alias) lets autograd detect an in-place edit of the result
            res = _shaped(_scatter_rows_auto(s2, index, dim_size, reduce),
                          (dim_size, *src.shape[1:]))
            ctx.save_for_backward(index, s2, res)
            return res
        else:
            out = _scatter_rows_auto(s2, index, dim_size, reduce)
            ctx.save_for_backward(index)
        return _shaped(out, (dim_size, *src.shape[1:]))

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        reduce = ctx.reduce
        # the forward's index flag has normally arrived by now: raise before gathering with an
        # index the forward found out of range (no wait: INDEX_CHECK='async')
        _native.poll_index_errors()
        g2 = _rows(grad_out)
        if reduce in ('sum', 'add'):
            (index,) = ctx.saved_tensors
            grad = _native.gather_rows(g2, index)
        elif reduce == 'mean':
            index, count = ctx.saved_tensors
            grad = _native.gather_rows(g2 / count.clamp(min=1).view(-1, 1), index)
        elif reduce in ('min', 'max'):
            index, s2, out = ctx.saved_tensors
            grad = _native.scatter_minmax_backward(s2, index, _rows(out), g2)
        elif reduce == 'mul':
            # ATen's scatter_reduce 'prod' backward incl. its zero-count rule (one zero in the
            # group: that element gets g * prod(others); two or more: all 0) — g * out / src alone
            # would be NaN there
            index, s2, out = ctx.saved_tensors
            grad = _native.scatter_mul_backward(s2, index, _rows(out), g2)
        else:
            raise NotImplementedError(f"backward of scatter(reduce='{reduce}') is undefined")
        return grad.view(ctx.src_shape), None, None, None


class MultiReduceFunction(Function):
    """Several reductions of the same grouped rows in ONE read (``pygamd_multi_reduce_csr``; the
    shared work of nn/aggr/fused.py:191-336): returns one ``[dim_size, F]`` tensor per name in
    ``want`` (names from ``sum | pow_sum | min | max``).  ``perm`` is the stable sort permutation
    of ``index`` (``None`` when the rows are already grouped).  Backward composes the existing
    kernels: a gather for ``sum``, ``2 x`` times a gather for ``pow_sum`` (skipped with
    ``semi_grad``), the tie-splitting min / max gradient of the reference."""

    @staticmethod
    def forward(ctx, x: Tensor, index: Tensor, ptr: Tensor, perm: Optional[Tensor], want: tuple,
                semi_grad: bool):
        outs = _native.multi_reduce_csr(ptr, perm, x, want)
        ctx.want, ctx.semi_grad = want, semi_grad
        ctx.save_for_backward(x, index, *[outs[k] for k in want if k in ('min', 'max')])
        return tuple(outs[k] for k in want)

    @staticmethod
    def backward(ctx, *grads):
        x, index, *extrema = ctx.saved_tensors
        extrema = iter(extrema)
        total = None
        for name, g in zip(ctx.want, grads):
            out = next(extrema) if name in ('min', 'max') else None
            if g is None:
                continue
            g = g.contiguous()
            if name == 'sum':
                term = _native.gather_rows(g, index)
            elif name == 'pow_sum':
                if ctx.semi_grad:
                    continue
                term = _native.gather_rows(g, index).mul_(x).mul_(2.0)
            else:
                term = _native.scatter_minmax_backward(x, index, out, g)
            total = term if total is None else total.add_(term)
        return total, None, None, None, None, None


class SegmentFunction(Function):
    """``segment(src, ptr, reduce)`` over contiguous row ranges (utils/_segment.py:11-50).  For
    min / max the reference replaces an INFINITE extremum by 0 (``torch.where(out.isinf(), 0,
    out)``, utils/_segment.py:48-49): a segment of -inf masks, or one holding +inf, gives 0 and
    takes no gradient.  ``_native.spmm_csr`` itself keeps the plain extremum (``scatter`` and the
    graph aggregations return it as is)."""

    @staticmethod
    def forward(ctx, src: Tensor, ptr: Tensor, reduce: str):
        s2 = _rows(src)
        n_seg = ptr.numel() - 1
        out = _native.spmm_csr(ptr, None, s2, reduce, n_rows=n_seg)
        ctx.reduce, ctx.src_shape = reduce, src.shape
        if reduce in ('min', 'max'):
            # the plain extremum is what the backward compares against; the caller sees 0 where
            # it is infinite
            ctx.save_for_backward(ptr, s2, out)
            return _shaped(torch.where(out.isinf(), 0., out), (n_seg, *src.shape[1:]))
        ctx.save_for_backward(ptr)
        return _shaped(out, (n_seg, *src.shape[1:]))

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        reduce = ctx.reduce
        g2 = _rows(grad_out)
        n = ctx.src_shape[0]
        if reduce in ('min', 'max'):
            ptr, s2, out = ctx.saved_tensors
            # (a replaced extremum is a constant: nothing of that segment takes a gradient)
            g2 = torch.where(out.isinf(), 0., g2)
            # ATen's _segment_reduce backward (the reference's CPU path, utils/_segment.py:48)
            # counts as "attaining the extremum" every element equal to it AND every NaN
            # (SegmentReduce.cpp: `at::_isnan(value) || value == output`): a NaN extremum sends
            # its gradient to the NaN elements.
            nan = s2.isnan()
            ntie = _native.spmm_tie_count(ptr, None, s2, out, count_self=False)
            ntie = ntie + _native.spmm_csr(ptr, None, nan.to(s2.dtype), 'sum',
                                           n_rows=out.size(0))
            index = _native.ptr2index(ptr, n)
            # each row belongs to exactly one segment: grad = [src == out[seg]] * g[seg] / ntie[seg]
            o_e = _native.gather_rows(out, index)
            # It averages over the tied extrema ONLY where the incoming gradient is positive
            # (`if (grad_input > 0) grad_input /= counter`); a negative gradient reaches every
            # tied element undivided.  Matched as is.
            g_e = _native.gather_rows(torch.where(g2 > 0, g2 / ntie.clamp(min=1), g2), index)
            grad = torch.where((s2 == o_e) | nan, g_e, torch.zeros_like(g_e))
        else:
            (ptr,) = ctx.saved_tensors
            index = _native.ptr2index(ptr, n)
            if reduce == 'mean':
                cnt = (ptr[1:] - ptr[:-1]).clamp(min=1).to(torch.float32)
                g2 = g2 / cnt.view(-1, 1)
            grad = _native.gather_rows(g2, index)
        return grad.view(ctx.src_shape), None, None


class SegmentSoftmaxFunction(Function):
    """Softmax within ``ptr`` segments (utils/_softmax.py:60-81); the max is taken on the detached
    input, so the backward is the plain softmax Jacobian."""

    @staticmethod
    def forward(ctx, src: Tensor, ptr: Tensor):
        s2 = _rows(src)
        res = _shaped(_native.segment_softmax_forward(s2, ptr), src.shape)
        ctx.save_for_backward(res, ptr)
        ctx.src_shape = src.shape
        return res

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        out, ptr = ctx.saved_tensors
        out = _rows(out)
        g = _native.segment_softmax_backward(out, grad_out.reshape(out.shape), ptr)
        return g.view(ctx.src_shape), None


class IndexSoftmaxFunction(Function):
    """Softmax within the groups of an UNSORTED ``index`` (utils/_softmax.py:82-88: the maximum is
    taken on the detached input, ``1e-16`` joins the denominator) as dedicated kernels instead of
    the six-pass scatter / gather composition; backward = the softmax Jacobian,
    ``out * (g - sum_group(out * g))``."""

    @staticmethod
    def forward(ctx, src: Tensor, index: Tensor, num_groups: int):
        res = _shaped(_native.softmax_index_forward(_rows(src), index, num_groups), src.shape)
        ctx.save_for_backward(res, index)
        ctx.num_groups = num_groups
        return res

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        out, index = ctx.saved_tensors
        o2 = _rows(out)
        g = _native.softmax_index_backward(o2, grad_out.reshape(o2.shape), index, ctx.num_groups)
        return g.view(out.shape), None, None


class SegmentLogSumExpFunction(Function):
    """``segment_logsumexp(src, ptr, dim=0)`` (utils/_segment.py:53-80) for 2-D ``src``; the total
    derivative through the subtracted maximum is the in-segment softmax."""

    @staticmethod
    def forward(ctx, src: Tensor, ptr: Tensor):
        s2 = _rows(src)
        res = _shaped(_native.segment_logsumexp_forward(s2, ptr),
                      (ptr.numel() - 1, *src.shape[1:]))
        ctx.save_for_backward(s2, res, ptr)
        ctx.src_shape = src.shape
        return res

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        s2, out, ptr = ctx.saved_tensors
        g = _native.segment_logsumexp_backward(s2, _rows(out), _rows(grad_out), ptr)
        return g.view(ctx.src_shape), None


class GatEdgeSoftmaxFunction(Function):
    """alpha[k,h] = softmax_row(leaky_relu(alpha_src[col[k],h] + alpha_dst[i,h])) in by-destination
    slot order (nn/conv/gat_conv.py:387-406)."""

    @staticmethod
    def forward(ctx, alpha_src: Tensor, alpha_dst: Tensor, graph: EdgeIndex, slope: float):
        fwd = graph.by_dst()
        alpha = _native.gat_edge_softmax_forward(fwd.ptr, fwd.idx, alpha_src, alpha_dst, slope)
        ctx.save_for_backward(alpha_src, alpha_dst, alpha)
        ctx.graph, ctx.slope = graph, slope
        return alpha

    @staticmethod
    def backward(ctx, grad_alpha: Tensor):
        alpha_src, alpha_dst, alpha = ctx.saved_tensors
        fwd = ctx.graph.by_dst()
        g_src, g_dst = _native.gat_edge_softmax_backward(fwd.ptr, fwd.idx, alpha_src, alpha_dst,
                                                         alpha, grad_alpha, ctx.slope)
        return g_src, g_dst, None, None


# PYGAMD_GAT_FUSED_BWD=0: the SDDMM and the transposed SpMM of the GAT backward as two launches
GAT_FUSED_BACKWARD = os.environ.get('PYGAMD_GAT_FUSED_BWD', '1') != '0'


class GatAttendFunction(Function):
    """One GAT attention + aggregation step on projected features ``x [N, H, C]`` (source and
    destination features are the same tensor): node terms ``(x * att).sum(-1)``, edge logits +
    leaky ReLU + softmax per destination, weighted aggregation (gat_conv.py:330-332, 387-408) —
    the three kernels of HeadDotFunction / GatEdgeSoftmaxFunction / SpmmFunction under ONE
    autograd node, so that the two gradients of ``x`` (through the aggregation and through the
    node terms) meet inside ``head_dot_bwd_kernel`` instead of in a separate add pass."""

    @staticmethod
    def forward(ctx, x: Tensor, att_src: Tensor, att_dst: Tensor, graph: EdgeIndex,
                slope: float, n_dst: int):
        N, H, C = x.shape
        x2 = x.reshape(N, H * C)
        a_src, a_dst = _native.head_dot_forward(x2, att_src.reshape(-1), att_dst.reshape(-1),
                                                H, C)
        fwd = graph.by_dst()
        a_dst = a_dst[:n_dst].contiguous()
        alpha = _native.gat_edge_softmax_forward(fwd.ptr, fwd.idx, a_src, a_dst, slope)
        out = _native.spmm_csr(fwd.ptr, fwd.idx, x2, 'sum', n_rows=fwd.n_rows, w=alpha,
                               hub=fwd.hub)
        ctx.save_for_backward(x2, att_src, att_dst, a_src, a_dst, alpha)
        ctx.graph, ctx.slope, ctx.dims = graph, slope, (N, H, C)
        return out.view(fwd.n_rows, H, C)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        x2, att_src, att_dst, a_src, a_dst, alpha = ctx.saved_tensors
        N, H, C = ctx.dims
        graph = ctx.graph
        fwd, bwd = graph.by_dst(), graph.by_src()
        g2 = _rows(grad_out)
        if GAT_FUSED_BACKWARD:
            # ONE pass over the by-source slots gathers every gradient row once for both
            #   d alpha[k, h] = <grad_out[i, h, :], x[j, h, :]>  (filed under the edge's
            #   destination slot, where the softmax backward reads it) and
            #   d x through the aggregation = sum_i alpha * grad_out[i]
            # (two launches — SDDMM by destination + transposed weighted SpMM — gathered 2 x
            # E rows of H * C floats: 1.39 of config 3's 5.5 ms per step)
            grad_alpha, grad_x = _native.sddmm_spmm_csr(
                bwd.ptr, bwd.idx, graph.src_slot_to_dst_slot(), x2, g2, alpha, fwd.nnz, H)
        else:
            # d x through the aggregation: the same coefficients on the transposed handle
            grad_x = _native.spmm_csr(bwd.ptr, bwd.idx, g2, 'sum', n_rows=bwd.n_rows,
                                      eid=graph.src_slot_to_dst_slot(), w=alpha, hub=bwd.hub)
            # d alpha[k, h] = <grad_out[i, h, :], x[j, h, :]>, then back through the edge softmax
            grad_alpha = _native.sddmm_csr(fwd.ptr, fwd.idx, None, g2, x2, fwd.nnz, H)
        g_src, g_dst = _native.gat_edge_softmax_backward(fwd.ptr, fwd.idx, a_src, a_dst, alpha,
                                                         grad_alpha.view(alpha.shape), ctx.slope)
        if g_dst.size(0) < N:  # destinations are a prefix of the nodes
            pad = g_dst.new_zeros(N, H)
            pad[:g_dst.size(0)] = g_dst
            g_dst = pad
        # d x through the node terms is ADDED to grad_x by the kernel that also reduces d att
        _, g_att_src, g_att_dst = _native.head_dot_backward(
            x2, att_src.reshape(-1), att_dst.reshape(-1), g_src, g_dst, H, C, True,
            accumulate_into=grad_x)
        return (grad_x.view(N, H, C), g_att_src.view(att_src.shape),
                g_att_dst.view(att_dst.shape), None, None, None)


def _check_rows(graph: EdgeIndex, n_dst: int, src_name: str, src: Tensor, dst_name: str,
                dst: Optional[Tensor]):
    """``src``: one row per source of the graph; ``dst`` (None: not given): >= ``n_dst`` rows"""
    if src.size(0) != graph.num_src_nodes:
        raise ValueError(f"'{src_name}' has {src.size(0)} rows but the graph has "
                         f"{graph.num_src_nodes} source nodes")
    if n_dst != graph.num_dst_nodes or (dst is not None and dst.size(0) < n_dst):
        raise ValueError(f"the graph has {graph.num_dst_nodes} destinations: 'n_dst' = {n_dst}, "
                         f"'{dst_name}' has {None if dst is None else dst.size(0)} rows")


def _gatv2_forward(ctx, x_l, x_r, att, graph, slope, n_dst, aggregate):
    """The forward of both GATv2 nodes: ``out [n_dst, H, C]``, or ``alpha`` in the score mode."""
    _, H, C = x_l.shape
    _check_rows(graph, n_dst, 'x_l', x_l, 'x_r', x_r)
    fwd = graph.by_dst()
    xl2, xr2 = x_l.reshape(-1, H * C), x_r.reshape(-1, H * C)
    alpha, out = _native.gatv2_forward(fwd.ptr, fwd.idx, xl2, xr2, att, H, C, slope, hub=fwd.hub,
                                       aggregate=aggregate)
    ctx.save_for_backward(xl2, xr2, att, alpha, *((out, ) if aggregate else ()))
    ctx.graph, ctx.slope, ctx.dims, ctx.att_shape = graph, slope, (H, C), att.shape
    return out.view(fwd.n_rows, H, C) if aggregate else alpha


def _gatv2_backward(ctx, x_l, x_r, att, alpha, **grads):
    """The return tuple of both GATv2 nodes from the flat gradients of the shared body."""
    H, C = ctx.dims
    g_l, g_r, g_att = _onepass.gatv2_backward(
        Slots.of_graph(ctx.graph), x_l, x_r, att, alpha, H, C, ctx.slope,
        want_x_l=ctx.needs_input_grad[0], **grads)
    return (None if g_l is None else g_l.view(-1, H, C), g_r.view(-1, H, C),
            g_att.view(ctx.att_shape), None, None, None)


class Gatv2AttendFunction(Function):
    """One GATv2 attention + aggregation step on projected features ``x_l [N_src, H, C]`` (sources)
    and ``x_r [>= n_dst, H, C]`` (destinations, a prefix): score, softmax per destination and the
    weighted sum of ``x_l`` (gatv2_conv.py:358-378) in ONE pass over the by-destination slots; the
    backward is one pass by destination and one by source (csrc/gatv2.hip).  Saved: the inputs,
    ``alpha [E, H]`` and ``out`` — nothing of size ``E x H*C``."""

    @staticmethod
    def forward(ctx, x_l: Tensor, x_r: Tensor, att: Tensor, graph: EdgeIndex, slope: float,
                n_dst: int):
        return _gatv2_forward(ctx, x_l, x_r, att, graph, slope, n_dst, True)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        xl2, xr2, att, alpha, out = ctx.saved_tensors
        return _gatv2_backward(ctx, xl2, xr2, att, alpha, grad_out=_rows(grad_out), out=out)


class Gatv2ScoreFunction(Function):
    """The attention coefficients of :class:`Gatv2AttendFunction` alone: ``alpha [E, H]`` in
    by-destination slot order, for layers that consume them themselves (dropout on the
    coefficients, ``return_attention_weights``) and aggregate with ``SpmmFunction(..., 'slot')``."""

    @staticmethod
    def forward(ctx, x_l: Tensor, x_r: Tensor, att: Tensor, graph: EdgeIndex, slope: float,
                n_dst: int):
        return _gatv2_forward(ctx, x_l, x_r, att, graph, slope, n_dst, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_alpha: Tensor):
        xl2, xr2, att, alpha = ctx.saved_tensors
        return _gatv2_backward(ctx, xl2, xr2, att, alpha, grad_alpha=grad_alpha.contiguous())


class HanAttendFunction(Function):
    """HAN's node-level attention (han_conv.py:170-179, the 'add' aggregation and, under ``relu``,
    the ReLU of han_conv.py:155) for every edge type of a layer call in ONE pass over the stacked
    by-destination handle ``graph`` (``_han.stacked_graph``): ``x_all [S, H, D]`` holds every node
    type's projected rows once, ``a_src [n_cols, H]`` / ``a_dst [n_rows, H]`` the stacked per-node
    logits, ``types = (row_begin, src_begin, val_shift)`` the stacking plan.  Returns ``out
    [n_rows, H * D]``.  The backward is one pass by destination and one by source (csrc/han.hip).
    Saved: the inputs, ``alpha [E, H]`` and ``out`` — nothing of size ``E x H*D``."""

    @staticmethod
    def forward(ctx, x_all: Tensor, a_src: Tensor, a_dst: Tensor, graph: EdgeIndex, types,
                slope: float, relu: bool):
        _, H, C = x_all.shape
        types = tuple(tuple(int(v) for v in t) for t in types)
        _onepass.han_check_types(types, graph.num_dst_nodes, graph.num_src_nodes, x_all.size(0))
        if a_src.size(0) != graph.num_src_nodes or a_dst.size(0) != graph.num_dst_nodes:
            raise ValueError(f"'a_src' / 'a_dst' need {graph.num_src_nodes} / "
                             f"{graph.num_dst_nodes} rows (got {a_src.size(0)} / {a_dst.size(0)})")
        fwd = graph.by_dst()
        x2 = x_all.reshape(-1, H * C)
        alpha, out = _native.han_forward(fwd.ptr, fwd.idx, types[0], types[2], x2, a_src, a_dst,
                                         H, C, slope, relu, hub=fwd.hub)
        ctx.save_for_backward(x2, a_src, a_dst, alpha, out)
        ctx.graph, ctx.types, ctx.slope, ctx.relu, ctx.dims = graph, types, slope, relu, (H, C)
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor, _grad_alpha):
        x2, a_src, a_dst, alpha, out = ctx.saved_tensors
        H, C = ctx.dims
        g_x, g_src, g_dst = _onepass.han_backward(
            Slots.of_graph(ctx.graph), ctx.types, x2, a_src, a_dst, alpha, out,
            _rows(grad_out).contiguous(), H, C, ctx.slope, ctx.relu,
            want_x=ctx.needs_input_grad[0], want_a_src=ctx.needs_input_grad[1])
        return (None if g_x is None else g_x.view(-1, H, C), g_src, g_dst, None, None, None,
                None)


def _key_value(key: Tensor, value: Optional[Tensor], W: int):
    """``(key, value, packed)`` as ``[N_src, W]`` rows; ``value=None``: the halves of ``key``"""
    if value is None:
        kv = key.reshape(-1, 2 * W)
        return kv[:, :W], kv[:, W:], True
    return key.reshape(-1, W), value.reshape(-1, W), False


def _transformer_backward(ctx, query, key, value, alpha, want_value=False, **kwargs):
    """The shared body's five gradients under the public shapes of the four TransformerConv nodes
    (packed: grad_key is the one ``[N_src, 2, H, C]`` gradient), grad_edge_attr in edge order."""
    H, C = ctx.dims[:2]
    g_q, g_k, g_v, g_b, g_a = _onepass.transformer_backward(
        Slots.of_graph(ctx.graph), query, key, value, alpha, H, C, ctx.scale,
        want_key=ctx.needs_input_grad[1], want_value=want_value, **kwargs)
    return (g_q.view(-1, H, C), None if g_k is None else g_k.view(ctx.key_shape),
            None if g_v is None else g_v.view(ctx.key_shape),
            None if g_b is None else g_b.view(ctx.bias_shape), _edge_unslot(g_a, ctx.graph))


class TransformerAttendFunction(Function):
    """One dot-product attention + aggregation step of TransformerConv on projected features
    ``query [>= n_dst, H, C]`` (destinations, a prefix), ``key`` and ``value [N_src, H, C]``
    (sources): scaled score, softmax per destination and the weighted sum of ``value``
    (transformer_conv.py:263-283) in ONE pass over the by-destination slots; the backward is one
    pass by destination and one by source (csrc/transformer.hip).  ``value=None``: ``key`` is the
    packed projection ``[N_src, 2, H, C]`` (key, then value, of every source); both halves are
    read in place and ONE packed gradient comes back.  Saved: the inputs, ``alpha [E, H]`` (slot
    order) and ``out`` — nothing of size ``E x H*C``."""

    @staticmethod
    def forward(ctx, query: Tensor, key: Tensor, value: Optional[Tensor], graph: EdgeIndex,
                scale: float, n_dst: int):
        _, H, C = query.shape
        _check_rows(graph, n_dst, 'key', key, 'query', query)
        fwd = graph.by_dst()
        q2 = query.reshape(-1, H * C)
        k2, v2, packed = _key_value(key, value, H * C)
        alpha, out = _native.transformer_forward(fwd.ptr, fwd.idx, q2, k2, v2, H, C, scale,
                                                 hub=fwd.hub)
        ctx.save_for_backward(q2, k2, v2, alpha, out)
        ctx.graph, ctx.scale, ctx.dims, ctx.packed = graph, scale, (H, C), packed
        ctx.key_shape = key.shape
        return out.view(fwd.n_rows, H, C)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        q2, k2, v2, alpha, out = ctx.saved_tensors
        g_q, g_k, g_v, _, _ = _transformer_backward(
            ctx, q2, k2, v2, alpha, ctx.needs_input_grad[2], grad_out=_rows(grad_out), out=out,
            packed=ctx.packed)
        return g_q, g_k, g_v, None, None, None


class TransformerScoreFunction(Function):
    """The attention coefficients of :class:`TransformerAttendFunction` alone: ``alpha [E, H]`` in
    by-destination slot order, for layers that consume them themselves (dropout on the
    coefficients, ``return_attention_weights``) and aggregate with ``SpmmFunction(..., 'slot')``."""

    @staticmethod
    def forward(ctx, query: Tensor, key: Tensor, graph: EdgeIndex, scale: float, n_dst: int):
        _, H, C = query.shape
        _check_rows(graph, n_dst, 'key', key, 'query', query)
        fwd = graph.by_dst()
        q2, k2 = query.reshape(-1, H * C), key.reshape(-1, H * C)
        alpha, _ = _native.transformer_forward(fwd.ptr, fwd.idx, q2, k2, None, H, C, scale,
                                               hub=fwd.hub, aggregate=False)
        ctx.save_for_backward(q2, k2, alpha)
        ctx.graph, ctx.scale, ctx.dims, ctx.key_shape = graph, scale, (H, C), key.shape
        return alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_alpha: Tensor):
        q2, k2, alpha = ctx.saved_tensors
        g_q, g_k, _, _, _ = _transformer_backward(ctx, q2, k2, None, alpha,
                                                  grad_alpha=grad_alpha.contiguous())
        return g_q, g_k, None, None, None


def _edge_slots(edge_attr: Tensor, graph: EdgeIndex) -> Tensor:
    """``edge_attr [E, De]`` (the caller's edge order) in by-destination slot order, contiguous:
    the one permuted copy the edge kernels stream through."""
    if edge_attr.dim() != 2 or edge_attr.size(0) != graph.by_dst().idx.numel():
        raise ValueError(f"'edge_attr' must be [E, De] with one row per edge (got "
                         f"{tuple(edge_attr.shape)})")
    return edge_attr.index_select(0, graph.by_dst().perm.long())


def _edge_unslot(grad_slots: Optional[Tensor], graph: EdgeIndex) -> Optional[Tensor]:
    """a gradient in slot order back in the caller's edge order (``perm`` is a permutation: every
    row is written once)"""
    if grad_slots is None:
        return None
    grad = torch.empty_like(grad_slots)
    grad[graph.by_dst().perm.long()] = grad_slots
    return grad


class TransformerEdgeAttendFunction(Function):
    """:class:`TransformerAttendFunction` with edge features inside the kernel.  The edge term
    ``W_e a_k`` of key and value (transformer_conv.py:263-283) is linear, so it enters as a
    per-destination score bias and leaves as a per-destination sum of the RAW features:

        s[k,h] = scale <q_i, key_j> + <bias[i,h], a_k>       bias = scale * W_e^T q  [>= n_dst, H, De]
        out_nodes[i,h] = sum_k alpha value_j                 (without the edge term)
        z[i,h]         = sum_k alpha[k,h] a_k                [n_dst, H, De]

    and the caller adds ``W_e z`` to ``out_nodes``.  ``edge_attr [E, De]`` comes in the CALLER's
    edge order and is permuted into slot order once per call; its gradient is produced in slot
    order and scattered back, and skipped altogether when it is not required.  ``value=None``:
    ``key`` is the packed ``[N_src, 2, H, C]`` projection.  Saved: the inputs, ``alpha [E, H]``,
    ``out_nodes``, ``z`` and the slot-ordered ``edge_attr`` — nothing of size ``E x H*C``."""

    @staticmethod
    def forward(ctx, query: Tensor, key: Tensor, value: Optional[Tensor], edge_attr: Tensor,
                bias: Tensor, graph: EdgeIndex, scale: float, n_dst: int):
        _, H, C = query.shape
        _check_rows(graph, n_dst, 'key', key, 'query', query)
        fwd = graph.by_dst()
        q2 = query.reshape(-1, H * C)
        k2, v2, packed = _key_value(key, value, H * C)
        ea = _edge_slots(edge_attr, graph)
        De = ea.size(1)
        b2 = bias.reshape(-1, H * De)
        alpha, out, z = _native.transformer_edge_forward(fwd.ptr, fwd.idx, q2, k2, v2, ea, b2, H,
                                                         C, scale, hub=fwd.hub)
        ctx.save_for_backward(q2, k2, v2, ea, b2, alpha, out, z)
        ctx.graph, ctx.scale, ctx.dims, ctx.packed = graph, scale, (H, C, De), packed
        ctx.key_shape, ctx.bias_shape = key.shape, bias.shape
        return out.view(fwd.n_rows, H, C), z.view(fwd.n_rows, H, De)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor, grad_z: Tensor):
        q2, k2, v2, ea, b2, alpha, out, z = ctx.saved_tensors
        g_q, g_k, g_v, g_b, g_a = _transformer_backward(
            ctx, q2, k2, v2, alpha, ctx.needs_input_grad[2], grad_out=_rows(grad_out), out=out,
            edge_attr=ea, bias=b2, grad_z=_rows(grad_z), z=z,
            want_edge_attr=ctx.needs_input_grad[3], packed=ctx.packed)
        return g_q, g_k, g_v, g_a, g_b, None, None, None


class TransformerEdgeScoreFunction(Function):
    """The attention coefficients of :class:`TransformerEdgeAttendFunction` alone (``alpha [E, H]``
    in by-destination slot order), as :class:`TransformerScoreFunction` is to its node.  The
    backward takes ``grad_alpha`` and additionally returns ``grad_bias`` and the ``d s * bias``
    part of ``grad_edge_attr`` — all of it: ``z`` is formed by the caller from ``alpha``."""

    @staticmethod
    def forward(ctx, query: Tensor, key: Tensor, edge_attr: Tensor, bias: Tensor,
                graph: EdgeIndex, scale: float, n_dst: int):
        _, H, C = query.shape
        _check_rows(graph, n_dst, 'key', key, 'query', query)
        fwd = graph.by_dst()
        q2, k2 = query.reshape(-1, H * C), key.reshape(-1, H * C)
        ea = _edge_slots(edge_attr, graph)
        De = ea.size(1)
        b2 = bias.reshape(-1, H * De)
        alpha, _, _ = _native.transformer_edge_forward(fwd.ptr, fwd.idx, q2, k2, None, ea, b2, H,
                                                       C, scale, hub=fwd.hub, aggregate=False)
        ctx.save_for_backward(q2, k2, ea, b2, alpha)
        ctx.graph, ctx.scale, ctx.dims = graph, scale, (H, C, De)
        ctx.key_shape, ctx.bias_shape = key.shape, bias.shape
        return alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_alpha: Tensor):
        q2, k2, ea, b2, alpha = ctx.saved_tensors
        g_q, g_k, _, g_b, g_a = _transformer_backward(
            ctx, q2, k2, None, alpha, grad_alpha=grad_alpha.contiguous(), edge_attr=ea, bias=b2,
            want_edge_attr=ctx.needs_input_grad[2])
        return g_q, g_k, g_a, g_b, None, None, None


class GineAggregateFunction(Function):
    """The aggregation of GINEConv (gin_conv.py:185-207) in ONE pass over the by-destination slots:

        out[i] = (1 + eps) * x_root[i] + sum_{k of i} relu(x_src[j_k] + e_k)

    with ``e_k = edge_attr[k]`` (``weight=None``, the wide mode) or ``weight @ edge_attr[k] + bias``
    (the linear mode, ``edge_dim``), rebuilt per slot in registers (csrc/gine.hip).  ``edge_attr``
    stays in the caller's edge order and is read through the handle's permutations.  ``x_root``
    (destinations, a prefix of its rows), ``eps`` (one element), ``weight`` and ``bias`` may be
    ``None``.  The backward is one pass over the by-source slots, which rebuilds the ReLU mask:
    only the inputs are saved, nothing per edge; ``grad_edge_attr`` is not computed when it is
    not required."""

    @staticmethod
    def forward(ctx, x_src: Tensor, x_root: Optional[Tensor], eps: Optional[Tensor],
                edge_attr: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                graph: EdgeIndex, n_dst: int):
        _check_rows(graph, n_dst, 'x_src', x_src, 'x_root', x_root)
        fwd = graph.by_dst()
        eps1 = None if eps is None or x_root is None else eps.reshape(1)
        out = _native.gine_forward(fwd.ptr, fwd.idx, fwd.perm, x_src, x_root, eps1, edge_attr,
                                   weight, bias, hub=fwd.hub)
        ctx.save_for_backward(x_src, x_root, eps, edge_attr, weight, bias)
        ctx.graph = graph
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        need = ctx.needs_input_grad
        return _onepass.gine_backward(
            Slots.of_graph(ctx.graph), *ctx.saved_tensors, grad_out.contiguous(),
            want_x_src=need[0], want_root=need[1], want_eps=need[2], want_edge_attr=need[3],
            want_weight=need[4], want_bias=need[5]) + (None, None)


class GenAggregateFunction(Function):
    """The propagate step of GENConv under SoftmaxAggregation (gen_conv.py:213, 231-239 with
    aggr/basic.py:205-215) in ONE pass over the by-destination slots:

        out[i] = sum_{k of i} alpha_k m_k,   m_k = relu(x_src[j_k] + e_k) + eps_msg,
        alpha = softmax over the slots of i of t * m, per column

    with ``e_k`` = 0 (``edge_attr=None``), ``edge_attr[k]`` (width ``F``) or ``weight @ edge_attr[k]
    + bias`` (``lin_edge``), rebuilt per slot in registers (csrc/gen.hip).  ``t`` is a tensor of 1
    or ``F`` values.  ``edge_attr`` stays in the caller's edge order.  Saved for the backward: the
    inputs, ``out`` and two ``[n_dst, F]`` planes (three when ``t`` takes a gradient), nothing per
    edge.  The backward is an elementwise pre-pass and one pass over the by-source slots."""

    @staticmethod
    def forward(ctx, x_src: Tensor, edge_attr: Optional[Tensor], weight: Optional[Tensor],
                bias: Optional[Tensor], t: Tensor, graph: EdgeIndex, n_dst: int,
                eps_msg: float = 1e-7, semi_grad: bool = False):
        _check_rows(graph, n_dst, 'x_src', x_src, 'x_dst', None)
        fwd = graph.by_dst()
        out, saved = _native.gen_forward(fwd.ptr, fwd.idx, fwd.perm, x_src, edge_attr, weight,
                                         bias, t, eps_msg=eps_msg,
                                         want_s2=ctx.needs_input_grad[4], hub=fwd.hub)
        ctx.save_for_backward(x_src, edge_attr, weight, bias, t, out, saved)
        ctx.graph, ctx.eps_msg, ctx.semi_grad = graph, eps_msg, semi_grad
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        need = ctx.needs_input_grad
        return _onepass.gen_backward(
            Slots.of_graph(ctx.graph), *ctx.saved_tensors, grad_out.contiguous(),
            eps_msg=ctx.eps_msg, semi_grad=ctx.semi_grad, want_x_src=need[0],
            want_edge_attr=need[1], want_weight=need[2], want_bias=need[3],
            want_t=need[4]) + (None, None, None, None)


class ResGatedAggregateFunction(Function):
    """The propagate step of ResGatedGraphConv (res_gated_graph_conv.py:128, 138-148) in ONE pass
    over the by-destination slots:

        out[i] = sum_{k of i} sigmoid(k[i] + q[j_k] + Wg a_k) * (v[j_k] + Wv a_k)

    with the packed ``qv [N_src, 2F] = [q | v]`` gathered once per slot and ``a_k = edge_attr[k]``
    the RAW edge features (``edge_attr``, ``Wg`` and ``Wv [F, De]`` all None: no edge terms),
    rebuilt per slot in registers (csrc/resgated.hip).  ``k`` holds the destinations in a prefix of
    its rows; ``k`` and ``qv`` may be column blocks of wider tensors.  ``edge_attr`` stays in the
    caller's edge order.  Only the inputs are saved, nothing per edge: the backward, one pass by
    destination and one by source, recomputes the sigmoid."""

    @staticmethod
    def forward(ctx, k: Tensor, qv: Tensor, edge_attr: Optional[Tensor], Wg: Optional[Tensor],
                Wv: Optional[Tensor], graph: EdgeIndex, n_dst: int):
        _check_rows(graph, n_dst, 'qv', qv, 'k', k)
        fwd = graph.by_dst()
        out = _native.resgated_forward(fwd.ptr, fwd.idx, fwd.perm, k, qv, edge_attr,
                                       _onepass.resgated_weight(Wg, Wv), hub=fwd.hub)
        ctx.save_for_backward(k, qv, edge_attr, Wg, Wv)
        ctx.graph = graph
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        need = ctx.needs_input_grad
        return _onepass.resgated_backward(
            Slots.of_graph(ctx.graph), *ctx.saved_tensors, grad_out.contiguous(), want_k=need[0],
            want_qv=need[1], want_edge_attr=need[2],
            want_weights=need[3] or need[4]) + (None, None)


class CGAggregateFunction(Function):
    """The propagate step of CGConv (cg_conv.py:88, 93-98) with the residual of cg_conv.py:90 in
    ONE pass over the by-destination slots:

        out[i] = residual[i] + aggr_{k of i} sigmoid(zf_k) * softplus(zs_k)
        [zf_k | zs_k] = p[i] + q[j_k] + (edge terms of k)

    with the node-level ``p = [Pf | Ps] [>= n_dst, 2F]`` (both biases folded in) and ``q = [Qf |
    Qs] [N_src, 2F]``, one gathered row per slot — or ``q=None`` and ``p`` the packed ``[N, 4F] =
    [P | Q]`` of one node set in both roles, whose gradient is then ONE ``[N, 4F]`` plane.  Edge
    terms: none; ``edge_attr [E, De]`` with ``w_f``, ``w_s [F, De]`` (raw features, rebuilt per
    slot in registers); or ``edge_terms [E, 2F]`` (a dense product of the caller's; the backward
    writes its ``[E, 2F]`` gradient).  ``mean`` divides by the slot count; ``residual [n_dst, F]``
    may be None.  Only the inputs are saved; the backward, one pass by destination and one by
    source, recomputes both activations (csrc/cg.hip)."""

    @staticmethod
    def forward(ctx, p: Tensor, q: Optional[Tensor], edge_attr: Optional[Tensor],
                w_f: Optional[Tensor], w_s: Optional[Tensor], edge_terms: Optional[Tensor],
                residual: Optional[Tensor], graph: EdgeIndex, n_dst: int, mean: bool = False):
        if edge_terms is not None and edge_attr is not None:
            raise ValueError("'edge_attr' (with 'w_f', 'w_s') and 'edge_terms' exclude each other")
        P, Q = _onepass.cg_split(p, q)
        _check_rows(graph, n_dst, 'q', Q, 'p', P)
        fwd = graph.by_dst()
        out = _native.cg_forward(fwd.ptr, fwd.idx, fwd.perm, P, Q,
                                 edge_attr if edge_terms is None else edge_terms,
                                 _onepass.cg_weight(w_f, w_s), residual=residual, mean=mean,
                                 hub=fwd.hub)
        ctx.save_for_backward(p, q, edge_attr, w_f, w_s, edge_terms)
        ctx.graph, ctx.mean = graph, bool(mean)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        need = ctx.needs_input_grad
        grad_out = grad_out.contiguous()
        grads = _onepass.cg_backward(
            Slots.of_graph(ctx.graph), *ctx.saved_tensors, grad_out, mean=ctx.mean,
            want_p=need[0], want_q=need[1], want_edge_attr=need[2],
            want_weights=need[3] or need[4], want_edge_terms=need[5])
        return grads + (grad_out if need[6] else None, None, None, None)


class FiLMAggregateFunction(Function):
    """The R masked propagate steps of FiLMConv (film_conv.py:134-153, its message at 157-161) and
    the sum with the skip term in ONE pass over the by-destination slots of all edges:

        out[i] = residual[i] + sum_{k of i} scale[e_k] * act(gamma_{r,i} * H[j_k, block r] + beta_{r,i})

    with ``r`` the relation of slot ``k``'s edge, the node-level ``h = H [N_src, R * F]`` and ``g =
    G [>= n_dst, R * 2F]`` (block ``r`` = ``[beta_r | gamma_r]``) — or ``g=None`` and ``h`` the
    packed ``[N, 3 R F] = [H | G]`` of one node set in both roles, whose gradient is then ONE
    plane of that shape.  ``forms`` (:class:`_onepass.FilmForms`) carries the handle, ``rel``,
    the mean normaliser and the two pair forms of the backward; ``relu=False``: no activation.
    Only the inputs are saved; the backward, one pass over the ``(relation, destination)`` pair
    rows and one over the ``(relation, source)`` pair rows, recomputes the activation's mask
    (csrc/film.hip)."""

    @staticmethod
    def forward(ctx, h: Tensor, g: Optional[Tensor], residual: Optional[Tensor], forms,
                relu: bool = True):
        out = _onepass.film_forward(forms, h, g, residual, bool(relu))
        ctx.save_for_backward(h, g)
        ctx.forms, ctx.relu = forms, bool(relu)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        need = ctx.needs_input_grad
        grad_out = grad_out.contiguous()
        grads = _onepass.film_backward(ctx.forms, *ctx.saved_tensors, grad_out, relu=ctx.relu,
                                       want_h=need[0], want_g=need[1])
        return grads + (grad_out if need[2] else None, None, None)


class RGATAggregateFunction(Function):
    """RGATConv's additive message with the softmax across all relations of a destination, or
    (``within``) within every relation (rgat_conv.py:397-437, 500-502), and the 'add' aggregation
    in ONE pass over the by-destination slots of all edges (``within``: after one scalar launch
    over the ``(relation, destination)`` pair rows):

        out[i, h] = sum_k softmax_k(leaky_relu(QI[i, r, h] + KJ[j, r, h] + B[e, h])) * P[j, r, h]

    with ``r`` the relation of slot ``k``'s edge: ``p = P [N, R * H * C]``, ``qi`` / ``kj [N, R *
    H]`` — or ``qi = kj = None`` and ``p`` the packed ``[N, R (H C + 2 H)] = [P | QI | KJ]``, whose
    gradient is then ONE plane of that shape.  ``b [E, H]`` (or None) is the per-edge score bias
    in the CALLER's edge order.  ``forms`` is a :class:`_onepass.RgatForms`.  Returns ``(out [n_dst,
    H * C], alpha [E, H])``, ``alpha`` in the caller's edge order and not differentiable.  Saved:
    the inputs, ``alpha`` and ``out`` — nothing of size ``E x H*C``.  The backward is one pass over
    the same rows and one over each of the two pair forms (csrc/rgat.hip)."""

    @staticmethod
    def forward(ctx, p: Tensor, qi: Optional[Tensor], kj: Optional[Tensor], b: Optional[Tensor],
                forms, H: int, C: int, slope: float, within: bool = False):
        if (qi is None) != (kj is None):
            raise ValueError("'qi' and 'kj' are given together or not at all")
        if b is not None and forms.perm is not None:
            b = b.index_select(0, forms.perm)   # slot order
        alpha, out = _onepass.rgat_forward(forms, p, qi, kj, b, H, C, slope, bool(within))
        ctx.save_for_backward(p, qi, kj, b, alpha, out)
        ctx.forms, ctx.dims, ctx.within = forms, (int(H), int(C), float(slope)), bool(within)
        alpha_e = alpha if forms.inv is None else alpha.index_select(0, forms.inv)
        ctx.mark_non_differentiable(alpha_e)
        return out, alpha_e

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor, _grad_alpha):
        p, qi, kj, b, alpha, out = ctx.saved_tensors
        H, C, slope = ctx.dims
        g_p, g_qi, g_kj, g_b = _onepass.rgat_backward(
            ctx.forms, p, qi, kj, b, alpha, out, grad_out.contiguous(), H, C, slope,
            within=ctx.within, want_b=b is not None and ctx.needs_input_grad[3])
        if g_b is not None and ctx.forms.inv is not None:
            g_b = g_b.index_select(0, ctx.forms.inv)
        return g_p, g_qi, g_kj, g_b, None, None, None, None, None


class MixtureConvFunction(Function):
    """The propagate step of a layer whose message is a per-edge mixture of ``K`` linear maps —
    GMMConv (gmm_conv.py:154-165) and NNConv (nn_conv.py:119-122) — aggregate first:

        out[i] = (sum_{e: dst(e) = i} coef[e, :] (x) x_src[src(e)]).reshape(K * F) @ weight

    with ``coef [E, K]`` in the caller's edge order and ``weight [K, F, M]``: one expand launch
    that gathers ONE row of ``F`` floats per slot (csrc/mixture.hip) and one dense product on the
    package's GEMM route.  Only the inputs are saved; the backward recomputes the wide plane with
    one more expand, and nothing of size ``E x`` anything wider than ``K`` exists at any time.
    What ``needs_input_grad`` does not ask for is not computed."""

    @staticmethod
    def forward(ctx, x_src: Tensor, coef: Tensor, weight: Tensor, graph: EdgeIndex, n_dst: int):
        _check_rows(graph, n_dst, 'x_src', x_src, 'x_dst', None)
        if (x_src.dim() != 2 or coef.dim() != 2 or weight.dim() != 3
                or weight.size(1) != x_src.size(1) or weight.size(0) != coef.size(1)):
            raise ValueError(f"'x_src' [N, F], 'coef' [E, K] and 'weight' [K, F, M] do not agree "
                             f"(got {tuple(x_src.shape)}, {tuple(coef.shape)}, "
                             f"{tuple(weight.shape)})")
        fwd = graph.by_dst()
        out = _onepass.mixture_forward(fwd, fwd.perm, x_src, coef, weight)
        ctx.save_for_backward(x_src, coef, weight)
        ctx.graph = graph
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        need = ctx.needs_input_grad
        return _onepass.mixture_backward(
            Slots.of_graph(ctx.graph), *ctx.saved_tensors, grad_out.contiguous(), want_x=need[0],
            want_coef=need[1], want_weight=need[2]) + (None, None)


class PnaAggregateFunction(Function):
    """The aggregation of PNAConv with a linear message (pna_conv.py:175-188 under
    aggr/scaler.py:82) in ONE pass over the by-destination slots.  The message of slot ``k`` of
    destination ``i`` is ``p_dst[i] + u_k`` with ``u_k = p_src[j_k] + wc @ edge_attr[k]``
    (``edge_attr`` and ``wc`` None: ``u_k = p_src[j_k]``); ``stats`` is a tuple out of ``'mean'``,
    ``'min'``, ``'max'``, ``'std'`` and the result a tuple of ``[n_dst, W]`` tensors in its order,
    exactly 0 for destinations without slots.  ``edge_attr`` stays in the caller's edge order.
    Saved for the backward: the inputs and six ``[n_dst, W]`` planes, nothing per edge.  The
    backward is an elementwise pre-pass (:func:`pna_coefficients`) and one pass over the by-source
    slots; ``grad_edge_attr`` is not computed when it is not required."""

    @staticmethod
    def forward(ctx, p_src: Tensor, p_dst: Tensor, edge_attr: Optional[Tensor],
                wc: Optional[Tensor], graph: EdgeIndex, n_dst: int, stats):
        stats = tuple(stats)
        _check_rows(graph, n_dst, 'p_src', p_src, 'p_dst', p_dst)
        fwd = graph.by_dst()
        out, saved = _native.pna_forward(fwd.ptr, fwd.idx, fwd.perm, p_src, p_dst, edge_attr, wc,
                                         stats, hub=fwd.hub)
        ctx.save_for_backward(p_src, edge_attr, wc, saved)
        ctx.graph, ctx.stats, ctx.dst_rows = graph, stats, p_dst.size(0)
        order = sorted(stats, key=_native.PNA_STATS.index)
        return tuple(out[order.index(s)] for s in stats)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        need = ctx.needs_input_grad
        return _onepass.pna_backward(
            Slots.of_graph(ctx.graph), *ctx.saved_tensors, ctx.stats, grads, ctx.dst_rows,
            want_src=need[0], want_dst=need[1], want_edge_attr=need[2],
            want_wc=need[3]) + (None, None, None)


class HgtRelationPlan:
    """Static description of one relation-transform node: ``heads``; ``src_pos[e]``: the position
    (among the tensor inputs) of the source node type of edge type ``e`` of the call; ``widx[e]``:
    its position in the layer's metadata, i.e. its matrix ``h * T + widx[e]`` of the weights."""

    def __init__(self, heads: int, src_pos, widx):
        self.heads, self.src_pos, self.widx = int(heads), tuple(src_pos), tuple(widx)


class HGTRelationFunction(Function):
    """The typed relation transform of HGTConv (hgt_conv.py:118-154) for every edge type of a
    layer call in ONE launch: ``kqvs[t] [N_t, 3 * F]`` (the key | query | value projection of
    source node type ``t``, read in place) and the relation weights ``[H * T, D, D]`` as the
    parameters hold them -> the packed ``kv [S, 2 * F]`` of the stacked source rows, the table
    ``TransformerAttendFunction`` reads.  The backward is one launch too (csrc/hgt.hip): the key
    and value gradients of a node type land in the k and v column blocks of one ``[N_t, 3 * F]``
    buffer (its q block is cleared: the query gradient arrives through the caller's slice), the
    weight gradients are reduced from per-workgroup partials in a fixed order — no atomics."""

    @staticmethod
    def forward(ctx, plan: HgtRelationPlan, wk: Tensor, wv: Tensor, *kqvs: Tensor):
        H, D = plan.heads, wk.size(-1)
        F = H * D
        for x in kqvs:
            if x.dim() != 2 or x.size(1) != 3 * F:
                raise ValueError(f"every 'kqv' must be [N, {3 * F}] (got {tuple(x.shape)})")
        kqvs = tuple(_native._f32_rows(x, 'kqv') for x in kqvs)
        wk, wv = wk.contiguous(), wv.contiguous()
        ks, vs = _onepass.hgt_blocks(kqvs, plan.src_pos, F)
        kv = _native.hgt_relation_forward(ks, vs, plan.widx, wk, wv, H, D)
        ctx.save_for_backward(wk, wv, *kqvs)
        ctx.plan = plan
        return kv

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_kv: Tensor):
        wk, wv, *kqvs = ctx.saved_tensors
        plan, need = ctx.plan, ctx.needs_input_grad
        bufs, g_wk, g_wv = _onepass.hgt_backward(
            kqvs, wk, wv, plan.src_pos, plan.widx, plan.heads, grad_kv, want_kqvs=any(need[3:]),
            want_weights=need[1] or need[2])
        return (None, g_wk, g_wv) + (tuple(bufs) if bufs else (None, ) * len(kqvs))


class HeadDotFunction(Function):
    """(a_src, a_dst) = ((x * att_src).sum(-1), (x * att_dst).sum(-1)) for x [N, H, C] and
    att_* [1, H, C] (nn/conv/gat_conv.py:330-332) — one pass over x, one fused backward."""

    @staticmethod
    def forward(ctx, x: Tensor, att_a: Tensor, att_b: Optional[Tensor]):
        N, H, C = x.shape
        out_a, out_b = _native.head_dot_forward(x.reshape(N, H * C), att_a.reshape(-1),
                                                None if att_b is None else att_b.reshape(-1),
                                                H, C)
        if att_b is None:
            raise ValueError('HeadDotFunction needs both attention vectors')
        ctx.save_for_backward(x, att_a, att_b)
        ctx.has_b = True
        return out_a, out_b

    @staticmethod
    def backward(ctx, grad_a: Tensor, grad_b: Tensor):
        x, att_a, att_b = ctx.saved_tensors
        N, H, C = x.shape
        if grad_a is None:
            grad_a = x.new_zeros(N, H)
        if ctx.has_b and grad_b is None:
            grad_b = x.new_zeros(N, H)
        gx, ga, gb = _native.head_dot_backward(
            x.reshape(N, H * C), att_a.reshape(-1), None if att_b is None else att_b.reshape(-1),
            grad_a, grad_b if ctx.has_b else None, H, C, ctx.needs_input_grad[0])
        return (None if gx is None else gx.view(N, H, C), ga.view(att_a.shape),
                None if gb is None else gb.view(att_b.shape))


class LinearFunction(Function):
    """``x @ weight.T + bias`` (nn/dense/linear.py:121-127 ``F.linear``) on the fp32-MFMA kernels
    of csrc/gemm.hip: forward with the bias epilogue, input gradient with the same kernel on the
    transposed weight, weight gradient as a deterministic split reduction that also returns the
    bias gradient (column sums of ``grad_out``) from the same pass."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor]):
        x2 = x.reshape(-1, x.size(-1))
        ctx.save_for_backward(x2, weight)
        ctx.x_shape, ctx.has_bias = x.shape, bias is not None
        out = _native.linear_forward(x2, weight, bias)
        return _shaped(out, (*x.shape[:-1], weight.size(0)))

    @staticmethod
    @once_differentiable  # the kernels record no graph: create_graph=True raises instead of
    def backward(ctx, grad_out: Tensor):  # silently dropping the second derivative
        x2, weight = ctx.saved_tensors
        g2 = grad_out.reshape(-1, grad_out.size(-1))
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _native.linear_dgrad(g2, weight.t().contiguous()).view(ctx.x_shape)
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            gw = _native.linear_wgrad(g2, x2, bias_grad=need_b)  # column sums from the same pass
            if need_b:
                gw, gb = gw
        elif need_b:
            gb = _native.colsum(g2)
        return gx, gw, gb


# Below this many rows the library GEMM stays (F.linear): a Python-side autograd Function per call
# costs more than such a product.  From here up the own kernels fill the chip: 128-row tiles for
# the full-batch layers, 64 x 64 tiles + a deterministic split over the reduction for sampled
# blocks and Cora-sized inputs (csrc/gemm.hip nt_shape; round 3 drew this line at 16,384 rows).
OWN_GEMM_MIN_ROWS = 1024


def own_linear_eligible(x: Tensor, weight: Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32
            and x.dim() >= 2 and x.numel() // max(x.size(-1), 1) >= OWN_GEMM_MIN_ROWS
            and not torch.jit.is_scripting() and not torch.is_autocast_enabled())


# The autograd nodes of csrc/torch_binding.cpp (LinearAG / SpmmAG / BiasActAG): the same kernels in
# the same order as LinearFunction / SpmmFunction / BiasActFunction below, with forward AND backward
# running in C++ — an eager, launch-bound step (2-layer GCN at the Cora shape) spends most of its
# host time in the Python Functions and their marshalling (scripts/eager_probe.py).  Taken for
# plain float32 operands when nothing beyond those nodes is asked for; PYGAMD_CPP_AUTOGRAD=0, a
# missing binding, torch.compile tracing or bench.py's per-launch timing sink keep the Python nodes.
CPP_AUTOGRAD = os.environ.get('PYGAMD_CPP_AUTOGRAD', '1') != '0'


def _cpp_nodes():
    if not CPP_AUTOGRAD or _native.timing_sink is not None or torch.compiler.is_compiling():
        return None
    from . import _compiled
    return _compiled.ops()


def _plain_f32(*ts) -> bool:
    return all(t is None or (type(t) in (Tensor, torch.nn.Parameter) and t.is_cuda
                             and t.dtype == torch.float32) for t in ts)


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """``F.linear`` semantics (``weight [out, in]``); large float32 HIP inputs run on csrc/gemm.hip."""
    if own_linear_eligible(x, weight):
        C = _cpp_nodes()
        if C is not None and _plain_f32(x, weight, bias) and x.size(-1) == weight.size(1) \
                and (bias is None or bias.numel() == weight.size(0)):
            return C.linear_ag(x, weight, bias)
        return LinearFunction.apply(x, weight, bias)
    return torch.nn.functional.linear(x, weight, bias)


def spmm_node(x: Tensor, w: Optional[Tensor], graph: EdgeIndex, reduce: str,
              w_order: str) -> Tensor:
    """``SpmmFunction.apply`` semantics; sum / mean with no gradient asked for the weights run as
    the C++ autograd node."""
    C = _cpp_nodes()
    # The C++ node takes BOTH sorted forms up front.  The by-source one (a transposed sort + a hub
    # plan with a host read, per fresh graph) only serves the gradient of `x`: inference under
    # no_grad and first layers whose `x` takes no gradient keep the Python node, which builds it
    # inside backward() when needs_input_grad[0] says so.
    if (C is not None and reduce in ('sum', 'mean') and _plain_f32(x, w) and x.dim() >= 2
            and torch.is_grad_enabled() and x.requires_grad
            and x.numel() > 0 and x.size(0) == graph.num_src_nodes and not graph.atomic_backward
            and (w is None or (w.dim() == 1 and not w.requires_grad
                               and w.numel() == graph.num_edges))):
        fwd, bwd = graph.by_dst(), graph.by_src()
        hub, hub_t = fwd.hub, bwd.hub
        # (the node's schema takes ONE threshold and chunk for its two plans: plans made at
        # different settings go through the Python node, which launches each with its own)
        if (hub.threshold, hub.chunk) == (hub_t.threshold, hub_t.chunk):
            eid = eid_t = None
            if w is not None:
                eid = fwd.perm if w_order == 'coo' else None
                eid_t = bwd.perm if w_order == 'coo' else graph.src_slot_to_dst_slot()
            inv = fwd.inv_degree() if reduce == 'mean' else None
            return C.spmm_ag(x, w, fwd.ptr, fwd.idx, eid, *hub[:4], bwd.ptr, bwd.idx, eid_t,
                             *hub_t[:4], inv, _native.REDUCE_IDS[reduce], hub.threshold, hub.chunk)
    return SpmmFunction.apply(x, w, graph, reduce, w_order)


class BiasActFunction(Function):
    """``relu(x + bias)`` (or ``x + bias``) in one pass, backward in one pass: the masked gradient
    and — from the same read — its column sums, the bias gradient (``pygamd_bias_act`` /
    ``pygamd_relu_backward_colsum``).  Replaces ``out + self.bias`` of a conv layer
    (gat_conv.py:378-385, gcn_conv.py:278-281) followed by the model's ReLU
    (basic_gnn.py:262-263): four ATen passes forward + backward become two."""

    @staticmethod
    def forward(ctx, x: Tensor, bias: Optional[Tensor], relu: bool):
        x2 = x.reshape(-1, x.size(-1))
        out = _native.bias_act(x2, bias, relu)
        ctx.relu, ctx.has_bias, ctx.shape = relu, bias is not None, x.shape
        res = _shaped(out, x.shape)
        if relu:
            ctx.save_for_backward(res)
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        g2 = grad_out.reshape(-1, grad_out.size(-1))
        need_b = ctx.has_bias and ctx.needs_input_grad[1]
        if ctx.relu:
            (out, ) = ctx.saved_tensors
            g, gb = _native.relu_backward_colsum(g2, out.reshape(-1, out.size(-1)), need_b)
            return g.view(ctx.shape), (gb if need_b else None), None
        return grad_out, (_native.colsum(g2) if need_b else None), None


def bias_act(x: Tensor, bias: Optional[Tensor], relu: bool) -> Tensor:
    """``relu(x + bias)`` / ``x + bias``; float32 device tensors take the one-pass kernels."""
    if x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and x.numel() > 0 \
            and (bias is None or (bias.dtype == torch.float32 and bias.dim() == 1)) \
            and not torch.jit.is_scripting() and not torch.is_autocast_enabled():
        C = _cpp_nodes()
        if C is not None and _plain_f32(x, bias) and (bias is None or bias.numel() == x.size(-1)):
            return C.bias_act_ag(x, bias, bool(relu))
        return BiasActFunction.apply(x, bias, relu)
    out = x if bias is None else x + bias
    return out.relu() if relu else out


class CrossEntropyRowsFunction(Function):
    """``F.cross_entropy(logits[index], target[index])`` — the loss a full-batch model takes on its
    training split (``examples/ogbn_train.py``-style ``out[train_idx]``) — as ONE pass over the
    selected rows forward (no gathered copy of the rows, no separate log-softmax / NLL launches)
    and a row scatter backward: seven ATen launches (0.75 ms at the ogbn-products shape, whose
    ``nll_loss`` reductions run on one workgroup) become two + three."""

    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor, index: Optional[Tensor]):
        loss, grad_rows = _native.cross_entropy_rows(logits, target, index)
        ctx.save_for_backward(grad_rows, index)
        ctx.shape = logits.shape
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g: Tensor):
        grad_rows, index = ctx.saved_tensors
        scaled = grad_rows * g
        if index is None:
            return scaled, None, None
        dense = torch.zeros(ctx.shape, dtype=torch.float32, device=scaled.device)
        dense.index_add_(0, index, scaled)   # (duplicate indices add up, as out[index] would)
        return dense, None, None


def cross_entropy(logits: Tensor, target: Tensor, index: Optional[Tensor] = None) -> Tensor:
    """Mean cross entropy of ``logits[index]`` against ``target[index]`` (``index`` None: every
    row); ``target``: one int64 label per row of ``logits``.  Float32 HIP logits take the one-pass
    kernel; anything else (CPU tensors, other dtypes, class weights are not offered) runs
    ``F.cross_entropy`` on the gathered rows."""
    if (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
            and logits.size(0) > 0 and logits.size(1) > 0 and logits.stride(1) == 1
            and target.dtype == torch.int64 and target.dim() == 1
            and target.numel() == logits.size(0)
            and (index is None or (index.dtype == torch.int64 and index.dim() == 1
                                   and index.numel() > 0))
            and not torch.cuda.is_current_stream_capturing()):
        return CrossEntropyRowsFunction.apply(
            logits, target.contiguous(), None if index is None else index.contiguous())
    if index is None:
        return torch.nn.functional.cross_entropy(logits, target)
    return torch.nn.functional.cross_entropy(logits[index], target[index])


class GraphNormFunction(Function):
    """Per-graph normalisation of the rows of ``x [N, F]`` over the graphs of a by-graph handle
    (``_norm.BatchHandle``: ``ptr`` and its hub plan), csrc/graph_norm.hip:

    * ``mode='channel'`` — GraphNorm (graph_norm.py:72-76): ``weight * u / sqrt(mean(u^2) + eps) +
      bias`` with ``u = x - mean_scale * mean(x)``, statistics per graph and column;
    * ``mode='graph'`` — LayerNorm over whole graphs (layer_norm.py:82-108); ``std_eps`` selects
      the reference's formula without a batch vector, ``/ (std + eps)``.

    One launch forward and two backward when no graph is longer than the plan's threshold (three
    and four otherwise).  Saved: ``x``, the parameters and the per-graph ``mean`` and ``rstd`` —
    nothing of size ``N x F``."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                mean_scale: Optional[Tensor], handle, eps: float, mode: str,
                std_eps: bool = False):
        y, mean, rstd = _native.graph_norm_forward(handle.ptr, x, weight, bias, mean_scale, eps,
                                                   mode, std_eps=std_eps, hub=handle.hub)
        ctx.save_for_backward(x, weight, mean_scale, mean, rstd)
        ctx.handle, ctx.eps, ctx.mode, ctx.std_eps = handle, eps, mode, bool(std_eps)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y: Tensor):
        x, weight, mean_scale, mean, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_x, g_w, g_b, g_ms = _native.graph_norm_backward(
            ctx.handle.ptr, x, grad_y, mean, rstd, weight, mean_scale, ctx.eps, ctx.mode,
            std_eps=ctx.std_eps, hub=ctx.handle.hub, want_weight=need[1] and weight is not None,
            want_bias=need[2] and ctx.has_bias,
            want_mean_scale=need[3] and mean_scale is not None)
        return g_x if need[0] else None, g_w, g_b, g_ms, None, None, None, None


class GatherScaleFunction(Function):
    """``(multiplier * (x[perm] * score[perm].view(-1, 1)), score[perm])`` of the pooling layers
    (topk_pool.py:118-122, sag_pool.py:132-136), csrc/pool.hip: one launch forward and — after the
    one memset of the two gradients' shared buffer — one backward, where the reference has two or
    three ``[M, F]`` passes and an ``index_put``, a broadcast multiply and a row sum.  ``perm``
    holds no node twice.  Saved: ``x``, ``score`` and ``perm`` — nothing of size ``M x F``."""

    @staticmethod
    def forward(ctx, x: Tensor, score: Tensor, perm: Tensor, multiplier: float):
        out, weight = _native.gather_scale_forward(x, score, perm, multiplier)
        ctx.save_for_backward(x, score, perm)
        ctx.multiplier = float(multiplier)
        return out, weight

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor, grad_weight: Optional[Tensor]):
        """When both gradients are wanted they are views of ONE zero-filled buffer (one memset):
        ``grad_x`` keeps the storage of the ``[N]`` score gradient alive and the reverse."""
        x, score, perm = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not (need[0] or need[1]):
            return None, None, None, None
        g_x, g_s = _native.gather_scale_backward(x, score, perm, ctx.multiplier, grad_out,
                                                 grad_weight, want_x=need[0], want_score=need[1])
        return g_x, g_s, None, None


def _check_hop(graph: EdgeIndex, x: Tensor, w: Optional[Tensor], square: bool = False):
    if x.size(0) != graph.num_src_nodes:
        raise ValueError(f"'x' has {x.size(0)} rows but the graph has {graph.num_src_nodes} "
                         f"source nodes")
    if square and graph.num_src_nodes != graph.num_dst_nodes:
        raise ValueError(f"a repeated propagation needs a square graph (got sparse_size="
                         f"{graph.sparse_size})")
    if w is not None and w.numel() != graph.num_edges:
        raise ValueError(f"'w' needs one value per edge ({graph.num_edges}), got {w.numel()}")


class HopFunction(Function):
    """One propagation step with its combination as the row epilogue (csrc/hop.hip; lg_conv.py:50,
    gcn2_conv.py:138-141, one iteration of appnp.py:129-131 and tag_conv.py:90):

        out[i] = a * sum_{(j -> i)} w_e x[j]  (+ b * y[i])  (+ c * z[i])

    ONE launch over the by-destination slots; ``w`` (one value per edge in the graph's edge order,
    or None) takes no gradient here — a layer whose weights require one runs its generic route.
    ``y`` / ``z``: one row per destination, column blocks of wider tensors are read in place.  The
    backward is the same launch over the by-source slots, ``grad_x = a * A^T grad_out``, and one
    elementwise pass per ``y`` / ``z`` that wants a gradient; nothing but ``w`` is saved."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Optional[Tensor], y: Optional[Tensor], z: Optional[Tensor],
                graph: EdgeIndex, a: float, b: float, c: float):
        _check_hop(graph, x, w)
        fwd = graph.by_dst()
        out = _onepass.hop_forward(fwd, fwd.perm, w, x, a, y, b, z, c)
        ctx.save_for_backward(w)
        ctx.graph, ctx.coef = graph, (a, b, c)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        w, = ctx.saved_tensors
        need = ctx.needs_input_grad
        a, b, c = ctx.coef
        g_x, g_y, g_z = _onepass.hop_backward(Slots.of_graph(ctx.graph), w, grad_out.contiguous(),
                                              a, b, c, want_x=need[0], want_y=need[2],
                                              want_z=need[3])
        return g_x, None, g_y, g_z, None, None, None, None


class HopsFunction(Function):
    """``K >= 1`` propagation steps ``x_k = a * A x_{k-1} + b * h`` (appnp.py:111-133 with ``h =
    x_0``, sg_conv.py:93-95 with ``b = 0``) and, with ``want_sum``, the running combination ``s =
    d0 * x_0 + d * (x_1 + ... + x_K)`` of ssg_conv.py:102-106, on a square graph.  Returns ``x_K``
    or ``(x_K, s)``.  ``h``: a tensor, None (no second term) or — ``tied`` — ``x`` itself.

    Forward: exactly K launches, the combination and the running sum being their epilogue.
    Backward: exactly K launches over the by-source slots and at most two elementwise passes,
    whatever K (:func:`_onepass.hops_backward`).  The recurrence is linear in ``x`` and ``h``, so
    the backward needs no iterate: only ``w`` is saved."""

    @staticmethod
    def forward(ctx, x: Tensor, h: Optional[Tensor], w: Optional[Tensor], graph: EdgeIndex,
                K: int, a: float, b: float, d0: float, d: float, want_sum: bool, tied: bool):
        if K < 1:
            raise ValueError("'K' must be at least 1 (K = 0 is the identity: no call)")
        if tied and h is not None:
            raise ValueError("'tied' takes 'x' as 'h': pass h=None")
        _check_hop(graph, x, w, square=True)
        if h is not None and h.shape != x.shape:
            raise ValueError(f"'h' must have the shape of 'x' (got {tuple(h.shape)})")
        fwd = graph.by_dst()
        xk, s = _onepass.hops_forward(fwd, fwd.perm, w, x, x if tied else h, K, a, b, d0, d,
                                      want_sum)
        ctx.save_for_backward(w)
        ctx.graph, ctx.args = graph, (K, a, b, d0, d)
        ctx.has_h, ctx.tied, ctx.want_sum = tied or h is not None, tied, want_sum
        ctx.set_materialize_grads(False)  # (an unused x_K or s costs no pass over zeros)
        return (xk, s) if want_sum else xk

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_x: Optional[Tensor], grad_s: Optional[Tensor] = None):
        w, = ctx.saved_tensors
        need = ctx.needs_input_grad
        if grad_x is None and grad_s is None:
            return (None, ) * 11
        g_x, g_h = _onepass.hops_backward(
            Slots.of_graph(ctx.graph), w, *ctx.args,
            None if grad_x is None else grad_x.contiguous(),
            None if grad_s is None else grad_s.contiguous(), has_h=ctx.has_h, tied=ctx.tied,
            want_x=need[0], want_h=need[1] and not ctx.tied)
        return (g_x, g_h) + (None, ) * 9
