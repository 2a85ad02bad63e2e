"""``torch.ops.pyg_amd.*`` — the kernels as registered PyTorch operators (seam S2 of SURVEY.md §8(b)).

The reference reaches its native code through operator SCHEMAS it expects to exist:
``torch.ops.torch_sparse.spmm_{sum,mean,min,max}`` (edge_index.py:1798-1810),
``torch_scatter.segment_csr`` / ``scatter`` (utils/_segment.py:34, utils/_scatter.py:104),
``pyg_lib.ops.softmax_csr`` (utils/_softmax.py:58), ``pyg_lib.ops.index_sort``
(utils/_index_sort.py:32).  This module registers the MI355X counterparts under the ``pyg_amd``
namespace with ``torch.library``:

* a device implementation (HIP, through the C ABI) for ``cuda`` tensors only — there is no CPU
  kernel, a CPU tensor fails in the dispatcher;
* a FAKE (meta) kernel per operator, so ``FakeTensorMode`` / ``torch.compile`` / ``torch.export``
  can propagate shapes and dtypes without running anything;
* autograd through ``torch.library.register_autograd``: every differentiable operator is paired
  with an opaque ``*_backward`` operator (itself registered with a fake kernel), so AOTAutograd can
  trace forward and backward graphs — under ``torch.compile`` the kernels stay single opaque nodes
  instead of forcing the backend to step aside (round-1 behaviour).

Operators (all index tensors int32 / int64, features float32):

==========================  ===========================================================
``index_sort``              ``(Tensor inputs, int? max_value) -> (Tensor, Tensor)``
``index2ptr`` / ``ptr2index``  ``(Tensor, int) -> Tensor``
``gather``                  ``(Tensor x, Tensor index) -> Tensor``           (index_select dim 0)
``scatter``                 ``(Tensor src, Tensor index, int dim_size, str reduce) -> Tensor``
``segment_csr``             ``(Tensor src, Tensor ptr, str reduce) -> Tensor``
``softmax_csr``             ``(Tensor src, Tensor ptr) -> Tensor``
``spmm``                    ``(Tensor rowptr, Tensor col, Tensor? value, Tensor other, str reduce)``
``linear``                  ``(Tensor x, Tensor weight, Tensor? bias) -> Tensor``
``gatv2_attend``            ``(Tensor x_l, Tensor x_r, Tensor att, Tensor rowptr, Tensor col,
                            float negative_slope) -> (Tensor out, Tensor alpha)``
``han_attend``              ``(Tensor x_all, Tensor a_src, Tensor a_dst, Tensor rowptr, Tensor col,
                            int[] row_begin, int[] src_begin, int[] val_shift,
                            float negative_slope, bool relu) -> (Tensor out, Tensor alpha)``
``transformer_attend``      ``(Tensor query, Tensor key, Tensor value, Tensor rowptr, Tensor col,
                            float scale) -> (Tensor out, Tensor alpha)``
``transformer_edge_attend`` ``(Tensor query, Tensor key, Tensor value, Tensor edge_attr,
                            Tensor bias, Tensor rowptr, Tensor col, float scale)
                            -> (Tensor out, Tensor z, Tensor alpha)``
``hgt_relation``            ``(Tensor[] kqvs, Tensor k_weight, Tensor v_weight, int[] src_pos,
                            int[] widx, int heads) -> Tensor``
``gine_aggregate``          ``(Tensor x_src, Tensor? x_root, Tensor? eps, Tensor edge_attr,
                            Tensor? weight, Tensor? bias, Tensor rowptr, Tensor col,
                            Tensor? edge_id) -> Tensor``
``pna_aggregate``           ``(Tensor p_src, Tensor p_dst, Tensor? edge_attr, Tensor? wc,
                            Tensor rowptr, Tensor col, Tensor? edge_id, int stats)
                            -> (Tensor out, Tensor saved)``
``gen_aggregate``           ``(Tensor x_src, Tensor? edge_attr, Tensor? weight, Tensor? bias,
                            Tensor t, Tensor rowptr, Tensor col, Tensor? edge_id, float eps_msg,
                            bool semi_grad, bool grad_t) -> (Tensor out, Tensor saved)``
``resgated_aggregate``      ``(Tensor k, Tensor qv, Tensor? edge_attr, Tensor? w_gate,
                            Tensor? w_value, Tensor rowptr, Tensor col, Tensor? edge_id)
                            -> Tensor``
``mixture_conv``            ``(Tensor x_src, Tensor coef, Tensor weight, Tensor rowptr,
                            Tensor col, Tensor? edge_id) -> Tensor``
``cg_aggregate``            ``(Tensor p, Tensor? q, Tensor? edge_attr, Tensor? w_f, Tensor? w_s,
                            Tensor? edge_terms, Tensor? residual, Tensor rowptr, Tensor col,
                            Tensor? edge_id, bool mean) -> Tensor``
``film_aggregate``          ``(Tensor h, Tensor? g, Tensor? residual, Tensor rowptr, Tensor col,
                            Tensor? edge_id, Tensor rel, Tensor? scale, int num_relations,
                            bool relu) -> Tensor``
``rgat_aggregate``          ``(Tensor p, Tensor? qi, Tensor? kj, Tensor? b, Tensor rowptr,
                            Tensor col, Tensor rel, int num_relations, int heads,
                            float negative_slope, bool within) -> (Tensor, Tensor)``
``graph_norm``              ``(Tensor x, Tensor ptr, Tensor? weight, Tensor? bias,
                            Tensor? mean_scale, float eps, str mode, bool std_eps)
                            -> (Tensor y, Tensor mean, Tensor rstd)``
``hop``                     ``(Tensor rowptr, Tensor col, Tensor? edge_id, Tensor? w, Tensor x,
                            float a, Tensor? y, float b, Tensor? z, float c) -> Tensor``
==========================  ===========================================================
"""
from typing import List, Optional, Tuple

import torch
from torch import Tensor
from torch.library import custom_op, register_autograd

from . import _native, _onepass
from ._onepass import Slots, _rows

_DEV = 'cuda'
_REDUCES = ('sum', 'mean', 'min', 'max', 'mul')


# ---- integer side (no gradients) ---------------------------------------------------------------
@custom_op('pyg_amd::index_sort', mutates_args=(), device_types=_DEV)
def index_sort(inputs: Tensor, max_value: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    return _native.index_sort(inputs, max_value)


@index_sort.register_fake
def _(inputs, max_value=None):
    return torch.empty_like(inputs), torch.empty(inputs.shape, dtype=torch.int64,
                                                 device=inputs.device)


@custom_op('pyg_amd::index2ptr', mutates_args=(), device_types=_DEV)
def index2ptr(index: Tensor, size: int) -> Tensor:
    return _native.index2ptr(index, size)


@index2ptr.register_fake
def _(index, size):
    return index.new_empty(size + 1)


@custom_op('pyg_amd::ptr2index', mutates_args=(), device_types=_DEV)
def ptr2index(ptr: Tensor, n: int) -> Tensor:
    return _native.ptr2index(ptr, n)


@ptr2index.register_fake
def _(ptr, n):
    return ptr.new_empty(n)


# ---- gather / scatter ----------------------------------------------------------------------------
@custom_op('pyg_amd::gather', mutates_args=(), device_types=_DEV)
def gather(x: Tensor, index: Tensor) -> Tensor:
    out = _native.gather_rows(_rows(x), index)
    return out.reshape(index.numel(), *x.shape[1:])


@gather.register_fake
def _(x, index):
    return x.new_empty(index.numel(), *x.shape[1:])


@custom_op('pyg_amd::scatter', mutates_args=(), device_types=_DEV)
def scatter(src: Tensor, index: Tensor, dim_size: int, reduce: str) -> Tensor:
    if reduce not in _REDUCES:
        raise ValueError(f"Encountered invalid `reduce` argument '{reduce}'")
    out = _native.scatter_rows(_rows(src), index, dim_size, reduce)
    return out.reshape(dim_size, *src.shape[1:])


@scatter.register_fake
def _(src, index, dim_size, reduce):
    return src.new_empty(dim_size, *src.shape[1:])


@custom_op('pyg_amd::scatter_backward', mutates_args=(), device_types=_DEV)
def scatter_backward(grad: Tensor, src: Tensor, index: Tensor, out: Tensor,
                     reduce: str) -> Tensor:
    g2 = _rows(grad).contiguous()
    s2 = _rows(src)
    if reduce == 'sum':
        res = _native.gather_rows(g2, index)
    elif reduce == 'mean':
        ones = torch.ones(index.numel(), 1, dtype=torch.float32, device=src.device)
        cnt = _native.scatter_rows(ones, index, grad.size(0), 'sum').clamp_(min=1)
        res = _native.gather_rows(g2 / cnt, index)
    elif reduce in ('min', 'max'):
        res = _native.scatter_minmax_backward(s2, index, _rows(out), g2)
    else:
        res = _native.scatter_mul_backward(s2, index, _rows(out), g2)
    return res.reshape(src.shape)


@scatter_backward.register_fake
def _(grad, src, index, out, reduce):
    return torch.empty_like(src)


def _scatter_setup(ctx, inputs, output):
    src, index, dim_size, reduce = inputs
    ctx.reduce = reduce
    ctx.save_for_backward(src, index, output)


def _scatter_bwd(ctx, grad):
    src, index, out = ctx.saved_tensors
    return scatter_backward(grad, src, index, out, ctx.reduce), None, None, None


register_autograd('pyg_amd::scatter', _scatter_bwd, setup_context=_scatter_setup)


def _gather_setup(ctx, inputs, output):
    x, index = inputs
    ctx.n = x.size(0)
    ctx.save_for_backward(index)


def _gather_bwd(ctx, grad):
    (index, ) = ctx.saved_tensors
    return scatter(grad.contiguous(), index, ctx.n, 'sum'), None


register_autograd('pyg_amd::gather', _gather_bwd, setup_context=_gather_setup)


# ---- segment_csr / softmax_csr -------------------------------------------------------------------
@custom_op('pyg_amd::segment_csr', mutates_args=(), device_types=_DEV)
def segment_csr(src: Tensor, ptr: Tensor, reduce: str) -> Tensor:
    if reduce not in ('sum', 'mean', 'min', 'max'):
        raise ValueError(f"Encountered invalid `reduce` argument '{reduce}'")
    n_seg = ptr.numel() - 1
    out = _native.spmm_csr(ptr, None, _rows(src), reduce, n_rows=n_seg)
    return out.reshape(n_seg, *src.shape[1:])


@segment_csr.register_fake
def _(src, ptr, reduce):
    return src.new_empty(ptr.numel() - 1, *src.shape[1:])


@custom_op('pyg_amd::segment_csr_backward', mutates_args=(), device_types=_DEV)
def segment_csr_backward(grad: Tensor, src: Tensor, ptr: Tensor, out: Tensor,
                         reduce: str) -> Tensor:
    n = src.size(0)
    g2 = _rows(grad).contiguous()
    index = _native.ptr2index(ptr, n)
    if reduce in ('min', 'max'):
        s2, o2 = src.reshape(n, -1), _rows(out)
        ntie = _native.spmm_tie_count(ptr, None, s2, o2, count_self=False)
        o_e = _native.gather_rows(o2, index)
        # (ATen averages over ties only where the gradient is positive — see SegmentFunction)
        g_e = _native.gather_rows(torch.where(g2 > 0, g2 / ntie.clamp(min=1), g2), index)
        res = torch.where(s2 == o_e, g_e, torch.zeros_like(g_e))
    else:
        if reduce == 'mean':
            g2 = g2 / (ptr[1:] - ptr[:-1]).clamp(min=1).to(torch.float32).view(-1, 1)
        res = _native.gather_rows(g2, index)
    return res.reshape(src.shape)


@segment_csr_backward.register_fake
def _(grad, src, ptr, out, reduce):
    return torch.empty_like(src)


def _segment_setup(ctx, inputs, output):
    src, ptr, reduce = inputs
    ctx.reduce = reduce
    ctx.save_for_backward(src, ptr, output)


def _segment_bwd(ctx, grad):
    src, ptr, out = ctx.saved_tensors
    return segment_csr_backward(grad, src, ptr, out, ctx.reduce), None, None


register_autograd('pyg_amd::segment_csr', _segment_bwd, setup_context=_segment_setup)


@custom_op('pyg_amd::softmax_csr', mutates_args=(), device_types=_DEV)
def softmax_csr(src: Tensor, ptr: Tensor) -> Tensor:
    out = _native.segment_softmax_forward(_rows(src), ptr)
    return out.reshape(src.shape)


@softmax_csr.register_fake
def _(src, ptr):
    return torch.empty_like(src)


@custom_op('pyg_amd::softmax_csr_backward', mutates_args=(), device_types=_DEV)
def softmax_csr_backward(out: Tensor, grad: Tensor, ptr: Tensor) -> Tensor:
    o2 = _rows(out)
    return _native.segment_softmax_backward(o2, grad.reshape(o2.shape), ptr).reshape(out.shape)


@softmax_csr_backward.register_fake
def _(out, grad, ptr):
    return torch.empty_like(out)


def _softmax_setup(ctx, inputs, output):
    ctx.save_for_backward(output, inputs[1])


def _softmax_bwd(ctx, grad):
    out, ptr = ctx.saved_tensors
    return softmax_csr_backward(out, grad.contiguous(), ptr), None


register_autograd('pyg_amd::softmax_csr', _softmax_bwd, setup_context=_softmax_setup)


# ---- spmm on a CSR pair (rows = destinations) ---------------------------------------------------------
@custom_op('pyg_amd::spmm', mutates_args=(), device_types=_DEV)
def spmm(rowptr: Tensor, col: Tensor, value: Optional[Tensor], other: Tensor,
         reduce: str) -> Tensor:
    if reduce not in ('sum', 'mean', 'min', 'max'):
        raise ValueError(f"`reduce` argument '{reduce}' not supported")
    if value is not None and reduce in ('min', 'max'):
        raise NotImplementedError('edge weights are not supported for min/max')
    n_rows = rowptr.numel() - 1
    out = _native.spmm_csr(rowptr, col, _rows(other), reduce, n_rows=n_rows,
                           w=value, hub=_native.hub_plan(rowptr))
    return out.reshape(n_rows, *other.shape[1:])


@spmm.register_fake
def _(rowptr, col, value, other, reduce):
    return other.new_empty(rowptr.numel() - 1, *other.shape[1:])


@custom_op('pyg_amd::spmm_backward', mutates_args=(), device_types=_DEV)
def spmm_backward(grad: Tensor, rowptr: Tensor, col: Tensor, value: Optional[Tensor],
                  other: Tensor, out: Tensor, reduce: str, need_other: bool,
                  need_value: bool) -> Tuple[Tensor, Tensor]:
    n_rows = rowptr.numel() - 1
    g2 = grad.reshape(n_rows, -1).contiguous()
    o2 = _rows(other)
    g_other = other.new_empty(0)
    g_value = other.new_empty(0)
    if reduce in ('min', 'max'):
        if need_other:
            g_other = _native.spmm_minmax_backward_dst(rowptr, col, o2, out.reshape(n_rows, -1),
                                                       g2, other.size(0)).reshape(other.shape)
        return g_other, g_value
    if reduce == 'mean':
        inv = 1.0 / (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(torch.float32)
        g2 = g2 * inv.view(-1, 1)
    if need_other:
        # edge-parallel transposed product on the CSR's own slots (no second sort): atomics
        dst = _native.ptr2index(rowptr, col.numel())
        g_other = _native.gather_scatter_add(g2, dst, col, other.size(0),
                                             w=value).reshape(other.shape)
    if need_value and value is not None:
        g_value = _native.sddmm_csr(rowptr, col, None, g2, o2, col.numel(), 1).reshape(value.shape)
    return g_other, g_value


@spmm_backward.register_fake
def _(grad, rowptr, col, value, other, out, reduce, need_other, need_value):
    g_other = torch.empty_like(other) if need_other else other.new_empty(0)
    g_value = (torch.empty_like(value) if (need_value and value is not None)
               else other.new_empty(0))
    return g_other, g_value


def _spmm_setup(ctx, inputs, output):
    rowptr, col, value, other, reduce = inputs
    ctx.reduce, ctx.has_value = reduce, value is not None
    ctx.save_for_backward(rowptr, col, value, other, output)


def _spmm_bwd(ctx, grad):
    rowptr, col, value, other, out = ctx.saved_tensors
    need_other, need_value = ctx.needs_input_grad[3], ctx.needs_input_grad[2] and ctx.has_value
    g_other, g_value = spmm_backward(grad.contiguous(), rowptr, col, value, other, out,
                                     ctx.reduce, need_other, need_value)
    return None, None, (g_value if need_value else None), (g_other if need_other else None), None


register_autograd('pyg_amd::spmm', _spmm_bwd, setup_context=_spmm_setup)


# ---- dense transform ----------------------------------------------------------------------------------
@custom_op('pyg_amd::linear', mutates_args=(), device_types=_DEV)
def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    out = _native.linear_forward(x.reshape(-1, x.size(-1)), weight, bias)
    return out.reshape(*x.shape[:-1], weight.size(0))


@linear.register_fake
def _(x, weight, bias=None):
    return x.new_empty(*x.shape[:-1], weight.size(0))


@custom_op('pyg_amd::linear_backward', mutates_args=(), device_types=_DEV)
def linear_backward(grad: Tensor, x: Tensor, weight: Tensor, need_x: bool, need_w: bool,
                    need_b: bool) -> Tuple[Tensor, Tensor, Tensor]:
    g2 = grad.reshape(-1, grad.size(-1)).contiguous()
    x2 = x.reshape(-1, x.size(-1))
    empty = x.new_empty(0)
    gx = (_native.linear_dgrad(g2, weight.t().contiguous()).reshape(x.shape) if need_x
          else empty)
    gw = gb = empty
    if need_w:
        gw = _native.linear_wgrad(g2, x2, bias_grad=need_b)
        if need_b:
            gw, gb = gw
    elif need_b:
        gb = _native.colsum(g2)
    return gx, gw, gb


@linear_backward.register_fake
def _(grad, x, weight, need_x, need_w, need_b):
    e = x.new_empty(0)
    return (torch.empty_like(x) if need_x else e, torch.empty_like(weight) if need_w else e,
            x.new_empty(weight.size(0)) if need_b else e)


def _linear_setup(ctx, inputs, output):
    x, weight, bias = inputs
    ctx.has_bias = bias is not None
    ctx.save_for_backward(x, weight)


def _linear_bwd(ctx, grad):
    x, weight = ctx.saved_tensors
    nx, nw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    nb = ctx.has_bias and ctx.needs_input_grad[2]
    gx, gw, gb = linear_backward(grad.contiguous(), x, weight, nx, nw, nb)
    return (gx if nx else None), (gw if nw else None), (gb if nb else None)


register_autograd('pyg_amd::linear', _linear_bwd, setup_context=_linear_setup)

# ---- GATv2 attention on a CSR pair (rows = destinations) -----------------------------------------
@custom_op('pyg_amd::gatv2_attend', mutates_args=(), device_types=_DEV)
def gatv2_attend(x_l: Tensor, x_r: Tensor, att: Tensor, rowptr: Tensor, col: Tensor,
                 negative_slope: float) -> Tuple[Tensor, Tensor]:
    """``(out [n_dst, H, C], alpha [nnz, H])`` of one GATv2 attention step (gatv2_conv.py:358-378)
    for ``x_l [n_src, H, C]``, ``x_r [>= n_dst, H, C]``, ``att`` with ``H * C`` entries; ``alpha``
    follows the slots of ``col`` and is returned for inspection (gradients flow through ``out``)."""
    _, H, C = x_l.shape
    if not _native.gatv2_supported(H, C):
        raise NotImplementedError(f'gatv2_attend serves H * C <= 512 and H <= 64 (got {H} x {C})')
    alpha, out = _native.gatv2_forward(rowptr, col, _rows(x_l), _rows(x_r), att, H, C,
                                       negative_slope, hub=_native.hub_plan(rowptr))
    return out.reshape(rowptr.numel() - 1, H, C), alpha


@gatv2_attend.register_fake
def _(x_l, x_r, att, rowptr, col, negative_slope):
    return (x_l.new_empty(rowptr.numel() - 1, *x_l.shape[1:]),
            x_l.new_empty(col.numel(), x_l.shape[1]))


@custom_op('pyg_amd::gatv2_attend_backward', mutates_args=(), device_types=_DEV)
def gatv2_attend_backward(grad: Tensor, x_l: Tensor, x_r: Tensor, att: Tensor, alpha: Tensor,
                          out: Tensor, rowptr: Tensor, col: Tensor,
                          negative_slope: float) -> Tuple[Tensor, Tensor, Tensor]:
    _, H, C = x_l.shape
    g_l, g_r, g_att = _onepass.gatv2_backward(
        Slots.of_csr(rowptr, col, x_l.size(0)), _rows(x_l), _rows(x_r), att, alpha, H, C,
        negative_slope, grad_out=_rows(grad).contiguous(), out=_rows(out))
    return g_l.reshape(x_l.shape), g_r.reshape(x_r.shape), g_att.reshape(att.shape)


@gatv2_attend_backward.register_fake
def _(grad, x_l, x_r, att, alpha, out, rowptr, col, negative_slope):
    return torch.empty_like(x_l), torch.empty_like(x_r), torch.empty_like(att)


def _gatv2_setup(ctx, inputs, output):
    x_l, x_r, att, rowptr, col, slope = inputs
    ctx.slope = slope
    ctx.save_for_backward(x_l, x_r, att, output[1], output[0], rowptr, col)


def _gatv2_bwd(ctx, grad, _grad_alpha):
    x_l, x_r, att, alpha, out, rowptr, col = ctx.saved_tensors
    g_l, g_r, g_att = gatv2_attend_backward(grad.contiguous(), x_l, x_r, att, alpha, out, rowptr,
                                            col, ctx.slope)
    return g_l, g_r, g_att, None, None, None


register_autograd('pyg_amd::gatv2_attend', _gatv2_bwd, setup_context=_gatv2_setup)

# ---- HAN's typed additive attention on a stacked CSR pair (rows = (edge type, destination)) -------
@custom_op('pyg_amd::han_attend', mutates_args=(), device_types=_DEV)
def han_attend(x_all: Tensor, a_src: Tensor, a_dst: Tensor, rowptr: Tensor, col: Tensor,
               row_begin: List[int], src_begin: List[int], val_shift: List[int],
               negative_slope: float, relu: bool) -> Tuple[Tensor, Tensor]:
    """``(out [n_rows, H * D], alpha [nnz, H])`` of HAN's node-level attention (han_conv.py:170-179)
    for every edge type of a call: rows ``row_begin[e] + i`` are the destinations of edge type
    ``e``, columns ``src_begin[e] + j`` its sources, which read row ``col + val_shift[e]`` of
    ``x_all [S, H, D]``; ``a_src [n_cols, H]`` / ``a_dst [n_rows, H]`` are the stacked logits.
    ``alpha`` follows the slots of ``col`` and is returned for inspection (gradients flow through
    ``out``).  ``col`` must hold ids below ``src_begin[-1]``."""
    _, H, C = x_all.shape
    if not _native.han_supported(H, C):
        raise NotImplementedError(f'han_attend serves H * D <= 512 and H <= 64 (got {H} x {C})')
    n_rows = rowptr.numel() - 1
    _onepass.han_check_types((row_begin, src_begin, val_shift), n_rows, a_src.size(0),
                             x_all.size(0))
    alpha, out = _native.han_forward(rowptr, col, row_begin, val_shift, _rows(x_all), a_src, a_dst,
                                     H, C, negative_slope, relu, hub=_native.hub_plan(rowptr))
    return out, alpha


@han_attend.register_fake
def _(x_all, a_src, a_dst, rowptr, col, row_begin, src_begin, val_shift, negative_slope, relu):
    return (x_all.new_empty(rowptr.numel() - 1, x_all.shape[1] * x_all.shape[2]),
            x_all.new_empty(col.numel(), x_all.shape[1]))


@custom_op('pyg_amd::han_attend_backward', mutates_args=(), device_types=_DEV)
def han_attend_backward(grad: Tensor, x_all: Tensor, a_src: Tensor, a_dst: Tensor, alpha: Tensor,
                        out: Tensor, rowptr: Tensor, col: Tensor, row_begin: List[int],
                        src_begin: List[int], val_shift: List[int], negative_slope: float,
                        relu: bool) -> Tuple[Tensor, Tensor, Tensor]:
    _, H, C = x_all.shape
    g_x, g_src, g_dst = _onepass.han_backward(
        Slots.of_csr(rowptr, col, a_src.size(0)), (row_begin, src_begin, val_shift), _rows(x_all),
        a_src, a_dst, alpha, out, grad.contiguous(), H, C, negative_slope, relu)
    return g_x.reshape(x_all.shape), g_src, g_dst


@han_attend_backward.register_fake
def _(grad, x_all, a_src, a_dst, alpha, out, rowptr, col, row_begin, src_begin, val_shift,
      negative_slope, relu):
    return torch.empty_like(x_all), torch.empty_like(a_src), torch.empty_like(a_dst)


def _han_setup(ctx, inputs, output):
    x_all, a_src, a_dst, rowptr, col, row_begin, src_begin, val_shift, slope, relu = inputs
    ctx.static = (list(row_begin), list(src_begin), list(val_shift), slope, relu)
    ctx.save_for_backward(x_all, a_src, a_dst, output[1], output[0], rowptr, col)


def _han_bwd(ctx, grad, _grad_alpha):
    x_all, a_src, a_dst, alpha, out, rowptr, col = ctx.saved_tensors
    g_x, g_src, g_dst = han_attend_backward(grad.contiguous(), x_all, a_src, a_dst, alpha, out,
                                            rowptr, col, *ctx.static)
    return g_x, g_src, g_dst, None, None, None, None, None, None, None


register_autograd('pyg_amd::han_attend', _han_bwd, setup_context=_han_setup)

# ---- TransformerConv's dot-product attention on a CSR pair (rows = destinations) ------------------
@custom_op('pyg_amd::transformer_attend', mutates_args=(), device_types=_DEV)
def transformer_attend(query: Tensor, key: Tensor, value: Tensor, rowptr: Tensor, col: Tensor,
                       scale: float) -> Tuple[Tensor, Tensor]:
    """``(out [n_dst, H, C], alpha [nnz, H])`` of one dot-product attention step
    (transformer_conv.py:263-283) for ``query [>= n_dst, H, C]`` and ``key``, ``value
    [n_src, H, C]``; ``alpha`` follows the slots of ``col`` and is returned for inspection
    (gradients flow through ``out``)."""
    _, H, C = query.shape
    if not _native.transformer_supported(H, C):
        raise NotImplementedError(
            f'transformer_attend serves H * C <= 512 and H <= 64 (got {H} x {C})')
    alpha, out = _native.transformer_forward(rowptr, col, _rows(query), _rows(key), _rows(value),
                                             H, C, scale, hub=_native.hub_plan(rowptr))
    return out.reshape(rowptr.numel() - 1, H, C), alpha


@transformer_attend.register_fake
def _(query, key, value, rowptr, col, scale):
    return (query.new_empty(rowptr.numel() - 1, *query.shape[1:]),
            query.new_empty(col.numel(), query.shape[1]))


@custom_op('pyg_amd::transformer_attend_backward', mutates_args=(), device_types=_DEV)
def transformer_attend_backward(grad: Tensor, query: Tensor, key: Tensor, value: Tensor,
                                alpha: Tensor, out: Tensor, rowptr: Tensor, col: Tensor,
                                scale: float) -> Tuple[Tensor, Tensor, Tensor]:
    _, H, C = query.shape
    g_q, g_k, g_v, _, _ = _onepass.transformer_backward(
        Slots.of_csr(rowptr, col, key.size(0)), _rows(query), _rows(key), _rows(value), alpha, H,
        C, scale, grad_out=_rows(grad).contiguous(), out=_rows(out))
    return g_q.reshape(query.shape), g_k.reshape(key.shape), g_v.reshape(value.shape)


@transformer_attend_backward.register_fake
def _(grad, query, key, value, alpha, out, rowptr, col, scale):
    return torch.empty_like(query), torch.empty_like(key), torch.empty_like(value)


def _transformer_setup(ctx, inputs, output):
    query, key, value, rowptr, col, scale = inputs
    ctx.scale = scale
    ctx.save_for_backward(query, key, value, output[1], output[0], rowptr, col)


def _transformer_bwd(ctx, grad, _grad_alpha):
    query, key, value, alpha, out, rowptr, col = ctx.saved_tensors
    g_q, g_k, g_v = transformer_attend_backward(grad.contiguous(), query, key, value, alpha, out,
                                                rowptr, col, ctx.scale)
    return g_q, g_k, g_v, None, None, None


register_autograd('pyg_amd::transformer_attend', _transformer_bwd,
                  setup_context=_transformer_setup)


# ---- ... with edge features inside the kernel (rows = destinations, edge_attr follows `col`) -----
@custom_op('pyg_amd::transformer_edge_attend', mutates_args=(), device_types=_DEV)
def transformer_edge_attend(query: Tensor, key: Tensor, value: Tensor, edge_attr: Tensor,
                            bias: Tensor, rowptr: Tensor, col: Tensor,
                            scale: float) -> Tuple[Tensor, Tensor, Tensor]:
    """``(out [n_dst, H, C], z [n_dst, H, De], alpha [nnz, H])`` of one dot-product attention step
    with edge features (transformer_conv.py:263-283): ``s = scale <q, key_j> + <bias[i, h], a_k>``
    for ``edge_attr [nnz, De]`` in the order of ``col`` and ``bias [>= n_dst, H, De]``; ``out`` is
    the weighted sum of ``value`` alone and ``z`` that of the raw edge features."""
    _, H, C = query.shape
    De = edge_attr.size(1)
    if not _native.transformer_edge_supported(H, C, De):
        raise NotImplementedError(
            f'transformer_edge_attend serves H * C <= 512, H <= 64 and De <= 4 * (64 // H rounded '
            f'down to a power of two) (got {H} x {C}, De = {De})')
    alpha, out, z = _native.transformer_edge_forward(
        rowptr, col, _rows(query), _rows(key), _rows(value), edge_attr, _rows(bias), H, C, scale,
        hub=_native.hub_plan(rowptr))
    n = rowptr.numel() - 1
    return out.reshape(n, H, C), z.reshape(n, H, De), alpha


@transformer_edge_attend.register_fake
def _(query, key, value, edge_attr, bias, rowptr, col, scale):
    n = rowptr.numel() - 1
    return (query.new_empty(n, *query.shape[1:]),
            query.new_empty(n, query.shape[1], edge_attr.shape[1]),
            query.new_empty(col.numel(), query.shape[1]))


@custom_op('pyg_amd::transformer_edge_attend_backward', mutates_args=(), device_types=_DEV)
def transformer_edge_attend_backward(grad: Tensor, grad_z: Tensor, query: Tensor, key: Tensor,
                                     value: Tensor, edge_attr: Tensor, bias: Tensor,
                                     alpha: Tensor, out: Tensor, z: Tensor, rowptr: Tensor,
                                     col: Tensor, scale: float
                                     ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    _, H, C = query.shape
    g_q, g_k, g_v, g_b, g_a = _onepass.transformer_backward(
        Slots.of_csr(rowptr, col, key.size(0)), _rows(query), _rows(key), _rows(value), alpha, H,
        C, scale, grad_out=_rows(grad).contiguous(), out=_rows(out), edge_attr=edge_attr,
        bias=_rows(bias), grad_z=_rows(grad_z).contiguous(), z=_rows(z))
    return (g_q.reshape(query.shape), g_k.reshape(key.shape), g_v.reshape(value.shape), g_a,
            g_b.reshape(bias.shape))


@transformer_edge_attend_backward.register_fake
def _(grad, grad_z, query, key, value, edge_attr, bias, alpha, out, z, rowptr, col, scale):
    return (torch.empty_like(query), torch.empty_like(key), torch.empty_like(value),
            torch.empty_like(edge_attr), torch.empty_like(bias))


def _transformer_edge_setup(ctx, inputs, output):
    query, key, value, edge_attr, bias, rowptr, col, scale = inputs
    ctx.scale = scale
    ctx.save_for_backward(query, key, value, edge_attr, bias, output[2], output[0], output[1],
                          rowptr, col)


def _transformer_edge_bwd(ctx, grad, grad_z, _grad_alpha):
    query, key, value, edge_attr, bias, alpha, out, z, rowptr, col = ctx.saved_tensors
    g_q, g_k, g_v, g_a, g_b = transformer_edge_attend_backward(
        grad.contiguous(), grad_z.contiguous(), query, key, value, edge_attr, bias, alpha, out, z,
        rowptr, col, ctx.scale)
    return g_q, g_k, g_v, g_a, g_b, None, None, None


register_autograd('pyg_amd::transformer_edge_attend', _transformer_edge_bwd,
                  setup_context=_transformer_edge_setup)


# ---- GINEConv's aggregation on a CSR pair (rows = destinations) ------------------------------------
@custom_op('pyg_amd::gine_aggregate', mutates_args=(), device_types=_DEV)
def gine_aggregate(x_src: Tensor, x_root: Optional[Tensor], eps: Optional[Tensor],
                   edge_attr: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                   rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor]) -> Tensor:
    """``out [n_dst, F] = (1 + eps) * x_root[:n_dst] + sum_k relu(x_src[col[k]] + e_k)``
    (gin_conv.py:185-207) with ``e_k = edge_attr[edge_id[k]]`` for ``edge_attr [E, F]``, or
    ``weight @ edge_attr[edge_id[k]] + bias`` for ``edge_attr [E, De]`` and ``weight [F, De]``.
    ``edge_id=None``: ``edge_attr`` follows the slots of ``col``.  The by-source form the backward
    walks is built from ``(rowptr, col)`` there, as the attention operators do."""
    F = x_src.size(1)
    De = 0 if weight is None else edge_attr.size(1)
    if not _native.gine_supported(F, De):
        raise NotImplementedError(
            f'gine_aggregate serves F <= 512 and, with a weight, De <= 32 and F * De <= 4096 '
            f'(got F = {F}, De = {De})')
    return _native.gine_forward(rowptr, col, edge_id, x_src, x_root,
                                None if eps is None else eps.reshape(1), edge_attr, weight, bias,
                                hub=_native.hub_plan(rowptr))


@gine_aggregate.register_fake
def _(x_src, x_root, eps, edge_attr, weight, bias, rowptr, col, edge_id):
    return x_src.new_empty(rowptr.numel() - 1, x_src.shape[1])


@custom_op('pyg_amd::gine_aggregate_backward', mutates_args=(), device_types=_DEV)
def gine_aggregate_backward(grad: Tensor, x_src: Tensor, x_root: Optional[Tensor],
                            eps: Optional[Tensor], edge_attr: Tensor, weight: Optional[Tensor],
                            bias: Optional[Tensor], rowptr: Tensor, col: Tensor,
                            edge_id: Optional[Tensor]
                            ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The gradients of ``(x_src, x_root, eps, edge_attr, weight, bias)``; an input that was not
    given gets an empty tensor."""
    grads = _onepass.gine_backward(Slots.of_csr(rowptr, col, x_src.size(0), edge_id), x_src,
                                   x_root, eps, edge_attr, weight, bias, grad)
    # (one empty tensor EACH: an operator's outputs must not alias one another)
    return tuple(grad.new_empty(0) if g is None else g for g in grads)


@gine_aggregate_backward.register_fake
def _(grad, x_src, x_root, eps, edge_attr, weight, bias, rowptr, col, edge_id):
    none = grad.new_empty(0)
    return (torch.empty_like(x_src), none if x_root is None else torch.empty_like(x_root),
            none if eps is None or x_root is None else torch.empty_like(eps),
            torch.empty_like(edge_attr), none if weight is None else torch.empty_like(weight),
            none if bias is None else torch.empty_like(bias))


def _gine_setup(ctx, inputs, output):
    x_src, x_root, eps, edge_attr, weight, bias, rowptr, col, edge_id = inputs
    ctx.given = (x_root is not None, eps is not None and x_root is not None, weight is not None,
                 bias is not None)
    ctx.save_for_backward(x_src, x_root, eps, edge_attr, weight, bias, rowptr, col, edge_id)


def _gine_bwd(ctx, grad):
    x_src, x_root, eps, edge_attr, weight, bias, rowptr, col, edge_id = ctx.saved_tensors
    g_x, g_root, g_eps, g_a, g_w, g_b = gine_aggregate_backward(
        grad.contiguous(), x_src, x_root, eps, edge_attr, weight, bias, rowptr, col, edge_id)
    has_root, has_eps, has_w, has_b = ctx.given
    return (g_x, g_root if has_root else None, g_eps if has_eps else None, g_a,
            g_w if has_w else None, g_b if has_b else None, None, None, None)


register_autograd('pyg_amd::gine_aggregate', _gine_bwd, setup_context=_gine_setup)


# ---- PNAConv's multi-statistic aggregation on a CSR pair (rows = destinations) ---------------------
def _pna_stats(stats: int):
    if not 1 <= stats <= 15:
        raise ValueError(f"'stats' is a non-empty bit set of 1 mean, 2 min, 4 max, 8 std (got {stats})")
    return tuple(s for q, s in enumerate(_native.PNA_STATS) if stats >> q & 1)


@custom_op('pyg_amd::pna_aggregate', mutates_args=(), device_types=_DEV)
def pna_aggregate(p_src: Tensor, p_dst: Tensor, edge_attr: Optional[Tensor],
                  wc: Optional[Tensor], rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor],
                  stats: int) -> Tuple[Tensor, Tensor]:
    """The statistics of PNAConv's linear message (pna_conv.py:175-188, aggr/scaler.py:82):
    ``out [n_stats, n_dst, W]``, the planes selected by the bit set ``stats`` (1 mean, 2 min, 4
    max, 8 std, in that order) of ``p_dst[i] + u_k`` with ``u_k = p_src[col[k]] + wc @
    edge_attr[edge_id[k]]`` (``edge_attr`` and ``wc`` None: ``u_k = p_src[col[k]]``), exactly 0 for
    rows without slots; and ``saved [6, n_dst, W]``, the planes the backward reads (no gradient
    flows through them).  ``edge_id=None``: ``edge_attr`` follows the slots of ``col``."""
    W = p_src.size(1)
    De = 0 if wc is None else wc.size(1)
    if not _native.pna_supported(W, De):
        raise NotImplementedError(
            f'pna_aggregate serves W <= 512 and, with edge features, De <= 32 and W * De <= 4096 '
            f'(got W = {W}, De = {De})')
    return _native.pna_forward(rowptr, col, edge_id, p_src, p_dst, edge_attr, wc,
                               _pna_stats(stats), hub=_native.hub_plan(rowptr))


@pna_aggregate.register_fake
def _(p_src, p_dst, edge_attr, wc, rowptr, col, edge_id, stats):
    n, W = rowptr.numel() - 1, p_src.shape[1]
    return p_src.new_empty(bin(stats).count('1'), n, W), p_src.new_empty(6, n, W)


@custom_op('pyg_amd::pna_aggregate_backward', mutates_args=(), device_types=_DEV)
def pna_aggregate_backward(grad: Tensor, p_src: Tensor, p_dst: Tensor,
                           edge_attr: Optional[Tensor], wc: Optional[Tensor], saved: Tensor,
                           rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor],
                           stats: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The gradients of ``(p_src, p_dst, edge_attr, wc)`` from ``grad [n_stats, n_dst, W]``; an
    input that was not given gets an empty tensor."""
    grads = _onepass.pna_backward(Slots.of_csr(rowptr, col, p_src.size(0), edge_id), p_src,
                                  edge_attr, wc, saved, _pna_stats(stats), grad.unbind(0),
                                  p_dst.size(0))
    # (one empty tensor EACH: an operator's outputs must not alias one another)
    return tuple(grad.new_empty(0) if g is None else g for g in grads)


@pna_aggregate_backward.register_fake
def _(grad, p_src, p_dst, edge_attr, wc, saved, rowptr, col, edge_id, stats):
    none = grad.new_empty(0)
    return (torch.empty_like(p_src, memory_format=torch.contiguous_format),
            torch.empty_like(p_dst, memory_format=torch.contiguous_format),
            none if edge_attr is None else torch.empty_like(edge_attr),
            none if wc is None else torch.empty_like(wc))


def _pna_setup(ctx, inputs, output):
    p_src, p_dst, edge_attr, wc, rowptr, col, edge_id, stats = inputs
    ctx.stats = stats
    ctx.given = edge_attr is not None
    ctx.save_for_backward(p_src, p_dst, edge_attr, wc, output[1], rowptr, col, edge_id)


def _pna_bwd(ctx, grad, _grad_saved):
    p_src, p_dst, edge_attr, wc, saved, rowptr, col, edge_id = ctx.saved_tensors
    g_src, g_dst, g_a, g_wc = pna_aggregate_backward(
        grad.contiguous(), p_src, p_dst, edge_attr, wc, saved, rowptr, col, edge_id, ctx.stats)
    return (g_src, g_dst, g_a if ctx.given else None, g_wc if ctx.given else None, None, None,
            None, None)


register_autograd('pyg_amd::pna_aggregate', _pna_bwd, setup_context=_pna_setup)


# ---- GENConv's softmax aggregation on a CSR pair (rows = destinations) -----------------------------
@custom_op('pyg_amd::gen_aggregate', mutates_args=(), device_types=_DEV)
def gen_aggregate(x_src: Tensor, edge_attr: Optional[Tensor], weight: Optional[Tensor],
                  bias: Optional[Tensor], t: Tensor, rowptr: Tensor, col: Tensor,
                  edge_id: Optional[Tensor], eps_msg: float = 1e-7, semi_grad: bool = False,
                  grad_t: bool = False) -> Tuple[Tensor, Tensor]:
    """GENConv's propagate under SoftmaxAggregation (gen_conv.py:213, 231-239; aggr/basic.py:
    205-215): ``out [n_dst, F] = sum_k alpha_k m_k`` with ``m_k = relu(x_src[col[k]] + e_k) +
    eps_msg`` and ``alpha`` the per-column softmax of ``t * m`` over a row's slots; ``e_k`` is 0
    (``edge_attr=None``), ``edge_attr[edge_id[k]]`` for ``edge_attr [E, F]``, or ``weight @
    edge_attr[edge_id[k]] + bias`` for ``edge_attr [E, De]`` and ``weight [F, De]``.  ``t`` holds 1
    or ``F`` values.  Also returned: ``saved [2, n_dst, F]``, the planes the backward reads (no
    gradient flows through them); ``grad_t`` adds the third plane the gradient of ``t`` needs.
    ``semi_grad`` treats the softmax weights as constants in the backward.  ``edge_id=None``:
    ``edge_attr`` follows the slots of ``col``."""
    F = x_src.size(1)
    De = 0 if weight is None else edge_attr.size(1)
    if not _native.gen_supported(F, De):
        raise NotImplementedError(
            f'gen_aggregate serves F <= 512 and, with a weight, De <= 32 and F * De <= 4096 '
            f'(got F = {F}, De = {De})')
    return _native.gen_forward(rowptr, col, edge_id, x_src, edge_attr, weight, bias, t,
                               eps_msg=eps_msg, want_s2=grad_t, hub=_native.hub_plan(rowptr))


@gen_aggregate.register_fake
def _(x_src, edge_attr, weight, bias, t, rowptr, col, edge_id, eps_msg=1e-7, semi_grad=False,
      grad_t=False):
    n, F = rowptr.numel() - 1, x_src.shape[1]
    return x_src.new_empty(n, F), x_src.new_empty(3 if grad_t else 2, n, F)


@custom_op('pyg_amd::gen_aggregate_backward', mutates_args=(), device_types=_DEV)
def gen_aggregate_backward(grad: Tensor, x_src: Tensor, edge_attr: Optional[Tensor],
                           weight: Optional[Tensor], bias: Optional[Tensor], t: Tensor,
                           out: Tensor, saved: Tensor, rowptr: Tensor, col: Tensor,
                           edge_id: Optional[Tensor], eps_msg: float, semi_grad: bool,
                           grad_t: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The gradients of ``(x_src, edge_attr, weight, bias, t)``; an input that was not given, and
    ``t`` without ``grad_t``, gets an empty tensor."""
    grads = _onepass.gen_backward(Slots.of_csr(rowptr, col, x_src.size(0), edge_id), x_src,
                                  edge_attr, weight, bias, t, out, saved, grad, eps_msg=eps_msg,
                                  semi_grad=semi_grad, want_t=grad_t)
    # (one empty tensor EACH: an operator's outputs must not alias one another)
    return tuple(grad.new_empty(0) if g is None else g for g in grads)


@gen_aggregate_backward.register_fake
def _(grad, x_src, edge_attr, weight, bias, t, out, saved, rowptr, col, edge_id, eps_msg,
      semi_grad, grad_t):
    none = grad.new_empty(0)
    return (torch.empty_like(x_src, memory_format=torch.contiguous_format),
            none if edge_attr is None else torch.empty_like(edge_attr),
            none if weight is None else torch.empty_like(weight),
            none if bias is None else torch.empty_like(bias),
            torch.empty_like(t) if grad_t else none)


def _gen_setup(ctx, inputs, output):
    x_src, edge_attr, weight, bias, t, rowptr, col, edge_id, eps_msg, semi_grad, grad_t = inputs
    ctx.static = (eps_msg, semi_grad, grad_t)
    ctx.given = (edge_attr is not None, weight is not None, bias is not None)
    ctx.save_for_backward(x_src, edge_attr, weight, bias, t, output[0], output[1], rowptr, col,
                          edge_id)


def _gen_bwd(ctx, grad, _grad_saved):
    x_src, edge_attr, weight, bias, t, out, saved, rowptr, col, edge_id = ctx.saved_tensors
    g_x, g_a, g_w, g_b, g_t = gen_aggregate_backward(
        grad.contiguous(), x_src, edge_attr, weight, bias, t, out, saved, rowptr, col, edge_id,
        *ctx.static)
    has_a, has_w, has_b = ctx.given
    return (g_x, g_a if has_a else None, g_w if has_w else None, g_b if has_b else None,
            g_t if ctx.static[2] else None, None, None, None, None, None, None)


register_autograd('pyg_amd::gen_aggregate', _gen_bwd, setup_context=_gen_setup)


# ---- ResGatedGraphConv's gated sum on a CSR pair (rows = destinations) --------------------------------
@custom_op('pyg_amd::resgated_aggregate', mutates_args=(), device_types=_DEV)
def resgated_aggregate(k: Tensor, qv: Tensor, edge_attr: Optional[Tensor],
                       w_gate: Optional[Tensor], w_value: Optional[Tensor], rowptr: Tensor,
                       col: Tensor, edge_id: Optional[Tensor]) -> Tensor:
    """ResGatedGraphConv's propagate (res_gated_graph_conv.py:128, 138-148): ``out [n_dst, F] =
    sum_k sigmoid(k[i] + q[col[k]] + w_gate @ a_k) * (v[col[k]] + w_value @ a_k)`` with the packed
    ``qv [n_src, 2F] = [q | v]`` and ``a_k = edge_attr[edge_id[k]]`` (``edge_attr [E, De]`` with
    ``w_gate``, ``w_value [F, De]``, or all three None).  ``edge_id=None``: ``edge_attr`` follows the
    slots of ``col``."""
    F = k.size(1)
    De = 0 if edge_attr is None else edge_attr.size(1)
    if not _native.resgated_supported(F, De):
        raise NotImplementedError(
            f'resgated_aggregate serves F <= 512 and, with edge features, De <= 32 and F * De <= '
            f'2048 (got F = {F}, De = {De})')
    return _native.resgated_forward(rowptr, col, edge_id, k, qv, edge_attr,
                                    _onepass.resgated_weight(w_gate, w_value),
                                    hub=_native.hub_plan(rowptr))


@resgated_aggregate.register_fake
def _(k, qv, edge_attr, w_gate, w_value, rowptr, col, edge_id):
    return k.new_empty(rowptr.numel() - 1, k.shape[1])


@custom_op('pyg_amd::resgated_aggregate_backward', mutates_args=(), device_types=_DEV)
def resgated_aggregate_backward(grad: Tensor, k: Tensor, qv: Tensor, edge_attr: Optional[Tensor],
                                w_gate: Optional[Tensor], w_value: Optional[Tensor],
                                rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor]
                                ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The gradients of ``(k, qv, edge_attr, w_gate, w_value)``; an input that was not given gets
    an empty tensor."""
    grads = _onepass.resgated_backward(Slots.of_csr(rowptr, col, qv.size(0), edge_id), k, qv,
                                       edge_attr, w_gate, w_value, grad)
    # (one tensor EACH, none a view of another: an operator's outputs must not alias)
    return tuple(grad.new_empty(0) if g is None else (g.clone() if g._base is not None else g)
                 for g in grads)


@resgated_aggregate_backward.register_fake
def _(grad, k, qv, edge_attr, w_gate, w_value, rowptr, col, edge_id):
    none = grad.new_empty(0)
    return (torch.empty_like(k, memory_format=torch.contiguous_format),
            torch.empty_like(qv, memory_format=torch.contiguous_format),
            none if edge_attr is None else torch.empty_like(edge_attr),
            none if w_gate is None else torch.empty_like(w_gate),
            grad.new_empty(0) if w_value is None else torch.empty_like(w_value))


def _resgated_setup(ctx, inputs, output):
    k, qv, edge_attr, w_gate, w_value, rowptr, col, edge_id = inputs
    ctx.given = edge_attr is not None
    ctx.save_for_backward(k, qv, edge_attr, w_gate, w_value, rowptr, col, edge_id)


def _resgated_bwd(ctx, grad):
    k, qv, edge_attr, w_gate, w_value, rowptr, col, edge_id = ctx.saved_tensors
    g_k, g_qv, g_a, g_wg, g_wv = resgated_aggregate_backward(
        grad.contiguous(), k, qv, edge_attr, w_gate, w_value, rowptr, col, edge_id)
    if not ctx.given:
        g_a = g_wg = g_wv = None
    return g_k, g_qv, g_a, g_wg, g_wv, None, None, None


register_autograd('pyg_amd::resgated_aggregate', _resgated_bwd, setup_context=_resgated_setup)


# ---- CGConv's gated softplus sum on a CSR pair (rows = destinations) -----------------------------------
def _cg_width(p: Tensor, q: Optional[Tensor]) -> int:
    return p.size(1) // (2 if q is not None else 4)


@custom_op('pyg_amd::cg_aggregate', mutates_args=(), device_types=_DEV)
def cg_aggregate(p: Tensor, q: Optional[Tensor], edge_attr: Optional[Tensor],
                 w_f: Optional[Tensor], w_s: Optional[Tensor], edge_terms: Optional[Tensor],
                 residual: Optional[Tensor], rowptr: Tensor, col: Tensor,
                 edge_id: Optional[Tensor], mean: bool) -> Tensor:
    """CGConv's propagate and residual (cg_conv.py:88-98): ``out [n_dst, F] = residual + aggr_k
    sigmoid(zf_k) * softplus(zs_k)`` with ``[zf_k | zs_k] = p[i] + q[col[k]] +`` the edge terms of
    ``edge_id[k]``: ``p [>= n_dst, 2F]``, ``q [n_src, 2F]`` (or ``q`` None and ``p`` the packed
    ``[n_src, 4F] = [P | Q]``); ``edge_attr [E, De]`` with ``w_f``, ``w_s [F, De]``, or
    ``edge_terms [E, 2F]``, or neither.  ``mean``: divide by the slot count.  ``edge_id=None``:
    the edge tensors follow the slots of ``col``."""
    F = _cg_width(p, q)
    De = 0 if edge_attr is None else edge_attr.size(1)
    if not _native.cg_supported(F, De):
        raise NotImplementedError(
            f'cg_aggregate serves F <= 512 and, with raw edge features, De <= 32 and F * De <= '
            f'2048 (got F = {F}, De = {De}); pass edge_terms [E, 2F] beyond that')
    if edge_terms is not None and edge_attr is not None:
        raise ValueError("'edge_attr' (with 'w_f', 'w_s') and 'edge_terms' exclude each other")
    P, Q = _onepass.cg_split(p, q)
    return _native.cg_forward(rowptr, col, edge_id, P, Q,
                              edge_attr if edge_terms is None else edge_terms,
                              _onepass.cg_weight(w_f, w_s), residual=residual, mean=mean,
                              hub=_native.hub_plan(rowptr))


@cg_aggregate.register_fake
def _(p, q, edge_attr, w_f, w_s, edge_terms, residual, rowptr, col, edge_id, mean):
    return p.new_empty(rowptr.numel() - 1, _cg_width(p, q))


@custom_op('pyg_amd::cg_aggregate_backward', mutates_args=(), device_types=_DEV)
def cg_aggregate_backward(grad: Tensor, p: Tensor, q: Optional[Tensor],
                          edge_attr: Optional[Tensor], w_f: Optional[Tensor],
                          w_s: Optional[Tensor], edge_terms: Optional[Tensor], rowptr: Tensor,
                          col: Tensor, edge_id: Optional[Tensor], mean: bool
                          ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The gradients of ``(p, q, edge_attr, w_f, w_s, edge_terms)``; an input that was not given
    gets an empty tensor.  (The residual's gradient is ``grad`` itself.)"""
    n_src = p.size(0) if q is None else q.size(0)
    grads = _onepass.cg_backward(Slots.of_csr(rowptr, col, n_src, edge_id), p, q, edge_attr, w_f,
                                 w_s, edge_terms, grad, mean=mean)
    # (one tensor EACH, none a view of another: an operator's outputs must not alias)
    return tuple(grad.new_empty(0) if g is None else (g.clone() if g._base is not None else g)
                 for g in grads)


@cg_aggregate_backward.register_fake
def _(grad, p, q, edge_attr, w_f, w_s, edge_terms, rowptr, col, edge_id, mean):
    def like(t):
        return (grad.new_empty(0) if t is None
                else torch.empty_like(t, memory_format=torch.contiguous_format))
    return tuple(like(t) for t in (p, q, edge_attr, w_f, w_s, edge_terms))


def _cg_setup(ctx, inputs, output):
    p, q, edge_attr, w_f, w_s, edge_terms, residual, rowptr, col, edge_id, mean = inputs
    ctx.given = tuple(t is not None for t in (p, q, edge_attr, w_f, w_s, edge_terms))
    ctx.mean, ctx.residual = mean, residual is not None
    ctx.save_for_backward(p, q, edge_attr, w_f, w_s, edge_terms, rowptr, col, edge_id)


def _cg_bwd(ctx, grad):
    p, q, edge_attr, w_f, w_s, edge_terms, rowptr, col, edge_id = ctx.saved_tensors
    grad = grad.contiguous()
    grads = cg_aggregate_backward(grad, p, q, edge_attr, w_f, w_s, edge_terms, rowptr, col,
                                  edge_id, ctx.mean)
    grads = tuple(g if given else None for g, given in zip(grads, ctx.given))
    return grads + (grad if ctx.residual else None, None, None, None, None)


register_autograd('pyg_amd::cg_aggregate', _cg_bwd, setup_context=_cg_setup)


# ---- FiLMConv's typed feature modulation on a CSR pair (rows = destinations) ---------------------------
def _film_forms(h, g, rowptr, col, edge_id, rel, scale, num_relations):
    n_src = h.size(0)
    return _onepass.FilmForms.of_csr(rowptr, col, edge_id, rel, scale, n_src, num_relations)


@custom_op('pyg_amd::film_aggregate', mutates_args=(), device_types=_DEV)
def film_aggregate(h: Tensor, g: Optional[Tensor], residual: Optional[Tensor], rowptr: Tensor,
                   col: Tensor, edge_id: Optional[Tensor], rel: Tensor, scale: Optional[Tensor],
                   num_relations: int, relu: bool) -> Tensor:
    """FiLMConv's per-relation propagates and the sum with the skip term (film_conv.py:128-161):
    ``out [n_dst, F] = residual + sum_k scale[e] * act(gamma * h[col[k], r F:(r + 1) F] + beta)``
    with ``e = edge_id[k]``, ``r = rel[e]`` (int32 ``[E]``, in ``[0, num_relations)``: checked) and
    ``[beta | gamma] = g[i, r * 2F:(r + 1) * 2F]``: ``h [n_src, R * F]``, ``g [>= n_dst, R * 2F]``
    (or ``g`` None and ``h`` the packed ``[n_src, 3 R F] = [H | G]``).  ``scale [E]``: the
    per-edge mean normaliser ``1 / |N_r(i)|`` (None: sum).  ``relu=False``: no activation.
    ``edge_id=None``: ``rel`` and ``scale`` follow the slots of ``col``.  The slots of a row may
    come in any order of relations."""
    R = int(num_relations)
    width = h.size(1) // (R if g is not None else 3 * R)
    if not _native.film_supported(width):
        raise NotImplementedError(f'film_aggregate serves 1 <= F <= 512 (got F = {width})')
    if rel.numel() > 0:
        lo, hi = _native.index_minmax(rel)
        if lo < 0 or hi >= R:
            raise ValueError(f"'rel' must lie in [0, {R}) (got values in [{lo}, {hi}])")
    forms = _film_forms(h, g, rowptr, col, edge_id, rel, scale, R)
    return _onepass.film_forward(forms, h, g, residual, relu)


@film_aggregate.register_fake
def _(h, g, residual, rowptr, col, edge_id, rel, scale, num_relations, relu):
    return h.new_empty(rowptr.numel() - 1,
                       h.size(1) // (num_relations if g is not None else 3 * num_relations))


@custom_op('pyg_amd::film_aggregate_backward', mutates_args=(), device_types=_DEV)
def film_aggregate_backward(grad: Tensor, h: Tensor, g: Optional[Tensor], rowptr: Tensor,
                            col: Tensor, edge_id: Optional[Tensor], rel: Tensor,
                            scale: Optional[Tensor], num_relations: int,
                            relu: bool) -> Tuple[Tensor, Tensor]:
    """The gradients of ``(h, g)``; ``g`` not given gets an empty tensor.  (The residual's
    gradient is ``grad`` itself.)"""
    forms = _film_forms(h, g, rowptr, col, edge_id, rel, scale, num_relations)
    grads = _onepass.film_backward(forms, h, g, grad, relu=relu)
    return tuple(grad.new_empty(0) if t is None else t for t in grads)


@film_aggregate_backward.register_fake
def _(grad, h, g, rowptr, col, edge_id, rel, scale, num_relations, relu):
    return (torch.empty_like(h, memory_format=torch.contiguous_format),
            grad.new_empty(0) if g is None
            else torch.empty_like(g, memory_format=torch.contiguous_format))


def _film_setup(ctx, inputs, output):
    h, g, residual, rowptr, col, edge_id, rel, scale, num_relations, relu = inputs
    ctx.static = (num_relations, relu)
    ctx.given, ctx.residual = g is not None, residual is not None
    ctx.save_for_backward(h, g, rowptr, col, edge_id, rel, scale)


def _film_bwd(ctx, grad):
    h, g, rowptr, col, edge_id, rel, scale = ctx.saved_tensors
    grad = grad.contiguous()
    g_h, g_g = film_aggregate_backward(grad, h, g, rowptr, col, edge_id, rel, scale, *ctx.static)
    return (g_h, g_g if ctx.given else None, grad if ctx.residual else None, None, None, None,
            None, None, None, None)


register_autograd('pyg_amd::film_aggregate', _film_bwd, setup_context=_film_setup)


# ---- RGATConv's additive relational attention on a CSR pair (rows = destinations) ---------------------
def _rgat_dims(p, qi, num_relations, heads):
    R, H = int(num_relations), int(heads)
    width = p.size(1) // R if qi is not None else p.size(1) // R - 2 * H
    if width < H or width % H:
        raise ValueError(f"'p' [., {p.size(1)}] does not hold {R} relations of {H} heads")
    return R, H, width // H


@custom_op('pyg_amd::rgat_aggregate', mutates_args=(), device_types=_DEV)
def rgat_aggregate(p: Tensor, qi: Optional[Tensor], kj: Optional[Tensor], b: Optional[Tensor],
                   rowptr: Tensor, col: Tensor, rel: Tensor, num_relations: int, heads: int,
                   negative_slope: float, within: bool) -> Tuple[Tensor, Tensor]:
    """RGATConv's additive message, softmax and sum (rgat_conv.py:397-437, 500-502): ``(out [n_dst,
    H * C], alpha [nnz, H])`` with ``out[i, h] = sum_k alpha[k, h] * p[col[k], r, h]``, ``alpha``
    the softmax of ``leaky_relu(qi[i, r, h] + kj[col[k], r, h] + b[k, h])`` over the slots of row
    ``i`` (``within``: over those of relation ``r``) and ``r = rel[k]`` (int32 ``[nnz]``, in ``[0,
    num_relations)``: checked): ``p [n_src, R * H * C]``, ``qi`` / ``kj [n_src, R * H]`` (or both
    None and ``p`` the packed ``[n_src, R (H C + 2 H)] = [P | QI | KJ]``).  ``rel``, ``b`` and
    ``alpha`` follow the slots of ``col``, which may come in any order of relations."""
    R, H, C = _rgat_dims(p, qi, num_relations, heads)
    if not _native.rgat_supported(H, C):
        raise NotImplementedError(f'rgat_aggregate serves H * C <= 512 and H <= 64 (got H = {H}, '
                                  f'C = {C})')
    if rel.numel() > 0:
        lo, hi = _native.index_minmax(rel)
        if lo < 0 or hi >= R:
            raise ValueError(f"'rel' must lie in [0, {R}) (got values in [{lo}, {hi}])")
    forms = _onepass.RgatForms.of_csr(rowptr, col, rel, p.size(0), R)
    alpha, out = _onepass.rgat_forward(forms, p, qi, kj, b, H, C, negative_slope, within)
    return out, alpha


@rgat_aggregate.register_fake
def _(p, qi, kj, b, rowptr, col, rel, num_relations, heads, negative_slope, within):
    _, H, C = _rgat_dims(p, qi, num_relations, heads)
    return p.new_empty(rowptr.numel() - 1, H * C), p.new_empty(col.numel(), H)


@custom_op('pyg_amd::rgat_aggregate_backward', mutates_args=(), device_types=_DEV)
def rgat_aggregate_backward(grad: Tensor, p: Tensor, qi: Optional[Tensor], kj: Optional[Tensor],
                            b: Optional[Tensor], alpha: Tensor, out: Tensor, rowptr: Tensor,
                            col: Tensor, rel: Tensor, num_relations: int, heads: int,
                            negative_slope: float,
                            within: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The gradients of ``(p, qi, kj, b)``; an input not given gets an empty tensor."""
    R, H, C = _rgat_dims(p, qi, num_relations, heads)
    forms = _onepass.RgatForms.of_csr(rowptr, col, rel, p.size(0), R)
    grads = _onepass.rgat_backward(forms, p, qi, kj, b, alpha, out, grad, H, C, negative_slope,
                                   within=within, want_b=b is not None)
    return tuple(grad.new_empty(0) if t is None else t for t in grads)


@rgat_aggregate_backward.register_fake
def _(grad, p, qi, kj, b, alpha, out, rowptr, col, rel, num_relations, heads, negative_slope,
      within):
    def like(t):
        return (grad.new_empty(0) if t is None
                else torch.empty_like(t, memory_format=torch.contiguous_format))
    return like(p), like(qi), like(kj), like(b)


def _rgat_setup(ctx, inputs, output):
    p, qi, kj, b, rowptr, col, rel, num_relations, heads, negative_slope, within = inputs
    out, alpha = output
    ctx.static = (num_relations, heads, negative_slope, within)
    ctx.given = (qi is not None, b is not None)
    ctx.save_for_backward(p, qi, kj, b, alpha, out, rowptr, col, rel)


def _rgat_bwd(ctx, grad, _grad_alpha):
    p, qi, kj, b, alpha, out, rowptr, col, rel = ctx.saved_tensors
    g_p, g_qi, g_kj, g_b = rgat_aggregate_backward(grad.contiguous(), p, qi, kj, b, alpha, out,
                                                   rowptr, col, rel, *ctx.static)
    split, biased = ctx.given
    return (g_p, g_qi if split else None, g_kj if split else None, g_b if biased else None, None,
            None, None, None, None, None, None)


register_autograd('pyg_amd::rgat_aggregate', _rgat_bwd, setup_context=_rgat_setup)


# ---- mixture messages (GMMConv, NNConv) aggregate first, on a CSR pair (rows = destinations) -----
@custom_op('pyg_amd::mixture_conv', mutates_args=(), device_types=_DEV)
def mixture_conv(x_src: Tensor, coef: Tensor, weight: Tensor, rowptr: Tensor, col: Tensor,
                 edge_id: Optional[Tensor]) -> Tensor:
    """The propagate of GMMConv (gmm_conv.py:154-165) and NNConv (nn_conv.py:119-122): ``out
    [n_dst, M] = Z.reshape(n_dst, K * F) @ weight`` with ``Z[i, k] = sum_s coef[edge_id[s], k] *
    x_src[col[s]]`` over the slots of ``i``, ``coef [E, K]`` and ``weight [K, F, M]``.
    ``edge_id=None``: ``coef`` follows the slots of ``col``."""
    K, F, M = weight.shape
    if not _native.mixture_supported(F, K):
        raise NotImplementedError(
            f'mixture_conv serves 1 <= F <= 512 and 1 <= K <= 256 (got F = {F}, K = {K})')
    return _onepass.mixture_forward(_onepass._Form(rowptr, col), edge_id, x_src, coef, weight)


@mixture_conv.register_fake
def _(x_src, coef, weight, rowptr, col, edge_id):
    return x_src.new_empty(rowptr.numel() - 1, weight.shape[2])


@custom_op('pyg_amd::mixture_conv_backward', mutates_args=(), device_types=_DEV)
def mixture_conv_backward(grad: Tensor, x_src: Tensor, coef: Tensor, weight: Tensor,
                          rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], need_x: bool,
                          need_coef: bool, need_weight: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """The gradients of ``(x_src, coef, weight)``; one that is not needed is an empty tensor."""
    grads = _onepass.mixture_backward(Slots.of_csr(rowptr, col, x_src.size(0), edge_id), x_src,
                                      coef, weight, grad, want_x=need_x, want_coef=need_coef,
                                      want_weight=need_weight)
    return tuple(grad.new_empty(0) if g is None else (g.clone() if g._base is not None else g)
                 for g in grads)


@mixture_conv_backward.register_fake
def _(grad, x_src, coef, weight, rowptr, col, edge_id, need_x, need_coef, need_weight):
    e = grad.new_empty(0)
    return (torch.empty_like(x_src, memory_format=torch.contiguous_format) if need_x else e,
            torch.empty_like(coef, memory_format=torch.contiguous_format) if need_coef else e,
            torch.empty_like(weight, memory_format=torch.contiguous_format) if need_weight else e)


def _mixture_setup(ctx, inputs, output):
    x_src, coef, weight, rowptr, col, edge_id = inputs
    ctx.save_for_backward(x_src, coef, weight, rowptr, col, edge_id)


def _mixture_bwd(ctx, grad):
    x_src, coef, weight, rowptr, col, edge_id = ctx.saved_tensors
    need = ctx.needs_input_grad[:3]
    grads = mixture_conv_backward(grad.contiguous(), x_src, coef, weight, rowptr, col, edge_id,
                                  *need)
    return tuple(g if n else None for g, n in zip(grads, need)) + (None, None, None)


register_autograd('pyg_amd::mixture_conv', _mixture_bwd, setup_context=_mixture_setup)


# ---- HGTConv's typed relation transform (every edge type of a layer call in one launch) ----------
@custom_op('pyg_amd::hgt_relation', mutates_args=(), device_types=_DEV)
def hgt_relation(kqvs: List[Tensor], k_weight: Tensor, v_weight: Tensor, src_pos: List[int],
                 widx: List[int], heads: int) -> Tensor:
    """The packed ``kv [S, 2 * F]`` of hgt_conv.py:118-154: for edge type ``e`` of the call, whose
    source node type is ``kqvs[src_pos[e]] [N, 3 * F]`` (key | query | value), the rows ``k[:, h] @
    k_weight[h * T + widx[e]]`` and ``v[:, h] @ v_weight[h * T + widx[e]]``, stacked in call order.
    The weights are ``[heads * T, D, D]``."""
    D = k_weight.size(-1)
    if not _native.hgt_supported(heads, D):
        raise NotImplementedError(
            f'hgt_relation serves H * D <= 512, H <= 64 and D <= 128 (got {heads} x {D})')
    kqvs = [_native._f32_rows(x, 'kqv') for x in kqvs]
    ks, vs = _onepass.hgt_blocks(kqvs, src_pos, heads * D)
    return _native.hgt_relation_forward(ks, vs, widx, k_weight.contiguous(),
                                        v_weight.contiguous(), heads, D)


@hgt_relation.register_fake
def _(kqvs, k_weight, v_weight, src_pos, widx, heads):
    S = sum(kqvs[p].shape[0] for p in src_pos)
    return k_weight.new_empty(S, 2 * heads * k_weight.shape[-1])


@custom_op('pyg_amd::hgt_relation_backward', mutates_args=(), device_types=_DEV)
def hgt_relation_backward(grad: Tensor, kqvs: List[Tensor], k_weight: Tensor, v_weight: Tensor,
                          src_pos: List[int], widx: List[int],
                          heads: int) -> Tuple[List[Tensor], Tensor, Tensor]:
    return _onepass.hgt_backward([_native._f32_rows(x, 'kqv') for x in kqvs],
                                 k_weight.contiguous(), v_weight.contiguous(), src_pos, widx,
                                 heads, grad.contiguous())


@hgt_relation_backward.register_fake
def _(grad, kqvs, k_weight, v_weight, src_pos, widx, heads):
    return ([torch.empty_like(x, memory_format=torch.contiguous_format) for x in kqvs],
            torch.empty_like(k_weight), torch.empty_like(v_weight))


def _hgt_setup(ctx, inputs, output):
    kqvs, k_weight, v_weight, src_pos, widx, heads = inputs
    ctx.static = (list(src_pos), list(widx), heads)
    ctx.n = len(kqvs)
    ctx.save_for_backward(k_weight, v_weight, *kqvs)


def _hgt_bwd(ctx, grad):
    k_weight, v_weight, *kqvs = ctx.saved_tensors
    g_x, g_wk, g_wv = hgt_relation_backward(grad.contiguous(), list(kqvs), k_weight, v_weight,
                                            *ctx.static)
    return list(g_x), g_wk, g_wv, None, None, None


register_autograd('pyg_amd::hgt_relation', _hgt_bwd, setup_context=_hgt_setup)

# ---- per-graph normalisation over a by-graph pointer ---------------------------------------------------
def _norm_stats_shape(x: Tensor, ptr: Tensor, mode: str):
    B = ptr.numel() - 1
    return (B, x.size(1)) if mode == 'channel' else (B, )


@custom_op('pyg_amd::graph_norm', mutates_args=(), device_types=_DEV)
def graph_norm(x: Tensor, ptr: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
               mean_scale: Optional[Tensor], eps: float, mode: str,
               std_eps: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """GraphNorm (``mode='channel'``, graph_norm.py:72-76) or LayerNorm over whole graphs
    (``mode='graph'``, layer_norm.py:82-108; ``std_eps``: its formula without a batch vector) of
    ``x [N, F]`` for the graphs ``ptr [B + 1]`` of its rows.  Returns ``(y, mean, rstd)``; the
    per-graph statistics (``[B, F]`` / ``[B]``) are what the backward takes and are not
    differentiable.  The operator builds the hub plan of ``ptr`` itself, which reads two counts
    back: ONE host synchronisation per call, and one more in the backward operator.  The layers
    (``nn.norm.GraphNorm`` / ``LayerNorm``) do not pay it: they cache ``ptr`` and its plan per
    ``batch`` tensor (``_norm.batch_handle``)."""
    if not _native.graph_norm_supported(x.size(1)):
        raise NotImplementedError(f'graph_norm serves 1 <= F <= 512 (got F = {x.size(1)})')
    return _native.graph_norm_forward(ptr, x, weight, bias, mean_scale, eps, mode,
                                      std_eps=std_eps, hub=_native.graph_norm_plan(ptr))


@graph_norm.register_fake
def _(x, ptr, weight, bias, mean_scale, eps, mode, std_eps):
    stats = _norm_stats_shape(x, ptr, mode)
    return (torch.empty_like(x, memory_format=torch.contiguous_format), x.new_empty(stats),
            x.new_empty(stats))


@custom_op('pyg_amd::graph_norm_backward', mutates_args=(), device_types=_DEV)
def graph_norm_backward(grad: Tensor, x: Tensor, ptr: Tensor, weight: Optional[Tensor],
                        mean_scale: Optional[Tensor], mean: Tensor, rstd: Tensor, eps: float,
                        mode: str, std_eps: bool, affine_bias: bool
                        ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The gradients of ``(x, weight, bias, mean_scale)``; a parameter that was not given gets an
    empty tensor (``affine_bias``: the forward had a bias)."""
    grads = _native.graph_norm_backward(
        ptr, x, grad, mean, rstd, weight, mean_scale, eps, mode, std_eps=std_eps,
        hub=_native.graph_norm_plan(ptr), want_weight=weight is not None, want_bias=affine_bias,
        want_mean_scale=mean_scale is not None)
    return tuple(grad.new_empty(0) if g is None else g for g in grads)


@graph_norm_backward.register_fake
def _(grad, x, ptr, weight, mean_scale, mean, rstd, eps, mode, std_eps, affine_bias):
    F = x.size(1)
    return (torch.empty_like(x, memory_format=torch.contiguous_format),
            grad.new_empty(F if weight is not None else 0),
            grad.new_empty(F if affine_bias else 0),
            grad.new_empty(F if mean_scale is not None else 0))


def _graph_norm_setup(ctx, inputs, output):
    x, ptr, weight, bias, mean_scale, eps, mode, std_eps = inputs
    _, mean, rstd = output
    ctx.static = (eps, mode, std_eps, bias is not None)
    ctx.given = (weight is not None, bias is not None, mean_scale is not None)
    ctx.mark_non_differentiable(mean, rstd)
    ctx.save_for_backward(x, ptr, weight, mean_scale, mean, rstd)


def _graph_norm_bwd(ctx, grad, grad_mean, grad_rstd):
    x, ptr, weight, mean_scale, mean, rstd = ctx.saved_tensors
    g_x, g_w, g_b, g_ms = graph_norm_backward(grad.contiguous(), x, ptr, weight, mean_scale, mean,
                                              rstd, *ctx.static)
    g_w, g_b, g_ms = (g if given else None for g, given in zip((g_w, g_b, g_ms), ctx.given))
    return g_x, None, g_w, g_b, g_ms, None, None, None


register_autograd('pyg_amd::graph_norm', _graph_norm_bwd, setup_context=_graph_norm_setup)


# ---- one propagation step on a CSR pair (rows = destinations) --------------------------------------
@custom_op('pyg_amd::hop', mutates_args=(), device_types=_DEV)
def hop(rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor], w: Optional[Tensor], x: Tensor,
        a: float, y: Optional[Tensor], b: float, z: Optional[Tensor], c: float) -> Tensor:
    """``out [n_dst, F] = a * sum_k w[edge_id[k]] x[col[k]] (+ b * y) (+ c * z)`` (lg_conv.py:50,
    gcn2_conv.py:138-141, one iteration of appnp.py:129-131): one launch, the combination being
    the epilogue of the row sum.  ``w`` (None: 1) is in the caller's edge order (``edge_id=None``:
    in slot order) and takes no gradient; ``y`` / ``z`` have one row per destination."""
    n_dst = rowptr.numel() - 1
    for name, t in (('y', y), ('z', z)):
        if t is not None and tuple(t.shape) != (n_dst, x.size(1)):
            raise ValueError(f"'{name}' must be [{n_dst}, {x.size(1)}] (got {tuple(t.shape)})")
    return _native.hop(rowptr, col, edge_id, w, x, a, y=y, b=b, z=z, c=c,
                       hub=_native.hub_plan(rowptr))


@hop.register_fake
def _(rowptr, col, edge_id, w, x, a, y, b, z, c):
    return x.new_empty(rowptr.numel() - 1, x.shape[1])


@custom_op('pyg_amd::hop_backward', mutates_args=(), device_types=_DEV)
def hop_backward(grad: Tensor, rowptr: Tensor, col: Tensor, edge_id: Optional[Tensor],
                 w: Optional[Tensor], n_src: int, a: float, b: float, c: float, need_x: bool,
                 need_y: bool, need_z: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """The gradients of ``(x, y, z)``; one that is not needed is an empty tensor."""
    grads = _onepass.hop_backward(Slots.of_csr(rowptr, col, n_src, edge_id), w, grad, a, b, c,
                                  want_x=need_x, want_y=need_y, want_z=need_z)
    return tuple(grad.new_empty(0) if g is None else g for g in grads)


@hop_backward.register_fake
def _(grad, rowptr, col, edge_id, w, n_src, a, b, c, need_x, need_y, need_z):
    none = grad.new_empty(0)
    return (grad.new_empty(n_src, grad.shape[1]) if need_x else none,
            torch.empty_like(grad) if need_y else grad.new_empty(0),
            torch.empty_like(grad) if need_z else grad.new_empty(0))


def _hop_setup(ctx, inputs, output):
    rowptr, col, edge_id, w, x, a, y, b, z, c = inputs
    ctx.coef, ctx.n_src = (a, b, c), x.size(0)
    ctx.save_for_backward(rowptr, col, edge_id, w)


def _hop_bwd(ctx, grad):
    rowptr, col, edge_id, w = ctx.saved_tensors
    need = ctx.needs_input_grad
    g_x, g_y, g_z = hop_backward(grad.contiguous(), rowptr, col, edge_id, w, ctx.n_src, *ctx.coef,
                                 need[4], need[6], need[8])
    return (None, None, None, None, g_x if need[4] else None, None, g_y if need[6] else None,
            None, g_z if need[8] else None, None)


register_autograd('pyg_amd::hop', _hop_bwd, setup_context=_hop_setup)

OPS = ('index_sort', 'index2ptr', 'ptr2index', 'gather', 'scatter', 'scatter_backward',
       'segment_csr', 'segment_csr_backward', 'softmax_csr', 'softmax_csr_backward', 'spmm',
       'spmm_backward', 'linear', 'linear_backward', 'gatv2_attend', 'gatv2_attend_backward', 'transformer_attend',
       'transformer_attend_backward', 'transformer_edge_attend',
       'transformer_edge_attend_backward', 'hgt_relation', 'hgt_relation_backward',
       'gine_aggregate', 'gine_aggregate_backward', 'pna_aggregate', 'pna_aggregate_backward',
       'gen_aggregate', 'gen_aggregate_backward', 'resgated_aggregate',
       'resgated_aggregate_backward', 'han_attend', 'han_attend_backward', 'mixture_conv',
       'mixture_conv_backward', 'cg_aggregate', 'cg_aggregate_backward', 'film_aggregate',
       'film_aggregate_backward', 'rgat_aggregate', 'rgat_aggregate_backward', 'graph_norm',
       'graph_norm_backward', 'hop', 'hop_backward')
