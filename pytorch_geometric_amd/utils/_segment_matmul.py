import torch
from typing import Optional

from torch import Tensor
from torch.autograd import Function

from .. import _native

_LOW = (torch.float16, torch.bfloat16)


def _product(x: Tensor, w: Tensor, plan, **kw) -> Tensor:
    """The grouped product on the kernels of the operands' storage: csrc/segmm_lp.hip for float16 /
    bfloat16 (one dtype for both, result in it), csrc/segmm.hip for float32."""
    if x.dtype in _LOW:
        return _native.segment_matmul_lp(x, w, plan, **kw)
    return _native.segment_matmul(x, w, plan, **kw)


def _wgrad(x: Tensor, g: Tensor, plan, n_seg: int, blocks: int, **kw) -> Tensor:
    if x.dtype in _LOW:
        return _native.segment_matmul_wgrad_lp(x, g, plan, n_seg, blocks, **kw)
    return _native.segment_matmul_wgrad(x, g, plan, n_seg, blocks, **kw)


def _route(inputs: Tensor, other: Tensor):
    """``(inputs, other, narrow_to)`` as the autograd nodes below take them.  float32 operands pass
    as they are.  A float16 / bfloat16 device ``inputs`` with ``other`` in the same dtype or in
    float32 (torch.autocast keeps parameters float32: ``other`` is narrowed by a differentiable
    cast, so its gradient comes back float32) runs in that storage — or, with PYGAMD_SEGMM_LP=0,
    widened around the float32 kernels and narrowed to ``narrow_to``.  Anything else is refused."""
    if inputs.dtype == torch.float32 and other.dtype == torch.float32:
        return inputs, other, None
    if (inputs.is_cuda and other.is_cuda and inputs.dtype in _LOW
            and other.dtype in (inputs.dtype, torch.float32)):
        from .. import _functions
        if _functions.SEGMM_LP is False:
            return inputs.float(), other.float(), inputs.dtype
        return inputs, other.to(inputs.dtype), None
    raise NotImplementedError("segment_matmul computes in float32, and in float16 / bfloat16 on "
                              "device tensors")


class _SegmentMatmul(Function):
    """``rows`` (16-bit operands only; a permutation of the rows): operand row ``s`` is
    ``inputs[rows[s]]`` and its product lands in ``out[rows[s]]`` — the type-sorted order of
    ``HeteroLinear`` applied inside the launches, forward and backward."""

    @staticmethod
    def forward(ctx, inputs: Tensor, ptr_host: tuple, other: Tensor, blocks: int = 1,
                rows: Optional[Tensor] = None):
        plan = _native.segmm_plan(ptr_host, inputs.device, blocks)
        ctx.plan, ctx.n_seg, ctx.blocks, ctx.rows = plan, other.size(0), blocks, rows
        ctx.save_for_backward(inputs, other)
        if rows is not None:
            return _native.segment_matmul_lp(inputs, other, plan, blocks=blocks, x_rows=rows,
                                             out_rows=rows)
        return _product(inputs, other, plan, blocks=blocks)

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        inputs, other = ctx.saved_tensors
        grad_in = grad_other = None
        perm = {} if ctx.rows is None else {'x_rows': ctx.rows}
        if ctx.needs_input_grad[0]:
            scatter = {} if ctx.rows is None else {'out_rows': ctx.rows}
            grad_in = _product(grad_out, other, ctx.plan, transpose_w=True, blocks=ctx.blocks,
                               **perm, **scatter)
        if ctx.needs_input_grad[2]:
            gather = {} if ctx.rows is None else {'g_rows': ctx.rows}
            grad_other = _wgrad(inputs, grad_out, ctx.plan, ctx.n_seg, ctx.blocks, **perm,
                                **gather)
        return grad_in, None, grad_other, None, None


class _SegmentMatmulSum(Function):
    """``segment_matmul`` followed by the per-destination sum of its rows (the tail of RGCNConv,
    rgcn_conv.py:284-290 + aggregate): ``out[i] = sum_{s : dst[s] = i} (inputs[s] @ other[seg(s)])``
    as ONE autograd node.  Forward = the grouped GEMM + one SpMM over ``out_graph`` (rows of the
    product -> destinations).  The backward of that sum gives every row ``s`` the gradient row of
    its destination: instead of gathering them into a ``[S, F]`` copy (one launch, 0.8 GB written
    and read twice at the FB15k-237 shape), the input- and weight-gradient launches read
    ``grad_out[dst[s]]`` themselves (``x_rows`` / ``g_rows`` of the C ABI)."""

    @staticmethod
    def forward(ctx, inputs: Tensor, ptr_host: tuple, other: Tensor, blocks: int, out_graph):
        plan = _native.segmm_plan(ptr_host, inputs.device, blocks)
        t = _product(inputs, other, plan, blocks=blocks)
        by_dst = out_graph.by_dst()
        spmm = _native.spmm_csr_lp if t.dtype in _LOW else _native.spmm_csr
        out = spmm(by_dst.ptr, by_dst.idx, t, 'sum', n_rows=by_dst.n_rows, hub=by_dst.hub)
        ctx.plan, ctx.n_seg, ctx.blocks = plan, other.size(0), blocks
        ctx.dst = out_graph.edge_index[1]
        ctx.save_for_backward(inputs, other)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        inputs, other = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        grad_in = grad_other = None
        if ctx.needs_input_grad[0]:
            grad_in = _product(grad_out, other, ctx.plan, transpose_w=True, blocks=ctx.blocks,
                               x_rows=ctx.dst)
        if ctx.needs_input_grad[2]:
            grad_other = _wgrad(inputs, grad_out, ctx.plan, ctx.n_seg, ctx.blocks,
                                g_rows=ctx.dst)
        return grad_in, None, grad_other, None, None


def segment_matmul_sum(inputs: Tensor, ptr_host: tuple, other: Tensor, out_graph) -> Tensor:
    r"""``out[i] = sum_{s: dst[s] = i} inputs[s] @ other[seg(s)]`` with ``out_graph`` the handle
    rows-of-the-product -> destinations (one entry per row ``s``); ``other`` is ``[R, K, N]`` or
    the block-diagonal ``[R, B, K, N]`` of :func:`block_segment_matmul`.  float32, or float16 /
    bfloat16 device operands (:func:`_route`; the sum then runs on ``spmm_csr_lp``)."""
    inputs, other, narrow_to = _route(inputs, other)
    if other.dim() == 4:
        R, B, K, N = other.shape
        if inputs.size(1) != B * K or len(ptr_host) != R + 1:
            raise ValueError("'inputs' must be [S, B*K] and 'ptr' must hold R + 1 entries")
        out = _SegmentMatmulSum.apply(inputs, tuple(ptr_host), other.reshape(R * B, K, N), B,
                                      out_graph)
    else:
        if len(ptr_host) != other.size(0) + 1 or inputs.size(1) != other.size(1):
            raise ValueError("'ptr' must hold R + 1 entries and 'inputs' must be [S, K]")
        out = _SegmentMatmulSum.apply(inputs, tuple(ptr_host), other, 1, out_graph)
    return out if narrow_to is None else out.to(narrow_to)


def block_segment_matmul(inputs: Tensor, ptr_host: tuple, other: Tensor) -> Tensor:
    r"""Block-diagonal variant used by ``RGCNConv(num_blocks=B)`` (rgcn_conv.py:222-244):
    ``other`` is ``[R, B, K, N]``; rows of segment ``r`` are multiplied block by block,
    ``out[s, b*N:(b+1)*N] = inputs[s, b*K:(b+1)*K] @ other[r, b]`` — one launch, no transposes."""
    if inputs.dtype in _LOW:
        inputs, other, narrow_to = _route(inputs, other)
    else:
        narrow_to = None
    R, B, K, N = other.shape
    if inputs.size(1) != B * K or len(ptr_host) != R + 1:
        raise ValueError("'inputs' must be [S, B*K] and 'ptr' must hold R + 1 entries")
    out = _SegmentMatmul.apply(inputs, tuple(ptr_host), other.reshape(R * B, K, N), B)
    return out if narrow_to is None else out.to(narrow_to)


def segment_matmul(inputs: Tensor, ptr, other: Tensor) -> Tensor:
    r"""``out[ptr[g]:ptr[g+1]] = inputs[ptr[g]:ptr[g+1]] @ other[g]`` — the contract of
    ``pyg_lib.ops.segment_matmul`` (call sites: torch_geometric/nn/conv/rgcn_conv.py:288,
    nn/dense/linear.py:255).  ``ptr`` may be a tensor (one host copy) or a Python sequence.

    ONE launch of the grouped GEMM for the forward, one for each gradient (the weight gradient of
    16-bit operands: two); the (segment, row tile) table is built once per pointer and cached.
    float32 operands run on the fp32 matrix cores (csrc/segmm.hip); float16 / bfloat16 device
    operands on the 16-bit matrix instruction in their own storage (csrc/segmm_lp.hip), result and
    gradients in that dtype — a float32 ``other`` next to 16-bit ``inputs`` (torch.autocast) is
    narrowed first and gets a float32 gradient."""
    inputs, other, narrow_to = _route(inputs, other)
    if inputs.dim() != 2 or other.dim() != 3:
        raise ValueError("'inputs' must be [S, K] and 'other' [G, K, N]")
    if isinstance(ptr, Tensor):
        ptr_host = tuple(int(v) for v in ptr.tolist())
    else:
        ptr_host = tuple(int(v) for v in ptr)
    if len(ptr_host) != other.size(0) + 1:
        raise ValueError(f"'ptr' has {len(ptr_host)} entries but 'other' holds "
                         f"{other.size(0)} matrices")
    if ptr_host[-1] != inputs.size(0) or ptr_host[0] != 0:
        raise ValueError("'ptr' must start at 0 and end at the number of input rows")
    out = _SegmentMatmul.apply(inputs, ptr_host, other)
    return out if narrow_to is None else out.to(narrow_to)
