"""One ``SAGEConv`` layer on float16 / bfloat16 storage as ONE forward kernel
(csrc/sage_fused_lp.hip, ``pygamd_sage_layer_lp``): after ``model.half()`` / ``model.bfloat16()`` the
aggregation, both linear maps and the bias of ``SAGEConv.forward`` (nn/conv/sage_conv.py:131-152)
run in one launch with one rounding of the aggregated row and one of the output, instead of the
16-bit SpMM, two ``torch`` linears and an add of the generic route (four launches, three roundings
per output).  The backward is composed from what exists: three ``torch`` products in the 16-bit type
and the 16-bit SpMM on the by-source handle.
"""
import os

import torch
from torch import Tensor
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ... import _native
from ...edge_index import EdgeIndex
from . import _fused_sage

# PYGAMD_FUSE_SAGE_LP=1 / 0 forces the route on / off for every layer built afterwards (the layer's
# `fuse_lp` attribute starts from it; `conv.fuse = False` opts out as well).  Unset: off — forward +
# backward the route measured 0.92-0.97 of the generic 16-bit route's speed in all twelve cells of
# profiles/sage_layer_lp.md (arxiv-sized and power-law graphs, F = Fo = 64 / 128 / 256, both
# dtypes), the eight with F >= 128 among them; the forward alone is faster at 64 columns and slower
# at 256.
_ENV = os.environ.get('PYGAMD_FUSE_SAGE_LP')
FUSE_LP_MEASURED = False
FUSE_LP = FUSE_LP_MEASURED if _ENV is None else _ENV != '0'


class SageLayerLpFunction(Function):
    r"""``out = narrow([aggr x | x] [W_l | W_r]^T + b)`` on a square handle, every tensor in one
    16-bit dtype.  Forward: ``pygamd_sage_layer_lp`` with the rounded aggregation saved.  Backward:
    ``grad_W_l = g^T agg``, ``grad_W_r = g^T x`` and ``grad_b = sum g`` by ``torch`` in the 16-bit
    type; ``grad_x = A^T (g W_l) + g W_r`` with the transposed aggregation on ``pygamd_spmm_lp``
    (``src_scale = 1 / deg`` for mean)."""

    @classmethod
    def apply(cls, x, graph, reduce, w_l, bias, w_r):
        # (forward() itself always runs with autograd off, and `needs_input_grad` follows
        # `requires_grad`, not the grad mode: whether the CALL records goes in as an argument)
        return super().apply(x, graph, reduce, w_l, bias, w_r, torch.is_grad_enabled())

    @staticmethod
    def forward(ctx, x: Tensor, graph: EdgeIndex, reduce: str, w_l: Tensor, bias, w_r: Tensor,
                recording: bool):
        fwd = graph.by_dst()
        ctx.graph, ctx.reduce = graph, reduce
        # `agg` is read by grad_W_l alone: an inference forward neither allocates nor writes it
        out, agg = _native.sage_layer_lp(fwd.ptr, fwd.idx, x, w_l, w_r, bias, reduce, hub=fwd.hub,
                                         save_agg=recording and ctx.needs_input_grad[3])
        ctx.save_for_backward(x, agg, w_l, w_r)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g: Tensor):
        x, agg, w_l, w_r = ctx.saved_tensors
        need = ctx.needs_input_grad
        grad_x = grad_wl = grad_b = grad_wr = None
        if need[0]:
            graph = ctx.graph
            bwd = graph.by_src()
            scale = graph.by_dst().inv_degree() if ctx.reduce == 'mean' else None
            grad_x = _native.spmm_csr_lp(bwd.ptr, bwd.idx, g @ w_l, 'sum', n_rows=bwd.n_rows,
                                         src_scale=scale, hub=bwd.hub) + g @ w_r
        if need[3]:
            grad_wl = g.t() @ agg
        if need[4]:
            grad_b = g.sum(0)
        if need[5]:
            grad_wr = g.t() @ x
        return grad_x, None, None, grad_wl, grad_b, grad_wr, None


def layer_eligible_lp(conv, x, edge_index, size) -> bool:
    """``conv(x, edge_index)`` is what :class:`SageLayerLpFunction` computes: every condition of
    ``_fused_sage.layer_eligible`` but the float32 ones, for a ``SAGEConv`` only, with ``x`` and
    the three parameters in one of float16 / bfloat16 on one device, inside the kernel's envelope
    and on a handle whose backward is not the atomic one."""
    if not getattr(conv, 'fuse_lp', FUSE_LP):
        return False
    if (not _fused_sage.LAYER_NODE or not _fused_sage.FUSE_LAYER
            or _fused_sage.GEMM_BACKEND != 'own'):
        return False
    if not (isinstance(x, Tensor) and x.is_cuda and x.dtype in _native.LP_DTYPES
            and x.dim() == 2):
        return False
    if x.size(0) == 0 or torch.is_autocast_enabled() or torch.compiler.is_compiling():
        return False
    if torch.jit.is_scripting() or torch.cuda.is_current_stream_capturing():
        return False
    if size is not None and tuple(size) != (x.size(0), x.size(0)):
        return False
    if not _fused_sage._conv_plain(conv, ('SAGEConv', )):
        return False
    params = (conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight)
    for p in params:
        if p is None:
            continue
        if isinstance(p, torch.nn.parameter.UninitializedParameter):
            return False
        if p.dtype != x.dtype or p.device != x.device:
            return False
    if conv.lin_l.weight.size(1) != x.size(1) or conv.lin_r.weight.size(1) != x.size(1):
        return False
    if not _native.sage_layer_lp_supported(x.dtype, x.size(1), conv.lin_l.weight.size(0),
                                           conv.aggr):
        return False
    if not _fused_sage._graph_ok(edge_index, x.size(0)):  # (no atomic-backward handle)
        return False
    return edge_index.size(1) > 0


def run_layer_lp(conv, x: Tensor, edge_index) -> Tensor:
    from ...edge_index import as_edge_index
    graph = as_edge_index(edge_index, x.size(0), x.size(0))
    aggr = 'sum' if conv.aggr == 'add' else conv.aggr
    return SageLayerLpFunction.apply(x, graph, aggr, conv.lin_l.weight, conv.lin_l.bias,
                                     conv.lin_r.weight)
