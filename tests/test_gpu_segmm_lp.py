"""The float16 / bfloat16 grouped GEMM (csrc/segmm_lp.hip) against float64 products of the same
16-bit values.  Kernel bound, elementwise: eps_T / 2 * |ref| (the one rounding) + 2 * L * 2^-24 *
(|a| @ |b|) (float32 accumulation over a reduction of length L).  Layer bound: 4 * eps_T * M, M
the layer's formula on absolute values (at most 8 roundings of eps_T / 2 of the running size)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_geometric_amd import _lib, _native, nn, utils  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
DEV = 'cuda'


def _close(out, ref, mag, L, dtype):
    bound = EPS[dtype] / 2 * ref.abs() + 2 * L * 2.0 ** -24 * mag
    err = (out.double() - ref).abs()
    assert bool((err <= bound).all()), float((err - bound).max())


def _segments(x, w, ptr, blocks=1):
    """float64 ``x[seg] @ w[g]`` per segment and column block -> (ref, |x| @ |w|)."""
    K, N = w.shape[1:]
    x, w = x.detach().double(), w.detach().double()
    ref = x.new_zeros(x.size(0), blocks * N)
    mag = torch.zeros_like(ref)
    for g in range(len(ptr) - 1):
        for b in range(blocks):
            a = x[ptr[g]:ptr[g + 1], b * K:(b + 1) * K]
            ref[ptr[g]:ptr[g + 1], b * N:(b + 1) * N] = a @ w[g * blocks + b]
            mag[ptr[g]:ptr[g + 1], b * N:(b + 1) * N] = a.abs() @ w[g * blocks + b].abs()
    return ref, mag


def _ptr():
    t = _lib.load().pygamd_segment_matmul_tile_rows()
    ptr = [0]
    for n in (0, 1, t - 1, t, t + 1):
        ptr.append(ptr[-1] + n)
    return tuple(ptr)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', ['plain', 'perm', 'slice'])
@pytest.mark.parametrize('blocks', [1, 2])
@pytest.mark.parametrize('transpose_w', [False, True])
@pytest.mark.parametrize('K,N', [(8, 8), (24, 40), (100, 100), (136, 72)])
def test_product(K, N, transpose_w, blocks, layout, dtype):
    torch.manual_seed(K + N)
    ptr = _ptr()
    S, G = ptr[-1], (len(ptr) - 1) * blocks
    x = torch.randn(S, blocks * K + 3, device=DEV).to(dtype)
    x = x[:, 1:1 + blocks * K] if layout == 'slice' else x[:, :blocks * K].contiguous()
    w = torch.randn(G, K, N, device=DEV).to(dtype)
    rows = torch.randperm(S, device=DEV) if layout == 'perm' else None
    plan = _native.segmm_plan(ptr, x.device, blocks)
    w_arg = w.transpose(1, 2).contiguous() if transpose_w else w
    out = _native.segment_matmul_lp(x, w_arg, plan, transpose_w=transpose_w, blocks=blocks,
                                    x_rows=rows, out_rows=rows)
    assert out.dtype == dtype and tuple(out.shape) == (S, blocks * N)
    ref, mag = _segments(x if rows is None else x[rows], w, ptr, blocks)
    _close(out if rows is None else out[rows], ref, mag, K, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', ['plain', 'gathered', 'slice'])
def test_weight_gradient(layout, dtype):
    """'slice': ``x`` starts at an odd element of a wider tensor — the 2-byte access path."""
    torch.manual_seed(3)
    gathered = layout == 'gathered'
    K, N = 24, 40
    ptr = (0, _native.WGRAD_CHUNK_ROWS + 1, _native.WGRAD_CHUNK_ROWS + 1,
           _native.WGRAD_CHUNK_ROWS + 4)
    S = ptr[-1]
    x = torch.randn(S, K + 3, device=DEV).to(dtype)
    x = x[:, 1:1 + K] if layout == 'slice' else x[:, :K].contiguous()
    g = torch.randn(257 if gathered else S, N, device=DEV).to(dtype)
    g_rows = torch.randint(0, 257, (S, ), device=DEV) if gathered else None
    plan = _native.segmm_plan(ptr, x.device)
    gw = _native.segment_matmul_wgrad_lp(x, g, plan, 3, g_rows=g_rows)
    again = _native.segment_matmul_wgrad_lp(x, g, plan, 3, g_rows=g_rows)
    assert gw.dtype == dtype and torch.equal(gw.view(torch.int16), again.view(torch.int16))
    gd = (g if g_rows is None else g[g_rows]).double()
    for s in range(3):
        a, b = x[ptr[s]:ptr[s + 1]].double().t(), gd[ptr[s]:ptr[s + 1]]
        _close(gw[s], a @ b, a.abs() @ b.abs(), ptr[s + 1] - ptr[s], dtype)


@pytest.mark.parametrize('w_dtype', [None, torch.float32])
@pytest.mark.parametrize('dtype', DTYPES)
def test_public_route(dtype, w_dtype):
    """``w_dtype`` float32: the autocast case (16-bit rows, float32 parameters)."""
    torch.manual_seed(5)
    ptr, K, N = (0, 5, 5, 140), 100, 100
    x = torch.randn(ptr[-1], K, device=DEV).to(dtype).requires_grad_()
    w = torch.randn(3, K, N, device=DEV).to(dtype).to(w_dtype or dtype).requires_grad_()
    out = utils.segment_matmul(x, torch.tensor(ptr), w)
    g = torch.randn_like(out)
    gx, gw = torch.autograd.grad(out, (x, w), g)
    assert (out.dtype, gx.dtype, gw.dtype) == (dtype, dtype, w_dtype or dtype)
    _close(out, *_segments(x, w, ptr), K, dtype)
    _close(gx, *_segments(g, w.transpose(1, 2), ptr), N, dtype)
    for s in range(3):
        a, b = x.detach()[ptr[s]:ptr[s + 1]].double().t(), g[ptr[s]:ptr[s + 1]].double()
        _close(gw[s], a @ b, a.abs() @ b.abs(), ptr[s + 1] - ptr[s], dtype)


_CHILD = """
import sys, torch
sys.path.insert(0, {tests!r})
import test_gpu_segmm_lp as t
from pytorch_geometric_amd import _functions, utils
assert _functions.SEGMM_LP is False
ptr = (0, 5, 5, 140)
x = torch.randn(140, 100, device='cuda').bfloat16()
w = torch.randn(3, 100, 100, device='cuda').bfloat16()
out = utils.segment_matmul(x, ptr, w)
assert out.dtype == torch.bfloat16
t._close(out, *t._segments(x, w, ptr), 100, torch.bfloat16)
"""


def test_widening_switch():
    env = dict(os.environ, PYGAMD_SEGMM_LP='0')
    code = _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert res.returncode == 0, res.stderr[-2000:]


# ---- layers: 40 nodes, 5 relations, relation 3 without edges ------------------------------------
def _graph():
    torch.manual_seed(11)
    ei = torch.randint(0, 40, (2, 300), device=DEV)
    et = torch.randint(0, 4, (300, ), device=DEV)
    et[et == 3] = 4
    return ei, et


def _rgcn_formula(conv, p, x, ei, et):
    """RGCNConv on float64 tensors ``p`` (the layer's parameters by name) with dense adjacencies."""
    R, n = conv.num_relations, x.size(0)
    w = p['weight']
    if conv.num_bases is not None:
        w = (p['comp'] @ w.reshape(conv.num_bases, -1)).reshape(R, x.size(1), -1)
    elif conv.num_blocks is not None:
        w = torch.stack([torch.block_diag(*w[r]) for r in range(R)])
    out = x @ p['root'] + p['bias']
    for r in range(R):
        adj = torch.zeros(n, n, dtype=torch.float64, device=x.device)
        sel = et == r
        adj.index_put_((ei[1, sel], ei[0, sel]), torch.ones((), dtype=torch.float64,
                                                            device=x.device), accumulate=True)
        if conv.aggr == 'mean':
            adj = adj / adj.sum(1, keepdim=True).clamp(min=1)
        out = out + adj @ x @ w[r]
    return out


def _check_layer(mod, formula, x, args, dtype):
    """Output and parameter gradients of ``mod`` (parameters and ``x`` in ``dtype``) against
    ``formula`` in float64, within 4 eps_T of the formula on absolute values."""
    names = [n for n, _ in mod.named_parameters()]
    params = [q for _, q in mod.named_parameters()]
    out = mod(x, *args)
    assert out.dtype == dtype
    g = torch.randn_like(out)
    grads = torch.autograd.grad(out, params, g)

    def evaluate(f):
        p64 = {n: f(q.detach().double()).requires_grad_() for n, q in zip(names, params)}
        o = formula(mod, p64, f(x.double()), *args)
        return [o] + list(torch.autograd.grad(o, list(p64.values()), f(g.double())))

    for got, ref, mag in zip([out] + list(grads), evaluate(lambda t: t), evaluate(torch.abs)):
        assert got.dtype == dtype
        err = (got.double() - ref).abs()
        assert bool((err <= 4 * EPS[dtype] * mag).all()), float((err - 4 * EPS[dtype] * mag).max())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kw', [{}, {'num_bases': 2}, {'num_blocks': 2}, {'aggr': 'add'}],
                         ids=['plain', 'bases', 'blocks', 'add'])
def test_rgcn(kw, dtype):
    ei, et = _graph()
    torch.manual_seed(13)
    conv = nn.RGCNConv(12, 20, 5, **kw).to(DEV)
    torch.nn.init.normal_(conv.bias, std=0.5)
    conv = conv.to(dtype)
    x = torch.randn(40, 12, device=DEV).to(dtype)
    _check_layer(conv, _rgcn_formula, x, (ei, et), dtype)


def _hetero_formula(mod, p, x, type_vec):
    return torch.einsum('sk,skn->sn', x, p['weight'][type_vec]) + p['bias'][type_vec]


@pytest.mark.parametrize('dtype', DTYPES)
def test_hetero_linear(dtype):
    torch.manual_seed(17)
    lin = nn.HeteroLinear(12, 20, 4).to(DEV).to(dtype)
    x = torch.randn(150, 12, device=DEV).to(dtype)
    type_vec = torch.randint(0, 3, (150, ), device=DEV)
    type_vec[type_vec == 1] = 3   # type 1 unused, rows unsorted
    _check_layer(lin, _hetero_formula, x, (type_vec, ), dtype)
    with pytest.raises(ValueError, match='one type per row'):   # (no launch on a short 'x')
        lin(x[:100], type_vec)
    with torch.no_grad(), torch.profiler.profile(
            activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        lin(x, type_vec)
        torch.cuda.synchronize()
    kernels = [e.name for e in prof.events()
               if e.device_type == torch.autograd.DeviceType.CUDA]
    assert sum('segmm_lp' in k for k in kernels) == 1, kernels
    assert not any('gather' in k for k in kernels), kernels
