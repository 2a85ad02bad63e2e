"""Host side of the "rows given" mode (`save_agg = PYGAMD_AGG_GIVEN`) of the one-kernel SAGE layer
and of the first-layer aggregation cache built on it (nn/models/_fused_sage.py) — WITHOUT a device:
the C entry points are asked only for what their validation answers before any launch, and the
cache logic runs with `_native.sage_layer_forward` replaced by a recorder on CPU tensors."""
import ctypes
import gc

import pytest
import torch

from tests._util import gen, random_graph

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3


def _args(F=100, Fo=256, n_rows=64, save_agg=2):
    """Argument blocks of a given-mode launch whose pointers are valid, 16-byte aligned HOST
    memory (validation never dereferences them; nothing here reaches a kernel)."""
    from pytorch_geometric_amd import _lib
    host = torch.zeros(n_rows * max(2 * F, Fo) + 64, dtype=torch.float32)
    p = (host.data_ptr() + 15) // 16 * 16
    a = _lib.SpmmArgs()
    a.out, a.ldo = p, F
    a.n_rows, a.n_src, a.F = n_rows, n_rows, F
    a.idx_dtype, a.reduce = _lib.IDX_I64, _lib.MEAN
    a.w_heads, a.head_dim = 1, F
    f = _lib.SageFusedArgs()
    f.x_root, f.ld_root = p, F
    f.w, f.ldw = p, 2 * F
    f.Fo, f.relu, f.save_agg = Fo, 1, save_agg
    f.y, f.ldy = p, Fo
    return a, f, host


@pytest.fixture
def split_lib():
    """The library in split mode: a launch that passes validation then asks for its workspace and
    answers PYGAMD_ERR_WORKSPACE for a NULL one — before any device call."""
    from pytorch_geometric_amd import _lib, _native
    lib = _lib.load()
    prev = _native.set_gemm_mode('split')
    yield lib
    _native.set_gemm_mode(prev)


def _launch(lib, a, f):
    return lib.pygamd_sage_layer_fused(ctypes.byref(a), ctypes.byref(f), None, 0, None)


def test_header_and_mirror_agree_on_the_value():
    import os
    import re
    from pytorch_geometric_amd import _lib, _native
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               'include', 'pyg_amd.h')).read()
    m = re.search(r'#define\s+PYGAMD_AGG_GIVEN\s+(\d+)', header)
    assert m and int(m.group(1)) == _lib.AGG_GIVEN == _native.AGG_GIVEN == 2


def test_given_mode_needs_neither_graph_nor_gather_source(split_lib):
    a, f, _keep = _args()
    assert a.rowptr is None and a.col is None and a.x is None
    assert _launch(split_lib, a, f) == WORKSPACE      # validation passed
    f.save_agg = 1                                    # the gathering launch does need them
    assert _launch(split_lib, a, f) == INVALID


def test_given_mode_needs_the_stored_rows(split_lib):
    a, f, _keep = _args()
    a.out = None
    assert _launch(split_lib, a, f) == INVALID
    a, f, _keep = _args()
    a.ldo = a.F - 4
    assert _launch(split_lib, a, f) == INVALID
    a, f, _keep = _args()
    a.out = a.out + 4                                 # not 16-byte aligned
    assert _launch(split_lib, a, f) == UNSUPPORTED


def test_given_mode_refuses_compressed_source_rows(split_lib):
    from pytorch_geometric_amd import _lib
    a, f, keep = _args(F=128)
    a.x, a.ldx, a.x_format = keep.data_ptr(), 128 + 12, _lib.X_COMPRESSED
    assert _launch(split_lib, a, f) in (INVALID, UNSUPPORTED)
    a.x_format = _lib.X_DENSE                         # (the combination, not the other fields)
    assert _launch(split_lib, a, f) == WORKSPACE


def test_given_mode_through_the_plain_entry_point(split_lib):
    a, f, _keep = _args()
    rc = split_lib.pygamd_sage_layer_forward(ctypes.byref(a), f.x_root, f.ld_root, f.w, f.ldw, None,
                                             f.Fo, 1, 2, f.y, f.ldy, None, 0, None, 0, None)
    assert rc == WORKSPACE
    a.out = None
    rc = split_lib.pygamd_sage_layer_forward(ctypes.byref(a), f.x_root, f.ld_root, f.w, f.ldw, None,
                                             f.Fo, 1, 2, f.y, f.ldy, None, 0, None, 0, None)
    assert rc == INVALID


def test_workspace_query_drops_the_hub_partials(split_lib):
    a, f, keep = _args(save_agg=1)
    a.n_hub, a.n_chunks = 3, 17
    a.hub_rows = a.hub_chunk_ptr = keep.data_ptr()
    n1, n2 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert split_lib.pygamd_sage_layer_fused_workspace_bytes(ctypes.byref(a), ctypes.byref(f),
                                                            ctypes.byref(n1)) == OK
    f.save_agg = 2
    assert split_lib.pygamd_sage_layer_fused_workspace_bytes(ctypes.byref(a), ctypes.byref(f),
                                                            ctypes.byref(n2)) == OK
    hub = 17 * a.F * 4
    assert n1.value - n2.value == (hub + 255) // 256 * 256 and n2.value > 0


# ---- the cache ----------------------------------------------------------------------------------
class _Csr:
    def __init__(self, key, other, n):
        order = torch.sort(key, stable=True).indices
        self.ptr = torch._convert_indices_from_coo_to_csr(key[order], n)
        self.idx = other[order].contiguous()
        self.n_rows = self.n_cols = n
        self.hub = None

    def inv_degree(self):
        return 1.0 / (self.ptr[1:] - self.ptr[:-1]).clamp(min=1).to(torch.float32)


class _Graph:
    def __init__(self, ei, n):
        self._fwd, self._bwd = _Csr(ei[1], ei[0], n), _Csr(ei[0], ei[1], n)

    def by_dst(self):
        return self._fwd

    def by_src(self):
        return self._bwd


def _aggregate(ptr, idx, x, reduce):
    n = ptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n), ptr[1:] - ptr[:-1])
    out = torch.zeros(n, x.size(1)).index_add_(0, rows, x[idx])
    if reduce == 'mean':
        out = out / (ptr[1:] - ptr[:-1]).clamp(min=1).view(-1, 1)
    return out


@pytest.fixture
def recorder(monkeypatch):
    """`_native` replaced by plain torch on CPU tensors; every one-kernel launch is logged as
    (gather width, save_agg).  A given-mode launch gets NaN for its gather source: what it computes
    must come from the rows it was handed."""
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn.models import _fused_sage
    log = []

    def sage_layer_forward(ptr, idx, x_gather, x_root, w, bias, reduce, relu, agg, out, hub=None,
                           save_agg=True, relu_bits=None, mask_bits=None, row_scale=None,
                           out_scaled=None, gather_width=None, compressed_out=None):
        assert gather_width is None and compressed_out is None
        given = save_agg is not True and save_agg is not False and save_agg == _native.AGG_GIVEN
        a = agg.clone() if given else _aggregate(ptr, idx, x_gather, reduce)
        y = torch.cat([a, x_root], 1) @ w.t()
        if bias is not None:
            y = y + bias
        if relu:
            y = y.relu()
        if mask_bits is not None:
            raise AssertionError('no masked launch in these models')
        if save_agg and not given:
            agg.copy_(a)
        if relu_bits is not None:
            relu_bits.copy_(_native.pack_relu_bits(y))
        out.copy_(y)
        if out_scaled is not None:
            out_scaled.copy_(y * row_scale.view(-1, 1))
        log.append((x_gather.size(1), 'given' if given else bool(save_agg)))
        return out

    def spmm_csr(ptr, idx, x, reduce, *, n_rows=None, hub=None, out=None, accumulate=False,
                 src_bits=None, src_bits_set=None, relu_bits=None, relu_mask=None, src_scale=None):
        res = _aggregate(ptr, idx, x, reduce)
        if accumulate:
            res = res + out
        if relu_bits is not None:
            w = relu_bits.to(torch.int64) & 0xffffffff
            m = ((w.unsqueeze(-1) >> torch.arange(32)) & 1).permute(0, 2, 1, 3)
            res = torch.where(m.reshape(m.size(0) * 32, -1)[:res.size(0), :res.size(1)].bool(),
                              res, torch.zeros_like(res))
        if out is None:
            return res
        out.copy_(res)
        return out

    def rows_pack(g, row_scale=None, *, scaled=None, copy=None, count=True):
        live = (g != 0).any(dim=1)
        words = torch.zeros((g.size(0) + 31) // 32, dtype=torch.int64)
        for i in torch.nonzero(live).flatten().tolist():
            words[i >> 5] |= 1 << (i & 31)
        if scaled is not None:
            scaled.zero_()
            scaled[:, :g.size(1)] = g if row_scale is None else g * row_scale.view(-1, 1)
        if copy is not None:
            copy.zero_()
            copy[:, :g.size(1)] = g
        return words, (live.sum().view(1) if count else None)

    def linear_forward(x, w, bias=None, relu=False, out=None, accumulate=False):
        y = x @ w.t() + (0 if bias is None else bias)
        y = y.relu() if relu else y
        if out is None:
            return y
        out.copy_(y)
        return out

    def linear_dgrad(g, w_t, row_scale=None, n_scaled=0, out=None, accumulate=False,
                     relu_mask=None, relu_bits=None, out_scaled=None):
        y = g @ w_t.t()
        if row_scale is not None and n_scaled:
            y[:, :n_scaled] *= row_scale.view(-1, 1)
        if relu_bits is not None:
            w = relu_bits.to(torch.int64) & 0xffffffff
            m = ((w.unsqueeze(-1) >> torch.arange(32)) & 1).permute(0, 2, 1, 3)
            y = torch.where(m.reshape(m.size(0) * 32, -1)[:y.size(0), :y.size(1)].bool(), y,
                            torch.zeros_like(y))
        if out_scaled is not None:
            out_scaled.copy_(y * row_scale.view(-1, 1))
        return y

    def linear_wgrad(g, x, out=None, accumulate=False, wgs_per_cu=0, bias_grad=False, x2=None):
        gw = g.t() @ (x if x2 is None else torch.cat([x, x2], 1))
        return (gw, g.sum(0)) if bias_grad else gw

    for name, fn in dict(spmm_csr=spmm_csr, sage_layer_forward=sage_layer_forward,
                         rows_pack=rows_pack, linear_forward=linear_forward,
                         linear_dgrad=linear_dgrad, linear_wgrad=linear_wgrad).items():
        monkeypatch.setattr(_native, name, fn)
    monkeypatch.setattr(_native, 'sage_layer_forward_supported', lambda F, Fo, r: F % 4 == 0)
    # the one-launch input gradient stays out of the way: its launches are not what is counted
    monkeypatch.setattr(_fused_sage, 'FUSE_BWD', False)
    monkeypatch.setattr(_fused_sage, 'GEMM_BACKEND', 'own')
    monkeypatch.setattr(_fused_sage, 'FUSE_LAYER', True)
    monkeypatch.setattr(_fused_sage, 'OVERLAP_WGRAD', False)
    monkeypatch.delenv('PYGAMD_CACHE_AGG0', raising=False)
    return log


N, DIMS = 75, (20, 32, 32, 12)   # post (one kernel, roots on x), post, pre


def _model(seed=0):
    g = gen(seed)
    return [t.requires_grad_(True) for fi, fo in zip(DIMS[:-1], DIMS[1:])
            for t in (torch.randn(fo, fi, generator=g) * 0.2, torch.randn(fo, generator=g),
                      torch.randn(fo, fi, generator=g) * 0.2)]


def _step(x, graph, params, aggr='mean'):
    from pytorch_geometric_amd.nn.models._fused_sage import FusedSageStack
    for p in params:
        p.grad = None
    out = FusedSageStack.apply(x, graph, aggr, True, *params)
    out.square().sum().backward()
    return [out.detach().clone()] + [p.grad.clone() for p in params]


def _layer0(log):
    return [e[1] for e in log if e[0] == DIMS[0]]


def test_cache_hits_from_the_second_step_on_and_changes_nothing(recorder, monkeypatch):
    ei = random_graph(N, N, 600, seed=1, skew=True)
    x = torch.randn(N, DIMS[0], generator=gen(2))
    graph, params = _Graph(ei, N), _model()
    first = _step(x, graph, params)
    second = _step(x, graph, params)
    third = _step(x, graph, params)
    assert _layer0(recorder) == [True, 'given', 'given']
    monkeypatch.setenv('PYGAMD_CACHE_AGG0', '0')
    plain = _step(x, graph, params)
    assert _layer0(recorder)[-1] is True
    for got in (first, second, third):
        assert all(torch.equal(a, b) for a, b in zip(got, plain))
    # hidden layers (F = 32 here) never run in given mode and never touch the entry
    assert all(e[1] is True for e in recorder if e[0] != DIMS[0])
    assert graph.by_dst()._agg0[0]() is x


def test_cache_key(recorder, monkeypatch):
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn.models import _fused_sage
    ei = random_graph(N, N, 600, seed=3, skew=True)
    x = torch.randn(N, DIMS[0], generator=gen(4))
    graph, params = _Graph(ei, N), _model()

    def misses(fn, *a, **k):
        """runs one step; True when its layer-0 launch gathered"""
        del recorder[:]
        res = fn(*a, **k)
        (mode, ) = _layer0(recorder)
        return mode is True, res

    assert misses(_step, x, graph, params)[0]
    assert not misses(_step, x, graph, params)[0]
    # an in-place write bumps the version
    x.add_(1)
    miss, got = misses(_step, x, graph, params)
    assert miss and not misses(_step, x, graph, params)[0]
    want = _step(x.clone(), _Graph(ei, N), params)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # another tensor with the same contents
    x2 = x.clone()
    assert misses(_step, x2, graph, params)[0] and not misses(_step, x2, graph, params)[0]
    assert misses(_step, x, graph, params)[0]          # (one entry per handle)
    # another graph has its own entry; the first one is untouched
    other = _Graph(random_graph(N, N, 500, seed=9), N)
    assert misses(_step, x, other, params)[0]
    assert not misses(_step, x, graph, params)[0] and not misses(_step, x, other, params)[0]
    # the reduction is part of the key
    miss, got = misses(_step, x, graph, params, 'sum')
    want = _step(x.clone(), _Graph(ei, N), params, 'sum')
    assert miss and all(torch.equal(a, b) for a, b in zip(got, want))
    assert not misses(_step, x, graph, params, 'sum')[0]
    # ... and so are the hub plan's settings: those of the handle's plan (a handle without one
    # keys as None, so giving it one is a miss as well)
    fwd = graph.by_dst()
    fwd.hub = _native.no_hubs()
    assert misses(_step, x, graph, params, 'sum')[0]
    assert not misses(_step, x, graph, params, 'sum')[0]
    fwd.hub = fwd.hub._replace(threshold=fwd.hub.threshold + 1)
    assert misses(_step, x, graph, params, 'sum')[0]
    # ... and not the module's: with the handle's plan unchanged, another module value is a hit
    with monkeypatch.context() as m:
        m.setattr(_native, 'HUB_THRESHOLD', _native.HUB_THRESHOLD + 1)
        assert not misses(_step, x, graph, params, 'sum')[0]
    # an input that takes a gradient is never served from, nor stored in, the cache
    xg = x.clone().requires_grad_(True)
    assert misses(_step, xg, graph, params)[0] and misses(_step, xg, graph, params)[0]
    assert xg.grad is not None
    assert graph.by_dst()._agg0[0]() is x
    # nor is a tensor with a history (a hidden activation of a layer-by-layer model)
    def hidden_step():
        hidden = x * 2.0 + params[1][:1].sum() * 0
        assert hidden.grad_fn is not None
        return _step(hidden, graph, params)

    assert misses(hidden_step)[0] and misses(hidden_step)[0]
    assert graph.by_dst()._agg0[0]() is x
    # clear_aggregation_cache() drops every entry
    assert not misses(_step, x, other, params)[0]
    _fused_sage.clear_aggregation_cache()
    assert graph.by_dst()._agg0 is None and other.by_dst()._agg0 is None
    assert misses(_step, x, other, params)[0]


def test_entry_dies_with_the_input_and_no_grad_layers_do_not_populate(recorder):
    from pytorch_geometric_amd.nn.models._fused_sage import FusedSageStack
    ei = random_graph(N, N, 600, seed=5, skew=True)
    graph, params = _Graph(ei, N), _model()
    x = torch.randn(N, DIMS[0], generator=gen(6))
    _step(x, graph, params)
    assert graph.by_dst()._agg0 is not None
    del x
    gc.collect()
    assert graph.by_dst()._agg0 is None
    # a single layer under no_grad may be a hidden layer of a layer-by-layer model: it may hit,
    # it never stores
    x = torch.randn(N, DIMS[0], generator=gen(7))
    with torch.no_grad():
        h = FusedSageStack.apply(x, graph, 'mean', True, *params[:3])
        assert graph.by_dst()._agg0 is None
        FusedSageStack.apply(h, graph, 'mean', True, *params[3:6])
        assert graph.by_dst()._agg0 is None
    # a training step of the first layer stores; the no_grad pass then reads it back and the
    # hidden layer after it leaves the entry alone
    out = FusedSageStack.apply(x, graph, 'mean', True, *params[:3])
    out.sum().backward()
    assert graph.by_dst()._agg0[0]() is x
    del recorder[:]
    with torch.no_grad():
        h = FusedSageStack.apply(x, graph, 'mean', True, *params[:3])
        FusedSageStack.apply(h, graph, 'mean', True, *params[3:6])
    assert recorder == [(DIMS[0], 'given'), (DIMS[1], True)]
    assert graph.by_dst()._agg0[0]() is x
    # a whole model under no_grad does store: its input is the model's input
    x3 = torch.randn(N, DIMS[0], generator=gen(8))
    del recorder[:]
    with torch.no_grad():
        a = FusedSageStack.apply(x3, graph, 'mean', True, *params)
        b = FusedSageStack.apply(x3, graph, 'mean', True, *params)
    assert _layer0(recorder) == [True, 'given'] and torch.equal(a, b)
