"""nn.ResGatedGraphConv on host tensors: the float32 restatement and the class against every
recorded reference case (tests/golden/golden_resgated_v1.pt), the state-dict keys, the exported
symbols, the registered operators and the envelope and argument checks of the
``pygamd_resgated_*`` entry points.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import _resgated_ref as R

SYMBOLS = ['pygamd_resgated_supported', 'pygamd_resgated_workspace_bytes',
           'pygamd_resgated_forward', 'pygamd_resgated_backward_dst',
           'pygamd_resgated_backward_src']


@pytest.mark.parametrize('name', R.CASES)
def test_restatement_reproduces_the_golden_cases(name):
    R.check_restatement_case(R.load_golden(), name)


@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_host_tensors(name):
    G = R.load_golden()
    layer = R.check_class_case(G, name, 'cpu')
    assert repr(layer) == G['cases'][name]['repr']


def test_golden_stack_on_host_tensors():
    R.check_stack(R.load_golden(), 'cpu')


def test_state_dicts_load_both_ways_with_the_reference_keys():
    from pytorch_geometric_amd.nn import ResGatedGraphConv
    from pytorch_geometric_amd.nn.conv import ResGatedGraphConv as FromConv
    assert ResGatedGraphConv is FromConv
    G = R.load_golden()
    for name in R.CASES:
        case = G['cases'][name]
        layer = R.make_layer(case)                      # reference -> this package (strict)
        back = layer.state_dict()                       # and what this package writes ...
        assert list(back) == list(case['state'])        # ... has the reference's keys, in order,
        for k, v in case['state'].items():              # shapes and dtypes
            assert back[k].shape == v.shape and back[k].dtype == v.dtype, (name, k)
            assert torch.equal(back[k], v)
    layer = ResGatedGraphConv((16, 12), 8, edge_dim=5)
    assert list(layer.state_dict()) == ['bias', 'lin_key.weight', 'lin_key.bias',
                                        'lin_query.weight', 'lin_query.bias', 'lin_value.weight',
                                        'lin_value.bias', 'lin_skip.weight']
    assert layer.lin_key.weight.shape == (8, 17) and layer.lin_query.weight.shape == (8, 21)
    assert layer.lin_value.weight.shape == (8, 21) and layer.lin_skip.weight.shape == (8, 12)
    assert float(layer.bias.detach().abs().max()) == 0.0
    bare = ResGatedGraphConv(4, 4, root_weight=False, bias=False)
    assert bare.lin_skip is None and bare.bias is None
    assert isinstance(bare.act, torch.nn.Sigmoid) and bare.aggr == 'add'


def test_edge_attr_and_edge_dim_come_together():
    from pytorch_geometric_amd.nn import ResGatedGraphConv
    x, ei = torch.randn(10, 8), torch.randint(0, 10, (2, 30))
    with pytest.raises(AssertionError):
        ResGatedGraphConv(8, 8)(x, ei, edge_attr=torch.randn(30, 3))
    with pytest.raises(AssertionError):
        ResGatedGraphConv(8, 8, edge_dim=3)(x, ei)


def test_fuse_switch_is_read_at_import():
    from pytorch_geometric_amd.nn import ResGatedGraphConv
    from pytorch_geometric_amd.nn.conv import res_gated_graph_conv as M
    want = os.environ.get('PYGAMD_FUSE_RESGATED', '1') not in ('', '0')
    assert M.FUSE_RESGATED is want and ResGatedGraphConv(4, 4).fuse is want


def test_symbols_are_exported_by_header_and_library():
    from pytorch_geometric_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'pyg_amd.h')) as f:
        text = f.read()
    for sym in SYMBOLS:
        assert re.search(r'PYGAMD_API\s+int\s+' + sym + r'\s*\(', text), sym
        assert sym in _lib.SIGNATURES, sym
    assert 'resgated.hip' in _build.SOURCES
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    _lib.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True,
                         text=True, check=True).stdout
    for sym in SYMBOLS:
        assert re.search(r'\sT\s+' + sym + r'$', out, re.M), sym


def test_operators_are_registered_with_fake_kernels():
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'resgated_aggregate' in ops.OPS and 'resgated_aggregate_backward' in ops.OPS
    schema = str(torch.ops.pyg_amd.resgated_aggregate.default._schema)
    assert schema.startswith('pyg_amd::resgated_aggregate(Tensor k, Tensor qv, Tensor? edge_attr, '
                             'Tensor? w_gate, Tensor? w_value, Tensor rowptr, Tensor col, '
                             'Tensor? edge_id')
    assert schema.endswith('-> Tensor')
    with FakeTensorMode():
        k, qv = torch.empty(7, 8), torch.empty(9, 16)
        ea, wg, wv = torch.empty(30, 3), torch.empty(8, 3), torch.empty(8, 3)
        ptr, col = torch.empty(8, dtype=torch.int64), torch.empty(30, dtype=torch.int64)
        out = torch.ops.pyg_amd.resgated_aggregate(k, qv, ea, wg, wv, ptr, col, None)
        assert out.shape == (7, 8)
        grads = torch.ops.pyg_amd.resgated_aggregate_backward(out, k, qv, ea, wg, wv, ptr, col,
                                                              None)
        assert [tuple(g.shape) for g in grads] == [(7, 8), (9, 16), (30, 3), (8, 3), (8, 3)]
        grads = torch.ops.pyg_amd.resgated_aggregate_backward(out, k, qv, None, None, None, ptr,
                                                              col, None)
        assert [tuple(g.shape) for g in grads] == [(7, 8), (9, 16), (0, ), (0, ), (0, )]


def test_envelope_and_argument_checks_without_a_device():
    """F <= 512; with De > 0, De <= 32 and F * De <= 2048.  Status 1 / 2 / 3 before any device
    work, 0 for a handle without rows."""
    from _util import csr_arg
    from pytorch_geometric_amd import _build, _lib, _native
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    ok = lib.pygamd_resgated_supported
    assert ok(1, 0) == 1 and ok(512, 0) == 1 and ok(513, 0) == 0 and ok(0, 0) == 0
    assert ok(64, 32) == 1 and ok(64, 33) == 0 and ok(65, 32) == 0
    assert ok(512, 4) == 1 and ok(512, 5) == 0 and ok(256, 8) == 1 and ok(257, 8) == 0
    assert ok(128, 16) == 1 and ok(129, 16) == 0 and ok(8, -1) == 0
    assert _native.resgated_supported(100, 20) and not _native.resgated_supported(100, 21)
    dev = ctypes.c_void_p(16)   # (never dereferenced: every call below is rejected or launches nothing)

    def fwd(g, F=8, De=0, ea=None, w=None, ld_k=8, ld_qv=16, ws=None, ws_bytes=0):
        return lib.pygamd_resgated_forward(g, None, dev, ld_k, dev, ld_qv, ea, w, 9, F, De, dev,
                                           ws, ws_bytes, None)

    def dst(g, F=8, De=0, ea=None, w=None, ld_g=8, ge=None, gw=None, ws=None, ws_bytes=0):
        return lib.pygamd_resgated_backward_dst(g, None, dev, 8, dev, 16, ea, w, dev, ld_g, 9, F,
                                                De, dev, ge, gw, ws, ws_bytes, None)

    def src(g, F=8, De=0, ea=None, w=None, ld_g=8, ws=None, ws_bytes=0):
        return lib.pygamd_resgated_backward_src(g, None, dev, 8, dev, 16, ea, w, dev, ld_g, 7, F,
                                                De, dev, ws, ws_bytes, None)

    assert fwd(None) == 1 and dst(None) == 1 and src(None) == 1
    empty = dict(rowptr=dev, col=dev, idx_dtype=1, n_rows=0, hub_threshold=1024, hub_chunk=256)
    e = lambda **kw: csr_arg(**dict(empty, **kw))                            # noqa: E731
    assert fwd(e()) == 0 and dst(e()) == 0 and src(e()) == 0                 # no rows: nothing to launch
    assert fwd(e(idx_dtype=5)) == 1 and src(e(n_hub=0, n_chunks=3)) == 1
    assert fwd(e(), F=513) == 2 and dst(e(), F=64, De=33) == 2 and src(e(), F=512, De=5) == 2
    assert fwd(e(), ld_k=7) == 1 and fwd(e(), ld_qv=15) == 1                 # strides below the widths
    assert dst(e(), ld_g=7) == 1 and src(e(), ld_g=7) == 1
    rows = lambda **kw: e(n_rows=4, **kw)                                    # noqa: E731
    assert fwd(rows(), De=3, ea=dev) == 1 and fwd(rows(), De=3, w=dev) == 1  # they come together
    assert fwd(rows(), De=0, ea=dev) == 1
    assert dst(rows(), De=3, ea=dev, w=dev) == 1                             # no grad_weight
    assert dst(rows(), De=0, ge=dev) == 1                                    # nothing to differentiate
    assert dst(rows(), De=3, ea=dev, w=dev, gw=dev) == 3                     # partials need room
    hub = dict(n_rows=4, hub_rows=dev, hub_chunk_ptr=dev, n_hub=1, n_chunks=5)
    assert fwd(e(**hub)) == 3 and fwd(e(**hub), ws=dev, ws_bytes=5 * 8 * 4 - 1) == 3
    assert src(e(**hub), ws=dev, ws_bytes=5 * 16 * 4 - 1) == 3
    n = ctypes.c_size_t(0)
    size = lib.pygamd_resgated_workspace_bytes
    assert size(5, 8, 0, ctypes.byref(n)) == 0 and n.value == 5 * 16 * 4
    assert size(0, 8, 3, ctypes.byref(n)) == 0 and n.value == 512 * 2 * 24 * 4
    assert size(0, 8, 0, None) == 1 and size(0, 1024, 0, ctypes.byref(n)) == 2
    assert size(0, 512, 5, ctypes.byref(n)) == 2
