"""nn.CGConv on host tensors: the float32 restatement and the class against every recorded
reference case (tests/golden/golden_cg_v1.pt), the state-dict keys, the exported symbols, the
registered operators and the envelope and argument checks of the ``pygamd_cg_*`` entry points.
No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import _cg_ref as R

SYMBOLS = ['pygamd_cg_supported', 'pygamd_cg_forward', 'pygamd_cg_backward_dst',
           'pygamd_cg_backward_src']
NONE, WIDE, LINEAR = 0, 1, 2   # PYGAMD_GEN_EDGE_*


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
    from pytorch_geometric_amd.nn import CGConv
    from pytorch_geometric_amd.nn.conv import CGConv as FromConv
    assert CGConv is FromConv
    G = R.load_golden()
    for name in R.CASES:
        case = G['cases'][name]
        layer = R.make_layer(case)                      # reference -> this package (strict)
        back = layer.state_dict()                       # and what this package writes ...
        assert list(back) == list(case['state'])        # ... has the reference's keys, in order,
        for k, v in case['state'].items():              # shapes and dtypes
            assert back[k].shape == v.shape and back[k].dtype == v.dtype, (name, k)
            assert torch.equal(back[k], v)
    layer = CGConv((16, 12), dim=5, batch_norm=True)
    assert list(layer.state_dict()) == ['lin_f.weight', 'lin_f.bias', 'lin_s.weight', 'lin_s.bias',
                                        'bn.weight', 'bn.bias', 'bn.running_mean',
                                        'bn.running_var', 'bn.num_batches_tracked']
    # the columns are [x_i (dst, 12) | x_j (src, 16) | edge (5)]
    assert layer.lin_f.weight.shape == (12, 33) and layer.lin_s.weight.shape == (12, 33)
    assert repr(layer) == 'CGConv((16, 12), dim=5)'
    bare = CGConv(4, bias=False)
    assert bare.bn is None and bare.lin_f.bias is None and bare.lin_s.bias is None
    assert bare.aggr == 'add' and bare.dim == 0 and repr(bare) == 'CGConv(4, dim=0)'


def test_edge_attr_and_dim_come_together():
    from pytorch_geometric_amd.nn import CGConv
    x, ei = torch.randn(10, 8), torch.randint(0, 10, (2, 30))
    with pytest.raises(ValueError):
        CGConv(8)(x, ei, edge_attr=torch.randn(30, 3))
    with pytest.raises(ValueError):
        CGConv(8, dim=3)(x, ei)


def test_fuse_switch_is_read_at_import():
    """``PYGAMD_FUSE_CG``: 1 = every edge mode, 0 = none, or a comma list of modes; a layer's
    ``fuse`` says whether ITS mode is named."""
    from pytorch_geometric_amd.nn import CGConv
    from pytorch_geometric_amd.nn.conv import cg_conv as M
    assert M.FUSE_CG == M._parse_modes(os.environ.get('PYGAMD_FUSE_CG', M._DEFAULT_FUSE_CG))
    assert M._parse_modes('1') == ('none', 'linear', 'wide') and M._parse_modes('0') == ()
    assert M._parse_modes('') == () and M._parse_modes('wide, none') == ('none', 'wide')
    layers = {'none': CGConv(4), 'linear': CGConv(64, dim=32), 'wide': CGConv(64, dim=41)}
    for mode, layer in layers.items():
        assert layer.edge_mode == mode and layer.fuse is (mode in M.FUSE_CG)
    assert CGConv(65, dim=32).edge_mode == 'wide' and CGConv(512, dim=4).edge_mode == 'linear'


def test_symbols_are_exported_by_header_and_library():
    from pytorch_geometric_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'pyg_amd.h')) as f:
        text = f.read()
    for sym in SYMBOLS:
        assert re.search(r'PYGAMD_API\s+int\s+' + sym + r'\s*\(', text), sym
        assert sym in _lib.SIGNATURES, sym
    assert 'pygamd_cg_workspace_bytes' not in text    # (resgated's query serves: the header says so)
    assert 'cg_conv.py:81-98' in text                  # the reference lines the block replaces
    assert 'cg.hip' in _build.SOURCES and _lib.ABI_VERSION == 11
    assert re.search(r'#define\s+PYGAMD_ABI_VERSION\s+11\b', text)
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    _lib.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True,
                         text=True, check=True).stdout
    for sym in SYMBOLS:
        assert re.search(r'\sT\s+' + sym + r'$', out, re.M), sym
    assert sorted(re.findall(r'\sT\s+(pygamd_cg_\w+)$', out, re.M)) == sorted(SYMBOLS)


def test_operators_are_registered_with_fake_kernels():
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'cg_aggregate' in ops.OPS and 'cg_aggregate_backward' in ops.OPS
    schema = str(torch.ops.pyg_amd.cg_aggregate.default._schema)
    assert schema == ('pyg_amd::cg_aggregate(Tensor p, Tensor? q, Tensor? edge_attr, Tensor? w_f, '
                      'Tensor? w_s, Tensor? edge_terms, Tensor? residual, Tensor rowptr, '
                      'Tensor col, Tensor? edge_id, bool mean) -> Tensor')
    with FakeTensorMode():
        p, q, res = torch.empty(7, 16), torch.empty(9, 16), torch.empty(7, 8)
        ea, wf, ws = torch.empty(30, 3), torch.empty(8, 3), torch.empty(8, 3)
        ptr, col = torch.empty(8, dtype=torch.int64), torch.empty(30, dtype=torch.int64)
        O = torch.ops.pyg_amd
        out = O.cg_aggregate(p, q, ea, wf, ws, None, res, ptr, col, None, False)
        assert out.shape == (7, 8)
        grads = O.cg_aggregate_backward(out, p, q, ea, wf, ws, None, ptr, col, None, False)
        assert [tuple(g.shape) for g in grads] == [(7, 16), (9, 16), (30, 3), (8, 3), (8, 3), (0, )]
        # one node set in both roles: the packed [N, 4F] plane and ITS gradient; dense edge terms
        pq, terms = torch.empty(7, 32), torch.empty(30, 16)
        out = O.cg_aggregate(pq, None, None, None, None, terms, None, ptr, col, None, True)
        assert out.shape == (7, 8)
        grads = O.cg_aggregate_backward(out, pq, None, None, None, None, terms, ptr, col, None,
                                        True)
        assert [tuple(g.shape) for g in grads] == [(7, 32), (0, ), (0, ), (0, ), (0, ), (30, 16)]


def test_envelope_and_argument_checks_without_a_device():
    """F <= 512; raw edge features: De <= 32 and F * De <= 2048 (what the layer's ``edge_mode``
    assumes).  Status 1 / 2 / 3 before any device work, 0 for a handle without rows; the workspace
    is ``pygamd_resgated_workspace_bytes``'s."""
    from _util import csr_arg
    from pytorch_geometric_amd import _build, _lib, _native
    from pytorch_geometric_amd.nn.conv.cg_conv import _native_envelope
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    ok = lib.pygamd_cg_supported
    assert ok(1, 0) == 1 and ok(512, 0) == 1 and ok(513, 0) == 0 and ok(0, 0) == 0
    assert ok(64, 32) == 1 and ok(64, 33) == 0 and ok(65, 32) == 0 and ok(16, 41) == 0
    assert ok(512, 4) == 1 and ok(512, 5) == 0 and ok(256, 8) == 1 and ok(257, 8) == 0
    assert ok(128, 16) == 1 and ok(129, 16) == 0 and ok(8, -1) == 0
    assert _native.cg_supported(100, 20) and not _native.cg_supported(100, 21)
    for F in (1, 16, 63, 64, 65, 128, 129, 256, 257, 400, 512, 513):
        for De in (1, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 41):
            assert _native_envelope(F, De) == bool(ok(F, De)), (F, De)
            # never past resgated's, whose workspace formula the entry points assume
            assert ok(F, De) <= lib.pygamd_resgated_supported(F, De), (F, De)
    dev = ctypes.c_void_p(16)   # (never dereferenced: every call below is rejected or launches nothing)

    def fwd(g, F=8, De=0, mode=NONE, ea=None, w=None, ld_p=16, ld_q=16, res=None, ld_r=0, scale=0,
            ws=None, ws_bytes=0):
        return lib.pygamd_cg_forward(g, None, dev, ld_p, dev, ld_q, mode, ea, w, res, ld_r, scale,
                                     9, F, De, dev, ws, ws_bytes, None)

    def dst(g, F=8, De=0, mode=NONE, ea=None, w=None, ld_g=8, ld_gp=16, scale=0, ge=None, gw=None,
            ws=None, ws_bytes=0):
        return lib.pygamd_cg_backward_dst(g, None, dev, 16, dev, 16, mode, ea, w, dev, ld_g, scale,
                                          9, F, De, dev, ld_gp, ge, gw, ws, ws_bytes, None)

    def src(g, F=8, De=0, mode=NONE, ea=None, w=None, ld_g=8, ld_gq=16, scale=0, ptr=None,
            ws=None, ws_bytes=0):
        return lib.pygamd_cg_backward_src(g, None, dev, 16, dev, 16, mode, ea, w, dev, ld_g, scale,
                                          ptr, 7, F, De, dev, ld_gq, ws, ws_bytes, None)

    assert fwd(None) == 1 and dst(None) == 1 and src(None) == 1
    empty = dict(rowptr=dev, col=dev, idx_dtype=1, n_rows=0, hub_threshold=1024, hub_chunk=256)
    e = lambda **kw: csr_arg(**dict(empty, **kw))                            # noqa: E731
    assert fwd(e()) == 0 and dst(e()) == 0 and src(e()) == 0                 # no rows: nothing to launch
    assert fwd(e(idx_dtype=5)) == 1 and src(e(n_hub=0, n_chunks=3)) == 1
    assert fwd(e(), F=513) == 2 and dst(e(), F=64, De=33) == 2 and src(e(), F=512, De=5) == 2
    assert fwd(e(), ld_p=15) == 1 and fwd(e(), ld_q=15) == 1                 # strides below the widths
    assert fwd(e(), res=dev, ld_r=7) == 1 and fwd(e(), scale=2) == 1
    assert dst(e(), ld_g=7) == 1 and dst(e(), ld_gp=15) == 1
    assert src(e(), ld_g=7) == 1 and src(e(), ld_gq=15) == 1 and src(e(), scale=-1) == 1
    rows = lambda **kw: e(n_rows=4, **kw)                                    # noqa: E731
    lin = dict(De=3, mode=LINEAR)
    assert fwd(rows(), ea=dev, **lin) == 1 and fwd(rows(), w=dev, **lin) == 1  # they come together
    assert fwd(rows(), mode=NONE, ea=dev) == 1 and fwd(rows(), mode=WIDE) == 1
    assert fwd(rows(), mode=WIDE, ea=dev, w=dev) == 1 and fwd(rows(), mode=7) == 1
    assert fwd(rows(), mode=WIDE, ea=dev, De=3) == 1                         # De counts for LINEAR only
    assert dst(rows(), ea=dev, w=dev, **lin) == 1                            # no grad_weight
    assert dst(rows(), mode=NONE, ge=dev) == 1                               # nothing to differentiate
    assert dst(rows(), mode=WIDE, ea=dev, gw=dev) == 1
    assert src(rows(), scale=1) == 1 and src(rows(), scale=0, ptr=dev) == 1  # mean <=> dst_rowptr
    n = ctypes.c_size_t(0)
    size = lib.pygamd_resgated_workspace_bytes
    assert size(0, 8, 3, ctypes.byref(n)) == 0 and n.value == 512 * 2 * 24 * 4
    assert dst(rows(), ea=dev, w=dev, gw=dev, **lin) == 3                    # partials need room
    assert dst(rows(), ea=dev, w=dev, gw=dev, ws=dev, ws_bytes=n.value - 1, **lin) == 3
    hub = dict(n_rows=4, hub_rows=dev, hub_chunk_ptr=dev, n_hub=1, n_chunks=5)
    assert size(5, 8, 0, ctypes.byref(n)) == 0 and n.value == 5 * 16 * 4
    for call in (fwd, dst, src):
        assert call(e(**hub)) == 3 and call(e(**hub), ws=dev, ws_bytes=n.value - 1) == 3
