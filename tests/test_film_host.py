"""nn.FiLMConv on host tensors: the restatement (tests/_film_ref.py) and the class against every
recorded reference case (tests/golden/golden_film_v1.pt), the state-dict keys, ``__repr__``, the
routing predicate, the ``ValueError`` for a missing ``edge_type``, the exported symbols, the
registered operators and the argument checks of the ``pygamd_film_*`` entry points.  No GPU
needed."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import _film_ref as R

SYMBOLS = ['pygamd_film_supported', 'pygamd_film_forward', 'pygamd_film_backward_dst',
           'pygamd_film_backward_src']


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


def test_recorded_margins_keep_every_relu_away_from_zero():
    G = R.load_golden()
    relu = [n for n in R.CASES if G['cases'][n]['act'] == 'relu']
    assert len(relu) == 8
    for case in [G['cases'][n] for n in relu] + [G['stack']]:
        assert case['margin'] >= 1e-4
    et = G['cases']['r3_empty_relation']['edge_type']
    assert int((et == 1).sum()) == 0 and int((et == 0).sum()) > 0 and int((et == 2).sum()) > 0
    et = G['cases']['r3_out_of_range']['edge_type']
    assert int((et >= 3).sum()) > 20 and G['cases']['r1_default']['edge_type'] is None
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_film_v1.pt')
    assert os.path.getsize(path) < 512 * 1024


def test_state_dicts_load_both_ways_with_the_reference_keys():
    from pytorch_geometric_amd.nn import FiLMConv
    from pytorch_geometric_amd.nn.conv import FiLMConv as FromConv
    assert FiLMConv is FromConv
    G = R.load_golden()
    for name in R.CASES:
        case = G['cases'][name]
        layer = R.make_layer(case)                      # reference -> this package (strict)
        back = layer.state_dict()                       # and what this package writes ...
        assert list(back) == list(case['state'])        # ... has the reference's keys, in order,
        for k, v in case['state'].items():              # shapes and dtypes
            assert back[k].shape == v.shape and back[k].dtype == v.dtype, (name, k)
            assert torch.equal(back[k], v)
    layer = FiLMConv((5, 7), 6, num_relations=2)
    assert list(layer.state_dict()) == [
        'lins.0.weight', 'lins.1.weight', 'films.0.weight', 'films.0.bias', 'films.1.weight',
        'films.1.bias', 'lin_skip.weight', 'film_skip.weight']       # (the skip's film: no bias)
    assert layer.lins[0].weight.shape == (6, 5) and layer.films[1].weight.shape == (12, 7)
    assert layer.lin_skip.weight.shape == (6, 7) and layer.film_skip.weight.shape == (12, 7)
    assert repr(layer) == 'FiLMConv((5, 7), 6, num_relations=2)'
    bare = FiLMConv(4, 3)
    assert bare.aggr == 'mean' and bare.num_relations == 1 and type(bare.act) is torch.nn.ReLU
    assert repr(bare) == 'FiLMConv(4, 3, num_relations=1)'
    assert FiLMConv(4, 3, num_relations=0).num_relations == 1
    # a caller's nn is deep-copied per relation and for the skip
    nn = torch.nn.Sequential(torch.nn.Linear(4, 5), torch.nn.Tanh(), torch.nn.Linear(5, 6))
    own = FiLMConv(4, 3, num_relations=2, nn=nn)
    nets = [own.films[0], own.films[1], own.film_skip]
    assert all(n is not nn for n in nets) and len({id(n[0].weight) for n in nets}) == 3
    assert 'film_skip.2.bias' in own.state_dict() and 'films.1.0.weight' in own.state_dict()
    before = own.films[0][0].weight.detach().clone()
    own.reset_parameters()
    assert not torch.equal(own.films[0][0].weight, before)


def test_routing_predicate_on_host_tensors():
    """host tensors never take the fused route, whatever ``fuse`` says; what else the predicate
    looks at is visible without a device"""
    from pytorch_geometric_amd.nn import FiLMConv
    layer = FiLMConv(8, 6, num_relations=2)
    layer.fuse = True
    x = torch.randn(10, 8)
    assert layer._fusable(x, x) is False
    ei, et = torch.randint(0, 10, (2, 30)), torch.randint(0, 2, (30, ))
    out = layer(x, ei, et)
    assert out.shape == (10, 6) and out.dtype == torch.float32
    out64 = layer.double()(x.double(), ei, et)
    assert out64.dtype == torch.float64
    assert float((out64 - out.double()).detach().abs().max()) < 1e-5
    # edges whose type is outside [0, R) contribute nothing
    et_bad = et.clone()
    et_bad[::3] = 5
    keep = et_bad < 2
    assert torch.equal(layer(x.double(), ei, et_bad), layer(x.double(), ei[:, keep], et_bad[keep]))


def test_missing_edge_type_is_a_value_error():
    from pytorch_geometric_amd.nn import FiLMConv
    x, ei = torch.randn(10, 8), torch.randint(0, 10, (2, 30))
    with pytest.raises(ValueError, match='edge_type'):
        FiLMConv(8, 6, num_relations=3)(x, ei)
    # one relation: edge_type is ignored and may be None
    layer = FiLMConv(8, 6)
    assert torch.equal(layer(x, ei), layer(x, ei, torch.full((30, ), 7)))


def test_fuse_switch_is_read_at_import():
    from pytorch_geometric_amd.nn import FiLMConv
    from pytorch_geometric_amd.nn.conv import film_conv as M
    value = os.environ.get('PYGAMD_FUSE_FILM', M._DEFAULT_FUSE_FILM)
    assert M.FUSE_FILM is (value.strip() not in ('', '0'))
    assert FiLMConv(4, 3).fuse is M.FUSE_FILM


def test_header_block_declares_exactly_the_four_symbols():
    from pytorch_geometric_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'pyg_amd.h')) as f:
        text = f.read()
    for sym in SYMBOLS:
        assert re.search(r'PYGAMD_API\s+int\s+' + sym + r'\s*\(', text), sym
        assert sym in _lib.SIGNATURES, sym
    bare = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert sorted(set(re.findall(r'\b(pygamd_film_\w+)\s*\(', bare))) == sorted(SYMBOLS)
    assert 'pygamd_film_workspace_bytes' not in text  # (resgated's query serves: the header says so)
    assert 'film_conv.py:128-161' in text              # the reference lines the block replaces
    assert 'film.hip' in _build.SOURCES and _lib.ABI_VERSION == 11
    assert re.search(r'#define\s+PYGAMD_ABI_VERSION\s+11\b', text)
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    _lib.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True,
                         text=True, check=True).stdout
    assert sorted(re.findall(r'\sT\s+(pygamd_film_\w+)$', out, re.M)) == sorted(SYMBOLS)


def test_operators_are_registered_with_fake_kernels():
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'film_aggregate' in ops.OPS and 'film_aggregate_backward' in ops.OPS
    schema = str(torch.ops.pyg_amd.film_aggregate.default._schema)
    assert schema == ('pyg_amd::film_aggregate(Tensor h, Tensor? g, Tensor? residual, Tensor rowptr, '
                      'Tensor col, Tensor? edge_id, Tensor rel, Tensor? scale, SymInt '
                      'num_relations, bool relu) -> Tensor')
    with FakeTensorMode():
        h, g, res = torch.empty(9, 24), torch.empty(7, 48), torch.empty(7, 8)
        ptr, col = torch.empty(8, dtype=torch.int64), torch.empty(30, dtype=torch.int64)
        rel, scale = torch.empty(30, dtype=torch.int32), torch.empty(30)
        O = torch.ops.pyg_amd
        out = O.film_aggregate(h, g, res, ptr, col, None, rel, scale, 3, True)
        assert out.shape == (7, 8)
        grads = O.film_aggregate_backward(out, h, g, ptr, col, None, rel, scale, 3, True)
        assert [tuple(t.shape) for t in grads] == [(9, 24), (7, 48)]
        # one node set in both roles: the packed [N, 3 R F] plane and ITS gradient
        plane = torch.empty(7, 72)
        out = O.film_aggregate(plane, None, None, ptr, col, None, rel, None, 3, False)
        assert out.shape == (7, 8)
        grads = O.film_aggregate_backward(out, plane, None, ptr, col, None, rel, None, 3, False)
        assert [tuple(t.shape) for t in grads] == [(7, 72), (0, )]


def test_envelope_and_argument_checks_without_a_device():
    """F <= 512.  Status 1 / 2 / 3 before any device work, 0 for a handle without rows; the
    workspace is ``pygamd_resgated_workspace_bytes(n_chunks, F, 0)``'s."""
    from _util import csr_arg
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    ok = lib.pygamd_film_supported
    assert ok(1) == 1 and ok(512) == 1 and ok(513) == 0 and ok(0) == 0 and ok(-3) == 0
    dev = ctypes.c_void_p(16)   # (never dereferenced: every call below is rejected or launches nothing)

    def fwd(g, F=8, R=2, rel=dev, ld_h=16, ld_gb=32, res=None, ld_r=0, act=1, ws=None, ws_bytes=0):
        return lib.pygamd_film_forward(g, None, rel, dev, ld_h, dev, ld_gb, None, res, ld_r, act,
                                       9, F, R, dev, ws, ws_bytes, None)

    def dst(g, F=8, R=2, prel=dev, ld_h=16, ld_gb=32, ld_g=8, ld_gg=32, act=1, mean=0, ws=None,
            ws_bytes=0):
        return lib.pygamd_film_backward_dst(g, prel, dev, dev, ld_h, dev, ld_gb, dev, ld_g, act,
                                            mean, 9, F, R, dev, ld_gg, ws, ws_bytes, None)

    def src(g, F=8, R=2, prel=dev, ld_h=16, ld_gb=32, ld_g=8, ld_gh=16, act=1, ws=None,
            ws_bytes=0):
        return lib.pygamd_film_backward_src(g, None, prel, dev, dev, ld_h, dev, ld_gb, None, dev,
                                            ld_g, act, 7, F, R, dev, ld_gh, ws, ws_bytes, None)

    assert fwd(None) == 1 and dst(None) == 1 and src(None) == 1
    empty = dict(rowptr=dev, col=dev, idx_dtype=1, n_rows=0, hub_threshold=1024, hub_chunk=256)
    e = lambda **kw: csr_arg(**dict(empty, **kw))                            # noqa: E731
    assert fwd(e()) == 0 and dst(e()) == 0 and src(e()) == 0                 # no rows: nothing to launch
    assert fwd(e(idx_dtype=5)) == 1 and src(e(n_hub=0, n_chunks=3)) == 1
    assert fwd(e(), F=513, ld_h=2048, ld_gb=4096) == 2 and dst(e(), F=600) == 2
    assert src(e(), F=513) == 2 and fwd(e(), F=0) == 1
    assert fwd(e(), R=0) == 1 and dst(e(), R=0) == 1 and src(e(), R=-1) == 1
    assert fwd(e(), ld_h=15) == 1 and fwd(e(), ld_gb=31) == 1                # strides below R F, 2 R F
    assert fwd(e(), res=dev, ld_r=7) == 1 and fwd(e(), act=2) == 1
    assert dst(e(), ld_g=7) == 1 and dst(e(), ld_gg=31) == 1 and dst(e(), mean=2) == 1
    assert dst(e(), act=-1) == 1 and dst(e(), ld_h=15) == 1
    assert src(e(), ld_g=7) == 1 and src(e(), ld_gh=15) == 1 and src(e(), act=3) == 1
    rows = lambda **kw: e(n_rows=4, **kw)                                    # noqa: E731
    assert fwd(rows(), rel=None) == 1                                        # the relation of an edge
    assert dst(rows(), prel=None) == 1 and src(rows(), prel=None) == 1       # the pair tables
    n = ctypes.c_size_t(0)
    hub = dict(n_rows=4, hub_rows=dev, hub_chunk_ptr=dev, n_hub=1, n_chunks=5)
    assert lib.pygamd_resgated_workspace_bytes(5, 8, 0, ctypes.byref(n)) == 0
    assert n.value == 5 * 16 * 4
    for call in (fwd, dst, src):
        assert call(e(**hub)) == 3 and call(e(**hub), ws=dev, ws_bytes=n.value - 1) == 3
