"""APPNP, SGConv, SSGConv, TAGConv, LGConv and GCN2Conv without a GPU: the restatement of
tests/_hops_ref.py against the reference's recorded results (tests/golden/golden_hops_v1.pt), the
classes on host tensors (the generic route), their state dicts, the exported symbols, the argument
checks of ``pygamd_hop``, the switch, the routing and the conditioning of the recurrence on the
degree-profile graph."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _degree_cases as D  # noqa: E402
import _hops_ref as R  # noqa: E402

G = R.load_golden()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['pygamd_hop', 'pygamd_hop_workspace_size']
LAYERS = ('APPNP', 'SGConv', 'SSGConv', 'TAGConv', 'LGConv', 'GCN2Conv')


def test_case_list_is_the_golden_file():
    assert sorted(R.CASES) == sorted(G['cases'])
    assert {c['cls'] for c in G['cases'].values()} == set(LAYERS)
    assert os.path.getsize(R.GOLDEN) < os.path.getsize(
        os.path.join(os.path.dirname(R.GOLDEN), 'golden_cg_v1.pt'))
    assert G['stack']['margin'] >= G['meta']['margin']


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_restatement_reproduces_the_golden_cases(name):
    R.check_restatement_case(G, name)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_golden_cases_on_host_tensors(name):
    routes = []
    R.check_class_case(G, name, 'cpu', routes=routes)
    assert set(routes) == {'generic'}


def test_golden_stack_on_host_tensors():
    R.check_stack(G, 'cpu')


def test_state_dicts_load_both_ways_with_the_reference_keys():
    want = {'appnp': [], 'lg': [], 'sg_k3': ['lin.bias', 'lin.weight'], 'sg_no_bias': ['lin.weight'],
            'ssg_k3': ['lin.bias', 'lin.weight'],
            'tag_k3': ['bias', 'lins.0.weight', 'lins.1.weight', 'lins.2.weight', 'lins.3.weight'],
            'tag_no_bias': ['lins.0.weight', 'lins.1.weight', 'lins.2.weight'],
            'gcn2_shared': ['weight1'], 'gcn2_separate': ['weight1', 'weight2']}
    for name, keys in want.items():
        case = G['cases'][name]
        assert sorted(case['state']) == keys, name
        layer = R.make_layer(case)                       # the reference's state, strict
        back = {k: torch.empty_like(v) for k, v in case['state'].items()}
        for k, v in layer.state_dict().items():          # and ours in the reference's shapes
            assert v.shape == back[k].shape and v.dtype == back[k].dtype, (name, k)
            back[k].copy_(v)
            assert torch.equal(back[k], case['state'][k])
        with pytest.raises(RuntimeError):
            layer.load_state_dict(dict(case['state'], extra=torch.zeros(1)), strict=True)


def test_constructor_errors_and_initialisers():
    from pytorch_geometric_amd import nn
    with pytest.raises(AssertionError):
        nn.GCN2Conv(8, 0.1, theta=0.5)                   # theta and layer come together
    with pytest.raises(ValueError):
        nn.APPNP(2, 0.1, flow='sideways')
    torch.manual_seed(0)
    conv = nn.GCN2Conv(64, 0.1, shared_weights=False)
    bound = (6.0 / 128) ** 0.5                           # glorot
    for w in (conv.weight1, conv.weight2):
        top = float(w.detach().abs().max())
        assert 0.8 * bound < top <= bound
    tag = nn.TAGConv(16, 4, K=2)
    assert len(tag.lins) == 3 and not bool(tag.bias.any())
    assert all(lin.bias is None for lin in tag.lins)
    assert nn.SGConv(16, 4).lin.bias is not None and nn.SSGConv(16, 4, 0.1, bias=False).lin.bias is None
    assert repr(nn.LGConv()) == 'LGConv()'


def test_symbols_are_exported_by_header_and_library():
    from pytorch_geometric_amd import _build, _lib, nn
    from pytorch_geometric_amd.nn import conv
    for name in LAYERS:
        assert getattr(nn, name) is getattr(conv, name)
        assert name in nn.__all__ and name in conv.__all__
    assert 'hop.hip' in _build.SOURCES and _lib.ABI_VERSION == 11
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES
    with open(os.path.join(ROOT, 'include', 'pyg_amd.h')) as f:
        text = f.read()
    for sym in SYMBOLS:
        assert re.search(r'PYGAMD_API\s+int\s+' + sym + r'\s*\(', text), sym
    assert re.search(r'#define\s+PYGAMD_ABI_VERSION\s+11\b', text)
    for site in ('appnp.py:111-133', 'sg_conv.py:93-95', 'ssg_conv.py:102-106', 'tag_conv.py:87-91',
                 'lg_conv.py:50', 'gcn2_conv.py:138-153'):
        assert site in text, site
    m = re.search(r'typedef struct pygamd_hop_args \{(.*?)\} pygamd_hop_args;', text, flags=re.S)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    fields = [re.split(r'[\s\*]+', d.strip())[-1].split('[')[0] for d in body.split(';') if d.strip()]
    assert fields == [n for n, _ in _lib.HopArgs._fields_]
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    _lib.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True,
                         text=True, check=True).stdout
    assert sorted(re.findall(r'\sT\s+(pygamd_hop\w*)$', out, re.M)) == sorted(SYMBOLS)


def test_operator_is_registered_with_fake_kernels():
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'hop' in ops.OPS and 'hop_backward' in ops.OPS
    schema = str(torch.ops.pyg_amd.hop.default._schema)
    assert schema == ('pyg_amd::hop(Tensor rowptr, Tensor col, Tensor? edge_id, Tensor? w, Tensor x, '
                      'float a, Tensor? y, float b, Tensor? z, float c) -> Tensor')
    with FakeTensorMode():
        ptr, col = torch.empty(8, dtype=torch.int64), torch.empty(30, dtype=torch.int64)
        x, y, w = torch.empty(9, 5), torch.empty(7, 5), torch.empty(30)
        O = torch.ops.pyg_amd
        out = O.hop(ptr, col, None, w, x, 0.9, y, 0.1, None, 0.0)
        assert out.shape == (7, 5)
        grads = O.hop_backward(out, ptr, col, None, w, 9, 0.9, 0.1, 0.0, True, True, False)
        assert [tuple(g.shape) for g in grads] == [(9, 5), (7, 5), (0, )]


def test_argument_checks_without_a_device():
    """Every check of ``pygamd_hop`` returns its status before any launch: 1 for a bad argument, 3
    for a hub plan whose workspace is short, 0 for a handle without rows."""
    from _util import csr_arg
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    dev, dev2, dev3 = ctypes.c_void_p(16), ctypes.c_void_p(4096), ctypes.c_void_p(8192)

    def p(v):
        return v.value if isinstance(v, ctypes.c_void_p) else v

    def hop(g, ws=None, ws_bytes=0, **kw):
        a = dict(x=dev, ldx=8, n_src=9, F=8, a=1.0, out=dev2, ldo=8)
        a.update(kw)
        reserved = a.pop('reserved', None)
        args = _lib.HopArgs(**{k: p(v) for k, v in a.items()})
        if reserved is not None:
            args.reserved[reserved] = 1
        return lib.pygamd_hop(g, None, ctypes.byref(args), ws, ws_bytes, None)

    empty = dict(rowptr=dev, col=dev, idx_dtype=1, n_rows=0, hub_threshold=1024, hub_chunk=256)
    e = lambda **kw: csr_arg(**dict(empty, **kw))                            # noqa: E731
    assert lib.pygamd_hop(None, None, ctypes.byref(_lib.HopArgs()), None, 0, None) == 1
    assert lib.pygamd_hop(e(), None, None, None, 0, None) == 1
    assert hop(e()) == 0                                                     # no rows: no launch
    assert hop(e(idx_dtype=5)) == 1 and hop(e(reserved0=1)) == 1 and hop(e(n_rows=-1)) == 1
    assert hop(e(), x=None) == 1                                             # null x
    assert hop(e(), out=None) == 1                                           # neither out nor sum
    assert hop(e(), out=None, sum=dev3, lds=8) == 0                          # sum alone is a call
    assert hop(e(), F=0) == 1 and hop(e(), F=-3) == 1 and hop(e(), n_src=-1) == 1
    assert hop(e(), ldx=7) == 1 and hop(e(), ldo=7) == 1                     # pitches below F
    assert hop(e(), y=dev3, ldy=7) == 1 and hop(e(), z=dev3, ldz=7) == 1
    assert hop(e(), sum=dev3, lds=7) == 1
    assert hop(e(), y=dev3, ldy=8, z=dev3, ldz=12, sum=dev3, lds=8) == 0
    assert hop(e(), out=dev) == 1                                            # out is x
    assert hop(e(), sum=dev, lds=8) == 1                                     # sum is x
    assert hop(e(), sum=dev2, lds=8) == 1                                    # out is sum
    assert hop(e(), y=dev2, ldy=8) == 0 and hop(e(), z=dev2, ldz=8) == 0     # out may be y or z
    assert hop(e(), sum_init=2) == 1
    for i in range(4):
        assert hop(e(), reserved=i) == 1
    hub = dict(n_rows=4, hub_rows=dev, hub_chunk_ptr=dev, n_hub=1, n_chunks=5)
    n = ctypes.c_size_t(0)
    size = lib.pygamd_hop_workspace_size
    assert size(5, 8, ctypes.byref(n)) == 0 and n.value == 5 * 8 * 4
    assert size(0, 8, ctypes.byref(n)) == 0 and n.value == 0
    assert size(5, 0, ctypes.byref(n)) == 1 and size(-1, 8, ctypes.byref(n)) == 1
    assert size(5, 8, None) == 1
    for chunks, F in ((2 ** 31 + 1, 3), (2 ** 20, 2 ** 13), (2 ** 40, 2 ** 20)):   # past 32 bits
        assert size(chunks, F, ctypes.byref(n)) == 0 and n.value == chunks * F * 4
    assert hop(e(**hub)) == 3 and hop(e(**hub), ws=dev3, ws_bytes=5 * 8 * 4 - 1) == 3
    assert hop(e(**dict(hub, hub_rows=None)), ws=dev3, ws_bytes=160) == 1


def test_fuse_switch_is_read_at_import():
    code = ('from pytorch_geometric_amd.nn import APPNP, SGConv, SSGConv, TAGConv, LGConv, GCN2Conv\n'
            'ls = [APPNP(2, 0.1), SGConv(4, 4), SSGConv(4, 4, 0.1), TAGConv(4, 4), LGConv(), '
            'GCN2Conv(4, 0.1)]\n'
            'print([l.fuse for l in ls])')
    # unset: every layer's measured default (LGConv, a single step without a combination, lost
    # to propagate at both shapes measured: profiles/propagate_hops.md)
    measured = [True, True, True, True, False, True]
    for value, want in (('0', [False] * 6), ('1', [True] * 6), (None, measured)):
        env = {k: v for k, v in os.environ.items() if k != 'PYGAMD_FUSE_HOPS'}
        env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
        if value is not None:
            env['PYGAMD_FUSE_HOPS'] = value
        out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True,
                             check=True).stdout
        assert out.strip() == str(want), (value, out)


class _FakeDevice(torch.Tensor):
    """A host tensor that says it lives on the device: what ``hop_route`` reads is the metadata"""
    is_cuda = True


def _on_device(t):
    return t.as_subclass(_FakeDevice)


def test_routing_reports_the_generic_route():
    from pytorch_geometric_amd.nn import APPNP, SGConv
    x = _on_device(torch.randn(6, 4))
    ei = _on_device(torch.randint(0, 6, (2, 12)))
    w = _on_device(torch.rand(12))
    layer = APPNP(2, 0.1)
    layer.fuse = True
    assert layer.hop_route(x, ei) == 'fused' and layer.hop_route(x, ei, w) == 'fused'
    assert layer.hop_route(x, ei, _on_device(torch.rand(12).requires_grad_(True))) == 'generic'
    assert layer.hop_route(torch.randn(6, 4), ei) == 'generic'                # host features
    assert layer.hop_route(_on_device(torch.randn(6, 4).half()), ei) == 'generic'
    assert layer.hop_route(_on_device(torch.randn(6, 4).double()), ei) == 'generic'
    layer.fuse = False
    assert layer.hop_route(x, ei) == 'generic'
    for aggr in ('max', 'mean', 'min'):
        other = APPNP(2, 0.1, aggr=aggr)
        other.fuse = True
        assert other.hop_route(x, ei) == 'generic', aggr
    hooked = SGConv(4, 4)
    hooked.fuse = True
    assert hooked.hop_route(x, ei) == 'fused'
    handle = hooked.register_message_forward_hook(lambda mod, inputs, out: None)
    assert hooked.hop_route(x, ei) == 'generic'
    handle.remove()
    assert hooked.hop_route(x, ei) == 'fused'

    class Doubled(APPNP):
        def message(self, x_j, edge_weight):
            return 2 * x_j

    own = Doubled(2, 0.1)
    own.fuse = True
    assert own.hop_route(x, ei) == 'generic'


# ---- conditioning: the inputs are not why a device test passes or fails ------------------------------
def _profile_problem(setting, F, seed):
    ei, n, _ = D.build(0, *setting)
    g = torch.Generator().manual_seed(seed)
    ei64, w64 = R.gcn_norm(ei, None, n, True, torch.float64)
    return ei64, w64, n, torch.randn(n, F, generator=g), torch.randn(n, F, generator=g)


@pytest.mark.parametrize('setting', [(64, 48), (9, 5), (256, 256)])
def test_float32_restatement_is_well_conditioned_on_the_profile_graph(setting):
    """The float32 restatement of the recurrence in a shuffled edge order stays within 1e-5 of the
    float64 one (relative to max(1, max |ref|)), output and input gradient, at K in {10, 64} and F
    in {7, 47, 128}: the 2e-5 of the device tests leaves the reference this margin."""
    worst = 0.0
    for F in (7, 47, 128):
        ei, w, n, x, go = _profile_problem(setting, F, 50 + F)
        perm = torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(F))
        for K in (10, 64):
            res = {}
            for dtype, order in ((torch.float64, slice(None)), (torch.float32, perm)):
                xd = x.to(dtype).requires_grad_(True)
                out = R.recurrence(ei[:, order], w[order].to(dtype), xd, xd, K, 0.9, 0.1)[0]
                res[dtype] = (out.detach(), torch.autograd.grad(out, xd, go.to(dtype))[0])
            for got, want in zip(res[torch.float32], res[torch.float64]):
                err = float((got.double() - want).abs().max())
                scale = max(1.0, float(want.abs().max()))
                worst = max(worst, err / scale)
                assert err <= 1e-5 * scale, (setting, F, K, err, scale)
    print(f'setting {setting}: worst float32 err / scale {worst:.2e}')
