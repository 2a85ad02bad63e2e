"""nn.GMMConv and nn.NNConv on host tensors: the float32 restatement and both classes against
every recorded reference case (tests/golden/golden_mixture_v1.pt), the state-dict keys, the refusal
of lazy initialisation, the fusability predicate with the C-ABI calls counted, the exported
symbols, the registered operators and the envelope and argument checks of the
``pygamd_mixture_*`` entry points.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import _mixture_ref as R

SYMBOLS = ['pygamd_mixture_supported', 'pygamd_mixture_workspace_bytes', 'pygamd_mixture_expand',
           'pygamd_mixture_coef_grad']


@pytest.mark.parametrize('name', R.CASES)
def test_restatement_reproduces_the_golden_cases(name):
    R.check_restatement_case(R.load_golden(), name)


def test_restated_kernels_agree_with_the_restated_operator():
    """expand, then the dense product, is mixture_conv; coef_grad is its gradient (float64)"""
    g = torch.Generator().manual_seed(3)
    n_src, n_dst, E, F, K, M = 30, 20, 200, 5, 3, 4
    src, dst = torch.randint(0, n_src, (E, ), generator=g), torch.randint(0, n_dst, (E, ), generator=g)
    x = torch.randn(n_src, F, generator=g, dtype=torch.float64).requires_grad_(True)
    coef = torch.randn(E, K, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(K, F, M, generator=g, dtype=torch.float64).requires_grad_(True)
    go = torch.randn(n_dst, M, generator=g, dtype=torch.float64)
    out = R.mixture_conv(x, coef, w, src, dst, n_dst)
    z = R.expand(x, coef, src, dst, n_dst)
    assert torch.allclose(out, z @ w.reshape(K * F, M), atol=1e-12)
    g_x, g_c, g_w = torch.autograd.grad(out, [x, coef, w], go)
    wide = go @ w.reshape(K * F, M).t()
    assert torch.allclose(g_c, R.coef_grad(wide, x, src, dst), atol=1e-12)
    assert torch.allclose(g_w.reshape(K * F, M), z.t() @ go, atol=1e-12)
    t = R.expand(go, coef, dst, src, n_src)                  # the transposed handle
    assert torch.allclose(g_x, t @ w.permute(0, 2, 1).reshape(K * M, F), atol=1e-12)


@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_host_tensors(monkeypatch, name):
    """the generic route, whatever the layer's switch says: no mixture call is made"""
    G = R.load_golden()
    state = {}
    calls = _call_counts_cpu(monkeypatch, lambda: state.update(
        layer=R.check_class_case(G, name, 'cpu')))
    assert not [n for n in calls if 'mixture_expand' in n or 'mixture_coef' in n], calls
    assert repr(state['layer']) == G['cases'][name]['repr']


def _call_counts_cpu(monkeypatch, fn):
    """``_util._call_counts`` without its device synchronisation"""
    from _util import CountingLib
    from pytorch_geometric_amd import _lib
    counter = CountingLib(_lib.load())
    monkeypatch.setattr(_lib, 'load', lambda: counter)
    try:
        fn()
    finally:
        monkeypatch.undo()
    return counter.calls


def test_state_dicts_load_both_ways_with_the_reference_keys():
    from pytorch_geometric_amd.nn import GMMConv, NNConv
    from pytorch_geometric_amd.nn.conv import GMMConv as G2, NNConv as N2
    assert GMMConv is G2 and NNConv is N2
    G = R.load_golden()
    for name in R.CASES:
        case = G['cases'][name]
        layer = R.make_layer(case)                      # reference -> this package (strict)
        back = layer.state_dict()
        assert list(back) == list(case['state'])
        for k, v in case['state'].items():
            assert back[k].shape == v.shape and back[k].dtype == v.dtype, (name, k)
            assert torch.equal(back[k], v)
    layer = GMMConv((16, 12), 8, dim=2, kernel_size=5)
    assert list(layer.state_dict()) == ['g', 'mu', 'sigma', 'bias', 'root.weight']
    assert layer.g.shape == (16, 40) and layer.mu.shape == (5, 2) and layer.sigma.shape == (5, 2)
    assert layer.root.weight.shape == (8, 12) and layer.aggr == 'mean'
    assert float(layer.bias.detach().abs().max()) == 0.0
    bound = (6.0 / (16 + 40)) ** 0.5                                        # glorot
    assert float(layer.g.detach().abs().max()) <= bound
    sep = GMMConv(4, 3, dim=2, kernel_size=5, separate_gaussians=True)
    assert sep.mu.shape == (4, 3, 5, 2) and sep.sigma.shape == (4, 3, 5, 2)
    bare = GMMConv(4, 4, dim=1, kernel_size=2, root_weight=False, bias=False)
    assert bare.root is None and bare.bias is None
    assert list(bare.state_dict()) == ['g', 'mu', 'sigma']
    net = torch.nn.Sequential(torch.nn.Linear(3, 7), torch.nn.ReLU(), torch.nn.Linear(7, 16 * 8))
    layer = NNConv((16, 12), 8, net)
    assert list(layer.state_dict()) == ['bias', 'nn.0.weight', 'nn.0.bias', 'nn.2.weight',
                                        'nn.2.bias', 'lin.weight']
    assert layer.lin.weight.shape == (8, 12) and layer.aggr == 'add' and layer.nn is net
    before = net[0].weight.detach().clone()
    layer.reset_parameters()                                 # resets the children of `nn` too
    assert not torch.equal(net[0].weight.detach(), before)
    bare = NNConv(4, 4, torch.nn.Linear(2, 16), root_weight=False, bias=False)
    assert bare.lin is None and bare.bias is None
    assert list(bare.state_dict()) == ['nn.weight', 'nn.bias']


def test_lazy_initialisation_is_refused():
    from pytorch_geometric_amd.nn import GMMConv, Linear, NNConv
    with pytest.raises(ValueError) as ref:
        Linear(-1, 4)
    for make in (lambda: GMMConv(-1, 4, dim=2, kernel_size=3),
                 lambda: GMMConv((-1, 4), 4, dim=2, kernel_size=3),
                 lambda: NNConv(-1, 4, torch.nn.Linear(2, 16)),
                 lambda: NNConv((8, -1), 4, torch.nn.Linear(2, 32))):
        with pytest.raises(ValueError) as err:
            make()
        assert str(err.value) == str(ref.value)


def test_fuse_switch_is_read_at_import():
    from pytorch_geometric_amd.nn import GMMConv, NNConv
    from pytorch_geometric_amd.nn.conv import gmm_conv as M
    want = os.environ.get('PYGAMD_FUSE_MIXTURE', '1') not in ('', '0')
    assert M.FUSE_MIXTURE is want
    assert GMMConv(4, 4, dim=2, kernel_size=3).fuse is want
    assert NNConv(4, 4, torch.nn.Linear(2, 16)).fuse is want


def test_fusability_predicate_without_a_device(monkeypatch):
    """the conditions of NNConv's fused route that need no tensor — the switch, hooks, a subclass's
    own ``message``, the edge network's shape, the envelope and the byte rule on both sides of its
    boundary — and GMMConv's; host tensors never reach a mixture kernel"""
    from pytorch_geometric_amd.nn import GMMConv, NNConv
    F, M = 16, 8
    mlp = lambda k=10, bias=True: torch.nn.Sequential(                       # noqa: E731
        torch.nn.Linear(3, k), torch.nn.ReLU(), torch.nn.Linear(k, F * M, bias=bias))

    def ok(layer, n_src=48, n_dst=48, E=400):
        layer.fuse = True
        return layer._fusable_shapes(n_src, n_dst, E)

    assert ok(NNConv(F, M, mlp())) and ok(NNConv(F, M, torch.nn.Linear(3, F * M)))
    assert ok(NNConv(F, M, mlp(bias=False))) and ok(NNConv(F, M, mlp(), aggr='mean'))
    from pytorch_geometric_amd.nn import Linear
    assert ok(NNConv(F, M, Linear(3, F * M)))
    layer = NNConv(F, M, mlp())
    layer.fuse = False
    assert not layer._fusable_shapes(48, 48, 400)
    assert not ok(NNConv(F, M, mlp(), aggr='max'))
    assert not ok(NNConv(F, M, mlp(), flow='target_to_source'))
    assert not ok(NNConv(F, M, torch.nn.Sequential(torch.nn.Linear(3, F * M), torch.nn.ReLU())))
    assert not ok(NNConv(F, M, mlp()[:2]))                                   # ends in ReLU
    assert not ok(NNConv(F, M, torch.nn.Sequential(torch.nn.Linear(3, 10), torch.nn.ReLU(),
                                                   torch.nn.Linear(10, F * M + 1))))
    assert not ok(NNConv(F, M, torch.nn.Tanh()))
    for hook_on in ('net', 'last', 'pre'):
        net = mlp()
        if hook_on == 'net':
            net.register_forward_hook(lambda *a: None)
        elif hook_on == 'last':
            net[2].register_forward_hook(lambda *a: None)
        else:
            net[2].register_forward_pre_hook(lambda *a: None)
        assert not ok(NNConv(F, M, net)), hook_on
    net = mlp()
    net[0].register_forward_hook(lambda *a: None)            # (a child that is run as it is)
    assert ok(NNConv(F, M, net))
    layer = NNConv(F, M, mlp())
    layer.register_message_forward_hook(lambda *a: None)
    assert not ok(layer)

    class Own(NNConv):
        def message(self, x_j, edge_attr):
            return 2 * super().message(x_j, edge_attr)

    assert not ok(Own(F, M, mlp()))
    # the envelope: K' = in_features + 1 <= 256 at max(F, M) <= 512
    assert ok(NNConv(F, M, mlp(255)), E=10 ** 6) and not ok(NNConv(F, M, mlp(256)), E=10 ** 6)
    wide = torch.nn.Linear(3, 513 * 2)
    assert not ok(NNConv(513, 2, wide), E=10 ** 6) and not ok(NNConv(2, 513, wide), E=10 ** 6)
    # the byte rule, K' = 11: K' * N_dst <= E * M and K' * N_src <= E * F
    layer = NNConv(F, M, mlp())
    assert ok(layer, n_src=10, n_dst=800, E=1100) and not ok(layer, n_src=10, n_dst=801, E=1100)
    assert ok(layer, n_src=1600, n_dst=10, E=1100) and not ok(layer, n_src=1601, n_dst=10, E=1100)
    # host tensors: the generic route; the predicate's tensor half says no before any C call
    x, ei, ea = torch.randn(48, F), torch.randint(0, 48, (2, 400)), torch.randn(400, 3)
    layer = NNConv(F, M, mlp())
    layer.fuse = True
    calls = _call_counts_cpu(monkeypatch, lambda: layer(x, ei, ea).sum().backward())
    assert not [n for n in calls if 'mixture' in n], calls
    gmm = GMMConv(F, M, dim=2, kernel_size=3)
    gmm.fuse = True
    calls = _call_counts_cpu(monkeypatch,
                             lambda: gmm(x, ei, torch.randn(400, 2)).sum().backward())
    assert not [n for n in calls if 'mixture' in n], calls
    assert not gmm._fusable(x, x, torch.randn(400, 2))


def test_symbols_are_exported_by_header_and_library():
    from pytorch_geometric_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'pyg_amd.h')) as f:
        text = f.read()
    for sym in SYMBOLS:
        assert re.search(r'PYGAMD_API\s+int\s+' + sym + r'\s*\(', text), sym
        assert sym in _lib.SIGNATURES, sym
    assert 'gmm_conv.py:154-165' in text and 'nn_conv.py:119-122' in text
    assert 'mixture.hip' in _build.SOURCES and _lib.ABI_VERSION == 11
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
    assert 'mixture_conv' in ops.OPS and 'mixture_conv_backward' in ops.OPS
    assert 'mixture_conv' in ops.__doc__
    schema = str(torch.ops.pyg_amd.mixture_conv.default._schema)
    assert schema == ('pyg_amd::mixture_conv(Tensor x_src, Tensor coef, Tensor weight, '
                      'Tensor rowptr, Tensor col, Tensor? edge_id) -> Tensor')
    with FakeTensorMode():
        x, coef, w = torch.empty(9, 8), torch.empty(30, 3), torch.empty(3, 8, 5)
        ptr, col = torch.empty(8, dtype=torch.int64), torch.empty(30, dtype=torch.int64)
        out = torch.ops.pyg_amd.mixture_conv(x, coef, w, ptr, col, None)
        assert out.shape == (7, 5)
        grads = torch.ops.pyg_amd.mixture_conv_backward(out, x, coef, w, ptr, col, None, True,
                                                        True, True)
        assert [tuple(g.shape) for g in grads] == [(9, 8), (30, 3), (3, 8, 5)]
        grads = torch.ops.pyg_amd.mixture_conv_backward(out, x, coef, w, ptr, col, None, False,
                                                        True, False)
        assert [tuple(g.shape) for g in grads] == [(0, ), (30, 3), (0, )]


def test_envelope_and_argument_checks_without_a_device():
    """1 <= F <= 512 and 1 <= K <= 256.  Status 1 / 2 / 3 before any device work, 0 for a handle
    without rows."""
    from _util import csr_arg
    from pytorch_geometric_amd import _build, _lib, _native
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    ok = lib.pygamd_mixture_supported
    assert ok(1, 1) == 1 and ok(512, 256) == 1 and ok(512, 1) == 1 and ok(1, 256) == 1
    assert ok(513, 1) == 0 and ok(1, 257) == 0 and ok(0, 1) == 0 and ok(1, 0) == 0
    assert ok(-3, 4) == 0 and ok(4, -3) == 0
    assert _native.mixture_supported(64, 25) and not _native.mixture_supported(64, 300)
    dev = ctypes.c_void_p(16)   # (never dereferenced: every call below is rejected or launches nothing)

    def expand(g, F=8, K=3, ld_x=8, x=dev, coef=dev, z=dev, ws=None, ws_bytes=0):
        return lib.pygamd_mixture_expand(g, None, x, ld_x, coef, 9, F, K, z, ws, ws_bytes, None)

    def cgrad(g, F=8, K=3, ld_x=8, wide=dev, x=dev, out=dev):
        return lib.pygamd_mixture_coef_grad(g, None, wide, x, ld_x, 9, F, K, out, None)

    assert expand(None) == 1 and cgrad(None) == 1
    empty = dict(rowptr=dev, col=dev, idx_dtype=1, n_rows=0, hub_threshold=1024, hub_chunk=256)
    e = lambda **kw: csr_arg(**dict(empty, **kw))                            # noqa: E731
    assert expand(e()) == 0 and cgrad(e()) == 0                              # no rows: nothing to launch
    assert expand(e(idx_dtype=5)) == 1 and cgrad(e(n_hub=0, n_chunks=3)) == 1
    assert expand(e(), F=513) == 2 and cgrad(e(), K=257) == 2
    assert expand(e(), F=0) == 1 and cgrad(e(), K=0) == 1
    assert expand(e(), ld_x=7) == 1 and cgrad(e(), ld_x=7) == 1              # stride below the width
    rows = lambda **kw: e(n_rows=4, **kw)                                    # noqa: E731
    assert expand(rows(), x=None) == 1 and expand(rows(), coef=None) == 1
    assert expand(rows(), z=None) == 1
    assert cgrad(rows(), wide=None) == 1 and cgrad(rows(), out=None) == 1
    hub = dict(n_rows=4, hub_rows=dev, hub_chunk_ptr=dev, n_hub=1, n_chunks=5)
    assert expand(e(**hub)) == 3
    assert expand(e(**hub), ws=dev, ws_bytes=5 * 3 * 8 * 4 - 1) == 3
    n = ctypes.c_size_t(0)
    size = lib.pygamd_mixture_workspace_bytes
    assert size(5, 8, 3, ctypes.byref(n)) == 0 and n.value == 5 * 3 * 8 * 4
    assert size(0, 8, 3, ctypes.byref(n)) == 0 and n.value == 0
    assert size(0, 8, 3, None) == 1 and size(-1, 8, 3, ctypes.byref(n)) == 1
    assert size(0, 1024, 3, ctypes.byref(n)) == 2 and size(0, 8, 257, ctypes.byref(n)) == 2
