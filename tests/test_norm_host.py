"""GraphNorm, LayerNorm, BatchNorm, the global pools and BasicGNN(norm=...) without a GPU: the class
surface, state dicts, every golden case of tests/golden/golden_norm_v1.pt through the generic
route on host tensors, the restatement of tests/_norm_ref.py against the same golden, the
resolver, the module tree of a model with a norm, the exported symbols and the argument statuses
of the C entry points."""
import ctypes
import os
import re

import pytest
import torch

import pytorch_geometric_amd.nn as nn
from pytorch_geometric_amd.nn.norm import normalization_resolver
from tests import _norm_ref as R
from tests._util import assert_close_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(R.load_golden()['cases'])


def test_class_surface():
    gn = nn.GraphNorm(12, eps=1e-4)
    assert [n for n, _ in gn.named_parameters()] == ['weight', 'bias', 'mean_scale']
    assert repr(gn) == 'GraphNorm(12)' and gn.eps == 1e-4 and gn.in_channels == 12
    with torch.no_grad():
        for p in gn.parameters():
            p.fill_(3.0)
    gn.reset_parameters()
    assert bool((gn.weight == 1).all() and (gn.bias == 0).all() and (gn.mean_scale == 1).all())
    ln = nn.LayerNorm(12)
    assert [n for n, _ in ln.named_parameters()] == ['weight', 'bias']
    assert repr(ln) == 'LayerNorm(12, affine=True, mode=graph)'
    plain = nn.LayerNorm(12, affine=False, mode='node')
    assert plain.weight is None and plain.bias is None and list(plain.state_dict()) == []
    assert repr(plain) == 'LayerNorm(12, affine=False, mode=node)'
    plain.reset_parameters()
    with pytest.raises(ValueError, match='Unknownn normalization mode'):
        nn.LayerNorm(12, mode='edge')(torch.randn(4, 12))
    bn = nn.BatchNorm(12, allow_single_element=True)
    assert list(bn.state_dict())[:2] == ['module.weight', 'module.bias']
    assert repr(bn).startswith('BatchNorm(12, eps=1e-05')
    assert bn(torch.randn(1, 12)).shape == (1, 12)      # one row, training mode
    with pytest.raises(ValueError, match='allow_single_element'):
        nn.BatchNorm(12, track_running_stats=False, allow_single_element=True)
    G = R.load_golden()
    assert repr(nn.GraphNorm(G['meta']['F'])) == G['reprs']['graph_norm']
    assert repr(nn.LayerNorm(G['meta']['F'])) == G['reprs']['layer_norm']
    assert repr(nn.LayerNorm(G['meta']['F'], affine=False, mode='node')) == \
        G['reprs']['layer_norm_node']


def test_state_dicts_interchange_with_the_reference_by_key_and_shape():
    G = R.load_golden()
    F = G['meta']['F']
    for name, layer in (('graph_norm', nn.GraphNorm(F)), ('layer_norm', nn.LayerNorm(F)),
                        ('layer_norm_no_affine', nn.LayerNorm(F, affine=False))):
        assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == G['keys'][name]
    layer = nn.GraphNorm(F)
    layer.load_state_dict(G['cases']['graph_norm_offset']['state'])
    assert torch.equal(layer.mean_scale, G['cases']['graph_norm_offset']['state']['mean_scale'])


@pytest.mark.parametrize('name', CASES)
def test_golden_cases_on_host_tensors(name):
    R.check_golden_case(name, 'cpu')


@pytest.mark.parametrize('name', [c for c in CASES if 'node' not in c])
def test_restatement_reproduces_the_golden_cases(name):
    G = R.load_golden()
    case = G['cases'][name]
    sizes = G['meta']['sizes'] if case['batch'] else [G['batch'].numel()]
    st = case['state']
    out, gx, gp = R.restate_with_grads(
        case['kind'], G['inputs'][case['x']], sizes, G['grad_out'],
        {k: st.get(k) for k in ('weight', 'bias', 'mean_scale')}, torch.float64,
        no_batch=not case['batch'])
    assert_close_scaled(out, case['out'].double(), tol=1e-6, what=f'{name} out')
    assert_close_scaled(gx, case['grad_x'].double(), tol=1e-6, what=f'{name} grad_x')
    for k, g in case['grad_params'].items():
        assert_close_scaled(gp[k], g, tol=1e-9, what=f'{name} grad_{k}')


def test_pools_on_host_tensors():
    R.check_pools('cpu')
    x = torch.randn(5, 3)
    assert nn.global_add_pool(x, None).shape == (1, 3)
    assert nn.global_mean_pool(x[:, 0], None).shape == (1, )
    assert nn.global_max_pool(x.view(1, 5, 3), None).shape == (1, 3)


def test_resolver_strings():
    for query, cls in (('graph_norm', nn.GraphNorm), ('GraphNorm', nn.GraphNorm),
                       ('graph', nn.GraphNorm), ('layer_norm', nn.LayerNorm),
                       ('LayerNorm', nn.LayerNorm), ('layer-norm', nn.LayerNorm),
                       ('batch_norm', nn.BatchNorm), ('BatchNorm', nn.BatchNorm),
                       ('batch', nn.BatchNorm)):
        layer = normalization_resolver(query, 8)
        assert type(layer) is cls and layer.in_channels == 8
    assert normalization_resolver('layer_norm', 8, mode='node').mode == 'node'
    module = torch.nn.LayerNorm(8)
    assert normalization_resolver(module, 8) is module
    with pytest.raises(ValueError, match='Could not resolve'):
        normalization_resolver('instance_norm', 8)


def test_basic_gnn_module_tree_with_and_without_a_norm():
    plain = nn.GCN(6, 8, 3, 4)
    assert not hasattr(plain, 'norms') and plain.supports_norm_batch is False
    assert not any(k.startswith('norms') for k in plain.state_dict())
    model = nn.GCN(6, 8, 3, 4, norm='graph_norm')
    assert [type(m).__name__ for m in model.norms] == ['GraphNorm', 'GraphNorm', 'Identity']
    assert model.norms[0] is not model.norms[1] and model.supports_norm_batch is True
    assert model.norms[0].in_channels == 8
    keys = [k for k in model.state_dict() if k.startswith('norms')]
    assert keys == [f'norms.{i}.{n}' for i in range(2) for n in ('weight', 'bias', 'mean_scale')]
    assert nn.GCN(6, 8, 2, norm='batch_norm').supports_norm_batch is False
    assert nn.GCN(6, 8, 2, norm='layer_norm', norm_kwargs=dict(mode='node')).norms[0].mode == 'node'
    mod = nn.GCN(6, 8, 2, norm=torch.nn.LayerNorm(8))
    assert type(mod.norms[0]) is torch.nn.LayerNorm and mod.norm is None
    sage = nn.GraphSAGE(6, 8, 3, norm='layer_norm')
    assert len(sage.norms) == 3
    with pytest.raises(NotImplementedError):
        nn.GCN(6, 8, 2, jk='cat')
    # batch and batch_size are keyword-only: positions 5 and 6 stay the per-hop counts
    import inspect
    sig = inspect.signature(nn.BasicGNN.forward).parameters
    assert list(sig)[5:7] == ['num_sampled_nodes_per_hop', 'num_sampled_edges_per_hop']
    assert sig['batch'].kind is sig['batch_size'].kind is inspect.Parameter.KEYWORD_ONLY
    # act_first / norm / act / dropout on every layer but the last (GCNConv has no host route: a
    # stack of stand-in layers that ignore the edges shows the order on host tensors)
    class Dense(torch.nn.Module):
        def __init__(self, i, o):
            super().__init__()
            self.lin = torch.nn.Linear(i, o)

        def reset_parameters(self):
            self.lin.reset_parameters()

        def forward(self, x, edge_index):
            return self.lin(x)

    class Stack(nn.BasicGNN):
        def init_conv(self, i, o, **kwargs):
            return Dense(i, o)

    x, ei = torch.randn(7, 6), torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]])
    batch = torch.tensor([0, 0, 0, 1, 1, 1, 1])
    for act_first in (False, True):
        model = Stack(6, 8, 3, 4, norm='graph_norm', act_first=act_first)
        h = x
        for i in range(2):
            h = model.convs[i](h, ei)
            h = model.norms[i](h.relu(), batch) if act_first else model.norms[i](h, batch).relu()
        assert torch.allclose(model(x, ei, batch=batch), model.convs[2](h, ei), atol=1e-6)
    # a norm without a batch argument is called with x alone
    assert Stack(6, 8, 2, norm='batch_norm')(x, ei, batch=batch).shape == (7, 8)


def test_layer_norm_without_a_batch_vector_differs_from_one_graph_with_one():
    """layer_norm.py:87-88 against :105: ``/ (std + eps)`` without a batch vector, ``/ sqrt(var +
    eps)`` with one; visible at a large eps"""
    x = torch.randn(40, 6, generator=torch.Generator().manual_seed(3)) * 0.1
    layer = nn.LayerNorm(6, eps=0.5)
    without = layer(x)
    with_batch = layer(x, torch.zeros(40, dtype=torch.long))
    c = x - x.mean()
    std = c.pow(2).mean().sqrt()
    assert torch.allclose(without, c / (std + 0.5), atol=1e-6)
    assert torch.allclose(with_batch, c / (std * std + 0.5).sqrt(), atol=1e-6)
    assert float((without - with_batch).detach().abs().max()) > 1e-2
    for no_batch, want in ((True, without), (False, with_batch)):
        assert torch.allclose(R.restate('layer_norm', x, [40], eps=0.5, no_batch=no_batch), want,
                              atol=1e-6)


def test_fuse_switch_is_read_at_import():
    import subprocess
    import sys
    code = ('import pytorch_geometric_amd.nn as nn; '
            'print(nn.GraphNorm(4).fuse, nn.LayerNorm(4).fuse)')
    for value, want in (('0', 'False False'), ('1', 'True True')):
        env = dict(os.environ, PYGAMD_FUSE_NORM=value)
        out = subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, check=True,
                             capture_output=True, text=True).stdout
        assert out.strip() == want


def test_symbols_are_exported_by_header_and_library():
    from pytorch_geometric_amd import _build, _lib
    text = open(os.path.join(ROOT, 'include', 'pyg_amd.h')).read()
    names = ('pygamd_graph_norm_supported', 'pygamd_graph_norm_forward',
             'pygamd_graph_norm_backward')
    for name in names:
        assert re.search(r'PYGAMD_API\s+int\s+' + name + r'\s*\(', text), name
        assert name in _lib.SIGNATURES
    assert 'graph_norm_workspace_bytes' not in text      # (the formula is stated, not queried)
    assert 'nn/norm/graph_norm.py:72-76' in text and 'nn/norm/layer_norm.py:82-108' in text
    assert 'graph_norm.hip' in _build.SOURCES and _lib.ABI_VERSION == 11
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name)


def test_operators_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import pytorch_geometric_amd.ops as ops
    assert 'graph_norm' in ops.OPS and 'graph_norm_backward' in ops.OPS
    with FakeTensorMode():
        x = torch.empty(30, 8, device='cuda', requires_grad=True)
        ptr = torch.empty(5, dtype=torch.int64, device='cuda')
        w = torch.empty(8, device='cuda')
        y, mean, rstd = torch.ops.pyg_amd.graph_norm(x, ptr, w, w, w, 1e-5, 'channel', False)
        assert y.shape == (30, 8) and mean.shape == rstd.shape == (4, 8) and y.requires_grad
        assert not mean.requires_grad and not rstd.requires_grad   # (statistics: no gradient)
        y, mean, rstd = torch.ops.pyg_amd.graph_norm(x, ptr, w, w, None, 1e-5, 'graph', True)
        assert y.shape == (30, 8) and mean.shape == rstd.shape == (4, )
        gx, gw, gb, gms = torch.ops.pyg_amd.graph_norm_backward(
            y, x, ptr, w, None, mean, rstd, 1e-5, 'graph', False, True)
        assert gx.shape == (30, 8) and gw.shape == gb.shape == (8, ) and gms.numel() == 0


def test_workspace_formula_matches_the_header():
    from pytorch_geometric_amd import _native
    text = open(os.path.join(ROOT, 'include', 'pyg_amd.h')).read()
    blocks = int(re.search(r'#define PYGAMD_GRAPH_NORM_BLOCKS (\d+)', text).group(1))
    assert blocks == _native.GRAPH_NORM_BLOCKS
    assert _native.graph_norm_workspace_bytes(7, 2, 20, False) == 8 * 20 * 7
    assert _native.graph_norm_workspace_bytes(7, 2, 20, True) == 4 * 20 * (14 + 6 + 3 * blocks)
    assert _native.graph_norm_workspace_bytes(0, 0, 20, False) == 0


def test_envelope_and_argument_checks_without_a_device():
    from pytorch_geometric_amd import _build, _lib, _native
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    P = ctypes.c_void_p
    assert [lib.pygamd_graph_norm_supported(f) for f in (0, 1, 512, 513)] == [0, 1, 1, 0]

    def handle(**kw):
        fields = dict(rowptr=16, col=None, idx_dtype=1, n_rows=3, n_hub=0, n_chunks=0,
                      hub_threshold=256, hub_chunk=128)
        fields.update(kw)
        return _lib.Csr(**fields)

    def fwd(g, F=8, ldx=8, mode=0, ws=None, nbytes=0, x=P(16), ms=None, std=0, ldy=None):
        return lib.pygamd_graph_norm_forward(
            None if g is None else ctypes.byref(g), mode, x, ldx, 10, F, None, None, ms, 1e-5, std,
            P(16), F if ldy is None else ldy, P(16), P(16), ws, nbytes, None)

    def bwd(g, F=8, mode=0, nbytes=0, ldg=8, gms=None, gy=P(16)):
        return lib.pygamd_graph_norm_backward(
            None if g is None else ctypes.byref(g), mode, P(16), F, gy, ldg, 10, F, None, None,
            1e-5, 0, P(16), P(16), P(16), F, None, None, gms, P(16), nbytes, None)

    g = handle()
    # status 1: no handle, a bad index type, a pitch under F, an unknown mode, a missing operand,
    # a parameter or flag of the other mode, F < 1, a plan that contradicts itself
    assert fwd(None) == 1 and bwd(None) == 1
    assert fwd(handle(idx_dtype=5)) == 1
    assert fwd(g, ldx=4) == 1 and fwd(g, ldy=7) == 1 and bwd(g, ldg=4, nbytes=1 << 20) == 1
    assert fwd(g, mode=2) == 1 and bwd(g, mode=-1) == 1
    assert fwd(g, x=None) == 1 and bwd(g, gy=None, nbytes=1 << 20) == 1
    assert fwd(g, mode=1, ms=P(16)) == 1 and fwd(g, std=1) == 1
    assert bwd(g, mode=1, gms=P(16), nbytes=1 << 20) == 1
    assert fwd(g, F=0, ldx=0) == 1
    assert fwd(handle(n_chunks=3)) == 1 and fwd(handle(n_hub=1, n_chunks=2)) == 1
    # status 2: past the envelope
    assert fwd(g, F=513, ldx=513) == 2 and bwd(g, F=513, ldg=513) == 2
    # status 3: a workspace under the header's formula (forward: only with hub graphs)
    hub = handle(hub_rows=16, hub_chunk_ptr=16, n_hub=1, n_chunks=4)
    need = _native.graph_norm_workspace_bytes(4, 1, 8, False)
    assert fwd(hub, ws=P(16), nbytes=need - 1) == 3 and fwd(hub) == 3
    assert bwd(g, nbytes=_native.graph_norm_workspace_bytes(0, 0, 8, True) - 1) == 3
    assert bwd(hub, nbytes=_native.graph_norm_workspace_bytes(4, 1, 8, True) - 1) == 3
    # a handle without rows: nothing to do
    empty = handle(rowptr=None, n_rows=0)
    assert fwd(empty) == 0 and bwd(empty) == 0


def test_generic_route_serves_what_the_kernel_does_not():
    """float64 host tensors, an unsorted batch vector and a model on host tensors all take the
    reference's arithmetic"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(30, 5, generator=g, dtype=torch.float64)
    batch = torch.randint(0, 4, (30, ), generator=g)
    order = batch.argsort(stable=True)
    for layer, kind in ((nn.GraphNorm(5).double(), 'graph_norm'),
                        (nn.LayerNorm(5).double(), 'layer_norm')):
        got = layer(x, batch)
        sizes = torch.bincount(batch, minlength=4).tolist()
        want = R.restate(kind, x[order], sizes, **dict(layer.named_parameters()))
        assert torch.allclose(got[order], want, atol=1e-12)
