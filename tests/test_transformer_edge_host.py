"""nn.TransformerConv with edge features inside the fused kernels: everything that needs no
device.  The recorded reference cases (tests/golden/golden_transformer_edge_v1.pt, with the
gradient of ``edge_attr``) against the float64 restatement and against the class on host tensors;
the ``fuse_edge`` switch; the ``supported`` predicate at its limits; the argument checks of the new
entry points."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import _transformer_edge_ref as RE
import _transformer_ref as R
from _util import assert_close, csr_arg


def test_golden_file_is_what_the_tests_expect():
    G = RE.load_golden()
    assert list(G['cases']) == RE.CASES
    assert G['x'].shape == (48, 16) and G['edge_index'].shape == (2, 400)
    assert G['x_dst'].shape == (20, 12) and G['edge_attr'].shape == (400, 9)
    old = R.load_golden()
    assert torch.equal(G['edge_index'], old['edge_index']) and torch.equal(G['x'], old['x'])
    kw = {n: c['kwargs'] for n, c in G['cases'].items()}
    assert all(k['edge_dim'] == (9 if n == 'e_wide' else 3) for n, k in kw.items())
    assert kw['e'] == dict(heads=2, out_channels=6, edge_dim=3, in_channels=16)
    assert kw['e_mean']['concat'] is False and kw['e_beta']['beta'] is True
    assert kw['e_noroot']['root_weight'] is False and kw['e_nobias']['bias'] is False
    assert kw['e_pair']['in_channels'] == (16, 12) and G['cases']['e_pair']['pair']
    assert G['cases']['e_attention']['attention'][1].shape == (400, 2)
    for name, c in G['cases'].items():
        assert c['grad_edge_attr'].shape == (400, c['kwargs']['edge_dim']), name
        assert 'lin_edge.weight' in c['grad_params'], name
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                        'golden_transformer_edge_v1.pt')) < 2 ** 20


@pytest.mark.parametrize('name', RE.CASES)
def test_golden_matches_the_float64_restatement(name):
    G = RE.load_golden()
    case = G['cases'][name]
    xs, ei, ea = RE.case_inputs(G, case)
    xs = [t.double().requires_grad_(True) for t in xs]
    ea = ea.double().requires_grad_(True)
    p = {k: v.double().requires_grad_(True) for k, v in case['state'].items()}
    out, alpha = R.conv(tuple(xs) if case['pair'] else xs[0], ei, p, edge_attr=ea,
                        **{k: v for k, v in case['kwargs'].items() if k != 'in_channels'})
    assert_close(out.float(), case['out'], what=f'{name} out')
    names = list(case['grad_params'])
    grads = torch.autograd.grad(out, xs + [ea] + [p[n] for n in names], case['grad_out'].double())
    for g, ref in zip(grads, case['grad_x']):
        assert_close(g.float(), ref, what=f'{name} grad_x')
    assert_close(grads[len(xs)].float(), case['grad_edge_attr'], what=f'{name} grad_edge_attr')
    for n, g in zip(names, grads[len(xs) + 1:]):
        assert_close(g.float(), case['grad_params'][n], atol=5e-5, rtol=5e-5,
                     what=f'{name} grad {n}')
    if 'attention' in case:
        assert torch.equal(ei, case['attention'][0])
        assert_close(alpha.float(), case['attention'][1], what=f'{name} attention')


@pytest.mark.parametrize('name', RE.CASES)
def test_class_on_host_tensors_matches_the_reference(name):
    """host tensors compute in plain torch whatever ``fuse_edge`` says"""
    for fuse_edge in (False, True):
        RE.check_class_case(RE.load_golden(), name, 'cpu', fuse_edge=fuse_edge)


def test_decomposition_equals_the_direct_formula():
    """b = scale W_e^T q and out = out_nodes + W_e z restate key_j + e, value_j + e exactly."""
    g = torch.Generator().manual_seed(5)
    H, C, De, n, E = 3, 5, 7, 30, 200
    q, k, v = [torch.randn(n, H, C, generator=g, dtype=torch.float64) for _ in range(3)]
    a = torch.randn(E, De, generator=g, dtype=torch.float64)
    w_e = torch.randn(H * C, De, generator=g, dtype=torch.float64)
    ei = torch.randint(0, n, (2, E), generator=g)
    want, want_alpha = R.attend(q, k, v, ei, n, e=(a @ w_e.t()).view(E, H, C))
    w3 = w_e.view(H, C, De)
    b = torch.einsum('nhc,hcd->nhd', q, w3) / C ** 0.5
    out, z, alpha = RE.attend_edge(q, k, v, a, b, ei, n)
    assert_close(out + torch.einsum('nhd,hcd->nhc', z, w3), want, rtol=1e-12, atol=1e-12)
    assert_close(alpha, want_alpha, rtol=1e-12, atol=1e-12)


def test_fuse_edge_is_off_by_default_and_follows_the_environment():
    from pytorch_geometric_amd.nn import TransformerConv
    from pytorch_geometric_amd.nn.conv import transformer_conv
    here = os.environ.get('PYGAMD_FUSE_EDGE', '0') not in ('', '0')
    assert transformer_conv.FUSE_EDGE is here
    layer = TransformerConv(8, 4, heads=2, edge_dim=3)
    assert layer.fuse_edge is here and layer.fuse
    if 'PYGAMD_FUSE_EDGE' not in os.environ:
        assert layer.fuse_edge is False                     # the default
    code = ('from pytorch_geometric_amd.nn import TransformerConv; '
            'print(TransformerConv(8, 4, heads=2, edge_dim=3).fuse_edge)')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (('1', 'True'), ('0', 'False')):
        env = dict(os.environ, PYGAMD_FUSE_EDGE=value,
                   PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
        res = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True,
                             text=True, cwd=root)
        assert res.returncode == 0, res.stderr
        assert res.stdout.split()[-1] == want, (value, res.stdout)


def _lib_or_skip():
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    return _lib.load()


def test_supported_predicate_at_its_limits():
    from pytorch_geometric_amd import _native
    lib = _lib_or_skip()
    want = {
        # De <= 32 for H <= 8 with C >= 8
        (8, 8, 32): 1, (8, 64, 32): 1, (8, 8, 33): 0, (5, 8, 32): 1, (1, 8, 32): 1, (4, 128, 32): 1,
        # the narrowest lane share: H = 64 leaves one lane per head, four edge registers
        (64, 8, 2): 1, (64, 8, 4): 1, (64, 8, 5): 0,
        # between: 4 * (largest power of two with H * lph <= 64)
        (16, 8, 16): 1, (16, 8, 17): 0, (9, 8, 16): 1, (9, 8, 17): 0, (3, 5, 64): 1, (3, 5, 65): 0,
        (2, 6, 9): 1, (1, 8, 1): 1,
        # no edge features, and the head layouts the kernels do not serve at all
        (2, 8, 0): 0, (2, 8, -1): 0, (8, 128, 4): 0, (65, 1, 1): 0, (0, 4, 2): 0,
    }
    for (H, C, De), ok in want.items():
        assert lib.pygamd_transformer_edge_supported(H, C, De) == ok, (H, C, De)
        assert _native.transformer_edge_supported(H, C, De) is bool(ok)
        if ok:
            assert lib.pygamd_transformer_supported(H, C) == 1


def test_entry_points_validate_without_gpu():
    """pygamd_transformer_edge_* reject bad arguments with status 1 / 2 / 3 before any device
    work."""
    lib = _lib_or_skip()
    dev = ctypes.c_void_p(16)   # (never dereferenced: every call below is rejected or launches nothing)
    nbytes = ctypes.c_size_t(0)
    ws_bytes = lib.pygamd_transformer_edge_workspace_bytes
    assert ws_bytes(3, 4, 8, 6, ctypes.byref(nbytes)) == 0
    # forward partials (acc, z, m, l) + statistics; by destination (grad_query, grad_b) + D
    assert nbytes.value >= 4 * 3 * max(32 + 24 + 8 + 8, 32 + 24 + 4)
    assert ws_bytes(0, 4, 8, 6, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    assert ws_bytes(3, 4, 8, 6, None) == 1 and ws_bytes(-1, 4, 8, 6, ctypes.byref(nbytes)) == 1
    assert ws_bytes(3, 4, 8, 0, ctypes.byref(nbytes)) == 1
    assert ws_bytes(3, 8, 128, 6, ctypes.byref(nbytes)) == 2
    assert ws_bytes(3, 64, 8, 5, ctypes.byref(nbytes)) == 2

    def fwd(rowptr=dev, idx=1, query=dev, key=dev, value=dev, ld=32, ea=dev, bias=dev, n_rows=5,
            H=4, C=8, De=6, hub_rows=None, n_hub=0, n_chunks=0, alpha=dev, out=dev, z=dev,
            ws=None, ws_bytes=0):
        g = csr_arg(rowptr=rowptr, col=dev, idx_dtype=idx, n_rows=n_rows, hub_rows=hub_rows,
                    hub_chunk_ptr=hub_rows, n_hub=n_hub, n_chunks=n_chunks, hub_threshold=1024,
                    hub_chunk=256)
        return lib.pygamd_transformer_edge_forward(
            g, query, key, value, ld, ea, bias, 9, H, C, De, 0.35, alpha, out, z, ws, ws_bytes,
            None)

    assert lib.pygamd_transformer_edge_forward(None, dev, dev, dev, 32, dev, dev, 9, 4, 8, 6, 0.35,
                                               dev, dev, dev, None, 0, None) == 1   # no descriptor
    assert fwd(rowptr=None) == 1 and fwd(query=None) == 1 and fwd(key=None) == 1
    assert fwd(ea=None) == 1 and fwd(bias=None) == 1 and fwd(alpha=None) == 1
    assert fwd(value=None) == 1                                 # aggregation asked for, no values
    assert fwd(z=None) == 1 and fwd(out=None) == 1              # out and z come together
    assert fwd(ld=31) == 1 and fwd(De=0) == 1 and fwd(De=-3) == 1
    assert fwd(idx=5) == 1 and fwd(n_rows=-1) == 1 and fwd(H=0) == 1 and fwd(C=0) == 1
    assert fwd(H=8, C=128, ld=1024) == 2 and fwd(H=65, C=1, ld=65) == 2
    assert fwd(De=65) == 2 and fwd(H=64, C=8, ld=512, De=5) == 2
    assert fwd(n_hub=2, n_chunks=8) == 1 and fwd(n_hub=0, n_chunks=3) == 1
    assert fwd(hub_rows=dev, n_hub=2, n_chunks=1) == 1          # fewer chunks than hub rows
    assert fwd(hub_rows=dev, n_hub=2, n_chunks=8) == 3          # no workspace for the partials
    assert fwd(hub_rows=dev, n_hub=2, n_chunks=8, ws=dev, ws_bytes=64) == 3
    assert fwd(n_rows=0) == 0                                   # no rows: nothing to launch

    def bwd(key=dev, value=dev, ld=32, ea=dev, bias=dev, grad_out=dev, out=dev, grad_z=dev, z=dev,
            grad_alpha=None, H=4, C=8, De=6, n_rows=5, grad_s=dev, grad_query=dev, grad_bias=dev,
            grad_ea=dev, hub_rows=None, n_hub=0, n_chunks=0, ws=None, ws_bytes=0):
        g = csr_arg(rowptr=dev, col=dev, idx_dtype=1, n_rows=n_rows, hub_rows=hub_rows,
                    hub_chunk_ptr=hub_rows, n_hub=n_hub, n_chunks=n_chunks, hub_threshold=1024,
                    hub_chunk=256)
        return lib.pygamd_transformer_edge_backward_dst(
            g, key, value, ld, ea, bias, dev, grad_out, out, grad_z, z, grad_alpha, 9, H, C, De,
            0.35, grad_s, grad_query, grad_bias, grad_ea, ws, ws_bytes, None)

    assert lib.pygamd_transformer_edge_backward_dst(
        None, dev, dev, 32, dev, dev, dev, dev, dev, dev, dev, None, 9, 4, 8, 6, 0.35, dev, dev,
        dev, dev, None, 0, None) == 1
    assert bwd(grad_out=None) == 1 and bwd(out=None) == 1
    assert bwd(grad_z=None) == 1 and bwd(z=None) == 1
    assert bwd(grad_alpha=dev) == 1                             # both sources of d alpha given
    assert bwd(grad_out=None, out=None, grad_z=None, z=None, grad_alpha=None) == 1
    assert bwd(grad_out=None, out=None, grad_alpha=dev) == 1    # score mode takes no grad_z / z
    assert bwd(key=None) == 1 and bwd(value=None) == 1 and bwd(ea=None) == 1
    assert bwd(bias=None) == 1 and bwd(grad_s=None) == 1 and bwd(grad_query=None) == 1
    assert bwd(grad_bias=None) == 1 and bwd(ld=8) == 1 and bwd(De=0) == 1 and bwd(n_rows=-2) == 1
    assert bwd(H=8, C=128, ld=1024) == 2 and bwd(De=65) == 2
    assert bwd(hub_rows=dev, n_hub=1, n_chunks=5) == 3
    assert bwd(hub_rows=dev, n_hub=1, n_chunks=5, ws=dev, ws_bytes=16) == 3
    assert bwd(n_rows=0) == 0 and bwd(n_rows=0, grad_ea=None) == 0
