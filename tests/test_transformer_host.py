"""nn.TransformerConv: everything that needs no device.  The class on host tensors and the
plain-torch restatement (tests/_transformer_ref.py) are pinned to the reference's recorded results
(tests/golden/golden_transformer_v1.pt); state dicts interchange with the reference; the argument
checks of the new entry points."""
import ctypes

import pytest
import torch

import _transformer_ref as R
from _util import assert_close, csr_arg

CASES = ['t', 't_mean', 't_beta', 't_beta_mean', 't_noroot', 't_nobias', 't_c5', 't_pair', 't_edge',
         't_attention']


def test_golden_file_is_what_the_tests_expect():
    G = R.load_golden()
    assert list(G['cases']) == CASES
    assert G['x'].shape == (48, 16) and G['edge_index'].shape == (2, 400)
    assert G['x_dst'].shape == (20, 12) and G['edge_attr'].shape == (400, 3)
    deg = torch.bincount(G['edge_index'][1], minlength=48)
    assert int((deg == 0).sum()) > 0 and int(deg.max()) > 40           # empty rows, a long row
    assert G['cases']['t']['kwargs'] == dict(heads=4, out_channels=6, in_channels=16)
    assert G['cases']['t_c5']['kwargs'] == dict(heads=3, out_channels=5, in_channels=16)
    assert G['cases']['t_attention']['attention'][1].shape == (400, 2)


@pytest.mark.parametrize('name', CASES)
def test_class_on_host_tensors_matches_the_reference(name):
    R.check_class_case(R.load_golden(), name, 'cpu')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_restatement_reproduces_every_golden_case(dtype):
    G = R.load_golden()
    for name in CASES:
        case = G['cases'][name]
        xs, ei, ea = R.case_inputs(G, case)
        xs = [t.to(dtype).requires_grad_(True) for t in xs]
        p = {k: v.to(dtype).requires_grad_(True) for k, v in case['state'].items()}
        out, alpha = R.conv(tuple(xs) if case['pair'] else xs[0], ei, p,
                            edge_attr=None if ea is None else ea.to(dtype),
                            **{k: v for k, v in case['kwargs'].items() if k != 'in_channels'})
        assert_close(out.float(), case['out'], what=f'{name} out')
        names = list(case['grad_params'])
        grads = torch.autograd.grad(out, xs + [p[n] for n in names], case['grad_out'].to(dtype))
        for g, ref in zip(grads, case['grad_x']):
            assert_close(g.float(), ref, what=f'{name} grad_x')
        for n, g in zip(names, grads[len(xs):]):
            assert_close(g.float(), case['grad_params'][n], atol=5e-5, rtol=5e-5,
                         what=f'{name} grad {n}')
        if 'attention' in case:
            assert torch.equal(ei, case['attention'][0])
            assert_close(alpha.float(), case['attention'][1], what=f'{name} attention')


def test_state_dict_and_structure():
    from pytorch_geometric_amd.nn import Linear, TransformerConv
    from pytorch_geometric_amd.nn.conv import TransformerConv as FromConv
    assert FromConv is TransformerConv
    G = R.load_golden()
    for name in CASES:
        case = G['cases'][name]
        kw = dict(case['kwargs'])
        layer = TransformerConv(kw.pop('in_channels'), **kw)
        assert list(layer.state_dict()) == list(case['state']), name   # the reference's keys
        for k, v in layer.state_dict().items():
            assert v.shape == case['state'][k].shape, (name, k)
        layer.load_state_dict(case['state'])
    plain = TransformerConv((8, 6), 4, heads=2, bias=False, edge_dim=3)
    assert plain.lin_key.weight.shape == (8, 8) and plain.lin_value.weight.shape == (8, 8)
    assert plain.lin_query.weight.shape == (8, 6) and plain.lin_skip.weight.shape == (8, 6)
    assert plain.lin_key.bias is None and plain.lin_skip.bias is None
    assert isinstance(plain.lin_edge, Linear) and plain.lin_edge.bias is None
    assert plain.lin_beta is None and 'lin_beta.weight' not in plain.state_dict()
    assert repr(plain) == 'TransformerConv((8, 6), 4, heads=2)' and plain.fuse
    mean = TransformerConv(8, 4, heads=2, concat=False, beta=True)
    assert mean.lin_skip.weight.shape == (4, 8) and mean.lin_beta.weight.shape == (1, 12)
    assert TransformerConv(8, 4, heads=2, beta=True).lin_beta.weight.shape == (1, 24)
    assert TransformerConv(8, 4).lin_edge is None and TransformerConv(8, 4).aggr == 'add'


def test_beta_needs_the_root_weight():
    """``self.beta = beta and root_weight`` (transformer_conv.py:119): without the skip term there is
    nothing to gate, so the gate's parameter does not exist."""
    from pytorch_geometric_amd.nn import TransformerConv
    for concat in (True, False):
        layer = TransformerConv(8, 4, heads=2, beta=True, root_weight=False, concat=concat)
        assert layer.beta is False and layer.lin_beta is None
        assert 'lin_beta.weight' not in layer.state_dict()
        assert TransformerConv(8, 4, heads=2, beta=True, concat=concat).beta is True
        assert TransformerConv(8, 4, heads=2, beta=False, concat=concat).beta is False
    # the skip projection exists either way (the reference builds it unconditionally)
    assert 'lin_skip.weight' in TransformerConv(8, 4, root_weight=False).state_dict()


def test_attention_weights_on_host_tensors():
    """Returned whenever the argument is a bool (True or False), and BEFORE dropout: in training
    with dropout every destination's coefficients still sum to one."""
    from pytorch_geometric_amd.nn import TransformerConv
    G = R.load_golden()
    torch.manual_seed(3)
    layer = TransformerConv(16, 6, heads=2, dropout=0.5)
    x, ei = G['x'], G['edge_index']
    assert isinstance(layer(x, ei), torch.Tensor)
    for flag in (True, False):
        out, (edges, alpha) = layer(x, ei, return_attention_weights=flag)
        assert torch.equal(edges, ei) and alpha.shape == (400, 2)
        sums = torch.zeros(48, 2).index_add(0, ei[1], alpha.detach())
        has = torch.bincount(ei[1], minlength=48) > 0
        assert_close(sums[has], torch.ones_like(sums[has]), what='row sums in training')
        assert int((alpha == 0).sum()) == 0


def test_entry_points_validate_without_gpu():
    """pygamd_transformer_* reject bad arguments with status 1 / 2 / 3 before any device work."""
    from pytorch_geometric_amd import _build, _lib, _native
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    dev = ctypes.c_void_p(16)   # (never dereferenced: every call below is rejected or launches nothing)
    nbytes = ctypes.c_size_t(0)
    for (H, C), want in {(4, 128): 1, (3, 5): 1, (1, 512): 1, (64, 8): 1, (8, 128): 0, (65, 1): 0,
                         (0, 4): 0}.items():
        assert lib.pygamd_transformer_supported(H, C) == want, (H, C)
        assert _native.transformer_supported(H, C) is bool(want)
    assert lib.pygamd_transformer_workspace_bytes(3, 4, 8, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= 4 * 3 * max(32 + 8, 2 * 32)     # forward partials, packed gradients
    assert lib.pygamd_transformer_workspace_bytes(0, 4, 8, ctypes.byref(nbytes)) == 0
    assert nbytes.value == 0                               # no long rows: no workspace
    assert lib.pygamd_transformer_workspace_bytes(3, 4, 8, None) == 1
    assert lib.pygamd_transformer_workspace_bytes(-1, 4, 8, ctypes.byref(nbytes)) == 1
    assert lib.pygamd_transformer_workspace_bytes(0, 8, 128, ctypes.byref(nbytes)) == 2

    def fwd(rowptr=dev, idx=1, query=dev, key=dev, value=dev, ld=32, n_rows=5, H=4, C=8,
            hub_rows=None, n_hub=0, n_chunks=0, alpha=dev, out=dev, ws=None, ws_bytes=0):
        g = csr_arg(rowptr=rowptr, col=dev, idx_dtype=idx, n_rows=n_rows, hub_rows=hub_rows,
                    hub_chunk_ptr=hub_rows, n_hub=n_hub, n_chunks=n_chunks, hub_threshold=1024,
                    hub_chunk=256)
        return lib.pygamd_transformer_forward(g, query, key, value, ld, 9, H, C, 0.35, alpha, out,
                                              ws, ws_bytes, None)

    assert lib.pygamd_transformer_forward(None, dev, dev, dev, 32, 9, 4, 8, 0.35, dev, dev, None,
                                          0, None) == 1          # no descriptor
    assert fwd(rowptr=None) == 1 and fwd(query=None) == 1 and fwd(key=None) == 1
    assert fwd(alpha=None) == 1 and fwd(value=None) == 1    # aggregation asked for, no values
    assert fwd(ld=31) == 1                                  # rows narrower than H * C
    assert fwd(idx=5) == 1 and fwd(n_rows=-1) == 1 and fwd(H=0) == 1 and fwd(C=0) == 1
    assert fwd(H=8, C=128, ld=1024) == 2 and fwd(H=65, C=1, ld=65) == 2
    assert fwd(n_hub=2, n_chunks=8) == 1                        # a plan without its arrays
    assert fwd(n_hub=0, n_chunks=3) == 1
    assert fwd(hub_rows=dev, n_hub=2, n_chunks=1) == 1          # fewer chunks than hub rows
    assert fwd(hub_rows=dev, n_hub=2, n_chunks=8) == 3          # no workspace for the partials
    assert fwd(hub_rows=dev, n_hub=2, n_chunks=8, ws=dev, ws_bytes=64) == 3
    assert fwd(n_rows=0) == 0                                   # no rows: nothing to launch

    def bwd_dst(key=dev, value=dev, ld=32, grad_out=dev, out=dev, grad_alpha=None, H=4, C=8,
                n_rows=5, grad_s=dev, grad_query=dev, hub_rows=None, n_hub=0, n_chunks=0,
                ws=None, ws_bytes=0):
        g = csr_arg(rowptr=dev, col=dev, idx_dtype=1, n_rows=n_rows, hub_rows=hub_rows,
                    hub_chunk_ptr=hub_rows, n_hub=n_hub, n_chunks=n_chunks, hub_threshold=1024,
                    hub_chunk=256)
        return lib.pygamd_transformer_backward_dst(
            g, key, value, ld, dev, grad_out, out, grad_alpha, 9, H, C, 0.35, grad_s, grad_query,
            ws, ws_bytes, None)

    assert lib.pygamd_transformer_backward_dst(None, dev, dev, 32, dev, dev, dev, None, 9, 4, 8,
                                               0.35, dev, dev, None, 0, None) == 1
    assert bwd_dst(grad_out=None) == 1 and bwd_dst(out=None) == 1
    assert bwd_dst(grad_alpha=dev) == 1                         # both sources of d alpha given
    assert bwd_dst(grad_out=None, out=None, grad_alpha=None) == 1
    assert bwd_dst(key=None) == 1 and bwd_dst(value=None) == 1
    assert bwd_dst(grad_s=None) == 1 and bwd_dst(grad_query=None) == 1 and bwd_dst(ld=8) == 1
    assert bwd_dst(H=8, C=128, ld=1024) == 2 and bwd_dst(n_rows=-2) == 1
    assert bwd_dst(hub_rows=dev, n_hub=1, n_chunks=5) == 3
    assert bwd_dst(hub_rows=dev, n_hub=1, n_chunks=5, ws=dev, ws_bytes=16) == 3
    assert bwd_dst(n_rows=0) == 0

    def bwd_src(slot_map=dev, idx=0, n_src=5, H=4, C=8, grad_out=dev, grad_key=dev,
                grad_value=dev, ld=64, hub_rows=None, n_hub=0, n_chunks=0):
        g = csr_arg(rowptr=dev, col=dev, idx_dtype=idx, n_rows=n_src, hub_rows=hub_rows,
                    hub_chunk_ptr=hub_rows, n_hub=n_hub, n_chunks=n_chunks, hub_threshold=1024,
                    hub_chunk=256)
        return lib.pygamd_transformer_backward_src(
            g, slot_map, dev, dev, dev, grad_out, 7, H, C, 0.35, grad_key, grad_value, ld, None, 0,
            None)

    assert lib.pygamd_transformer_backward_src(None, dev, dev, dev, dev, dev, 7, 4, 8, 0.35, dev,
                                               dev, 64, None, 0, None) == 1
    assert bwd_src(slot_map=None) == 1 and bwd_src(grad_key=None) == 1 and bwd_src(idx=2) == 1
    assert bwd_src(grad_value=None) == 1                        # grad_out given: both gradients
    assert bwd_src(ld=16) == 1
    assert bwd_src(H=2, C=300, ld=600) == 2 and bwd_src(n_src=-1) == 1
    assert bwd_src(n_hub=1, n_chunks=4) == 1
    assert bwd_src(hub_rows=dev, n_hub=1, n_chunks=4) == 3
    assert bwd_src(n_src=0) == 0
