"""nn.GINConv / nn.GINEConv on host tensors: every recorded reference case
(tests/golden/golden_gin_v1.pt), the state-dict keys, the two ValueErrors, ``__repr__`` and
``reset_parameters``.  No GPU needed."""
import pytest
import torch

import _gin_ref as R


@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_host_tensors(name):
    R.check_class_case(R.load_golden(), name, 'cpu')


def test_state_dict_keys():
    from pytorch_geometric_amd.nn import GINConv, GINEConv
    nn_keys = ['nn.0.weight', 'nn.0.bias', 'nn.2.weight', 'nn.2.bias']
    for cls in (GINConv, GINEConv):
        for train_eps in (False, True):
            layer = cls(R.make_nn(), eps=0.5, train_eps=train_eps)
            assert list(layer.state_dict()) == ['eps'] + nn_keys
            assert ('eps' in dict(layer.named_parameters())) is train_eps
            assert ('eps' in dict(layer.named_buffers())) is (not train_eps)
            assert float(layer.eps.detach()) == 0.5 and layer.eps.shape == (1, )
    layer = GINEConv(R.make_nn(), train_eps=True, edge_dim=3)
    assert list(layer.state_dict()) == ['eps'] + nn_keys + ['lin.weight', 'lin.bias']
    assert layer.lin.weight.shape == (16, 3) and layer.lin.bias.shape == (16, )
    assert GINEConv(R.make_nn()).lin is None

    class Block(torch.nn.Module):       # `in_channels` instead of `in_features`
        def __init__(self):
            super().__init__()
            self.in_channels = 10
            self.inner = torch.nn.Linear(10, 4)

        def forward(self, x):
            return self.inner(x)

    assert GINEConv(Block(), edge_dim=5).lin.weight.shape == (10, 5)


def test_value_errors():
    from pytorch_geometric_amd.nn import GINEConv
    with pytest.raises(ValueError, match='Could not infer input channels'):
        GINEConv(torch.nn.ReLU(), edge_dim=3)
    with pytest.raises(ValueError, match='Could not infer input channels'):
        GINEConv(torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Linear(4, 4)), edge_dim=3)
    layer = GINEConv(R.make_nn())
    x = torch.randn(10, 16)
    ei = torch.randint(0, 10, (2, 30))
    with pytest.raises(ValueError, match='dimensionalities do not match'):
        layer(x, ei, edge_attr=torch.randn(30, 5))
    assert layer(x, ei, edge_attr=torch.randn(30, 16)).shape == (10, 8)


def test_repr():
    from pytorch_geometric_amd.nn import GINConv, GINEConv
    nn = R.make_nn()
    assert repr(GINConv(nn)) == f'GINConv(nn={nn})'
    assert repr(GINEConv(nn, edge_dim=3)) == f'GINEConv(nn={nn})'


def test_reset_parameters_restores_eps_and_resets_nn():
    from pytorch_geometric_amd.nn import GINConv, GINEConv
    for layer in (GINConv(R.make_nn(), eps=0.3, train_eps=True),
                  GINEConv(R.make_nn(), eps=0.3, train_eps=True, edge_dim=3)):
        before = layer.nn[0].weight.detach().clone()
        layer.eps.data.fill_(7.0)
        layer.reset_parameters()
        assert float(layer.eps.detach()) == pytest.approx(0.3)
        assert not torch.equal(layer.nn[0].weight, before)      # nn was re-initialised


def test_entry_points_reject_a_missing_descriptor():
    """pygamd_gine_* take the CSR handle and its hub plan as one ``pygamd_csr``: without it the
    call is status 1 before any device work, and with it the first bad field still decides."""
    import ctypes
    from _util import csr_arg
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    dev = ctypes.c_void_p(16)   # (never dereferenced: every call below is rejected or launches nothing)

    def fwd(g, F=8, De=0):
        return lib.pygamd_gine_forward(g, None, dev, 8, None, 0, None, dev, None, None, 9, F, De,
                                       dev, None, 0, None)

    def bwd(g, F=8, De=0):
        return lib.pygamd_gine_backward(g, None, dev, 8, dev, None, None, dev, 7, F, De, dev, dev,
                                        None, None, None, 0, None)

    assert fwd(None) == 1 and bwd(None) == 1
    empty = dict(rowptr=dev, col=dev, idx_dtype=1, n_rows=0, hub_threshold=1024, hub_chunk=256)
    assert fwd(csr_arg(**empty)) == 0 and bwd(csr_arg(**empty)) == 0      # no rows: nothing to launch
    assert fwd(csr_arg(**dict(empty, idx_dtype=5))) == 1
    assert bwd(csr_arg(**dict(empty, n_hub=0, n_chunks=3))) == 1         # chunks without hub rows
    assert fwd(csr_arg(**empty), F=513) == 2 and bwd(csr_arg(**empty), F=64, De=33) == 2
