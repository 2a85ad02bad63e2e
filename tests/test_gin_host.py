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
