"""SplineConv without a device: the float64 restatement (tests/_spline_ref.py) against hand values,
the partition of unity, the layer's construction and the generic route on host tensors."""
import pytest
import torch

import _spline_ref as R
from _util import gen, random_graph


def test_restatement_against_hand_values():
    """dim 1, kernel_size 5, degree 1, open: span 4, so pseudo 0, 0.25, 0.3, 1 sit at v = 0, 1,
    1.2, 4: bins (0, 1), (1, 2), (1, 2) and (4, 0), the last one wrapped with weight 0"""
    from pytorch_geometric_amd.utils import spline_basis
    pseudo = torch.tensor([[0.0], [0.25], [0.3], [1.0]])
    want_b = torch.tensor([[1.0, 0.0], [1.0, 0.0], [0.8, 0.2], [1.0, 0.0]], dtype=torch.float64)
    want_w = torch.tensor([[0, 1], [1, 2], [1, 2], [4, 0]])
    b, wi = R.basis(pseudo, [5], [True], 1)
    assert torch.equal(wi, want_w)
    torch.testing.assert_close(b, want_b, atol=1e-7, rtol=0)
    b, wi = spline_basis(pseudo, torch.tensor([5]), torch.tensor([1], dtype=torch.uint8), 1)
    assert torch.equal(wi, want_w)
    torch.testing.assert_close(b.double(), want_b, atol=1e-6, rtol=0)


@pytest.mark.parametrize('degree', [1, 2, 3])
def test_basis_sums_to_one(degree):
    from pytorch_geometric_amd.utils import spline_basis
    pseudo = torch.rand(200, 3, generator=gen(degree))
    ks, op = [3, 4, 5], [True, False, True]
    b, wi = R.basis(pseudo, ks, op, degree)
    torch.testing.assert_close(b.sum(1), torch.ones(200, dtype=torch.float64))
    assert int(wi.min()) >= 0 and int(wi.max()) < 60
    b2, wi2 = spline_basis(pseudo, torch.tensor(ks), torch.tensor(op, dtype=torch.uint8), degree)
    assert torch.equal(wi2, wi)
    torch.testing.assert_close(b2.double(), b, atol=1e-6, rtol=0)


def test_construction_repr_state_dict_and_lazy_channels():
    from pytorch_geometric_amd.nn import SplineConv
    conv = SplineConv(8, 16, dim=2, kernel_size=5, degree=2, is_open_spline=[True, False])
    assert repr(conv) == 'SplineConv(8, 16, dim=2)' and conv.K == 25 and conv.aggr == 'mean'
    assert list(conv.state_dict()) == ['weight', 'bias', 'kernel_size', 'is_open_spline',
                                       'lin.weight']
    assert conv.weight.shape == (25, 8, 16) and conv.lin.weight.shape == (16, 8)
    assert conv.kernel_size.tolist() == [5, 5] and conv.kernel_size.dtype == torch.long
    assert conv.is_open_spline.tolist() == [1, 0] and conv.is_open_spline.dtype == torch.uint8
    assert float(conv.weight.detach().abs().max()) <= 1 / (25 * 8) ** 0.5
    assert float(conv.bias.detach().abs().max()) == 0
    bare = SplineConv((8, 4), 16, dim=1, kernel_size=3, root_weight=False, bias=False)
    assert list(bare.state_dict()) == ['weight', 'kernel_size', 'is_open_spline']
    lazy = SplineConv(-1, 6, dim=2, kernel_size=[3, 4])
    assert isinstance(lazy.weight, torch.nn.parameter.UninitializedParameter)
    ei = random_graph(10, 10, 30, 1)
    out = lazy(torch.randn(10, 7, generator=gen(2)), ei, torch.rand(30, 2, generator=gen(3)))
    assert out.shape == (10, 6) and lazy.weight.shape == (12, 7, 6)
    assert lazy.lin.weight.shape == (6, 7) and not hasattr(lazy, '_hook')
    conv2 = SplineConv(7, 6, dim=2, kernel_size=[3, 4])
    conv2.load_state_dict(lazy.state_dict())


@pytest.mark.parametrize('degree,aggr', [(1, 'mean'), (2, 'add'), (3, 'max')])
def test_generic_route_on_host_tensors(degree, aggr):
    """bipartite, a destination without edges, pseudo with exact 0 and 1; output and every
    gradient against the float64 restatement at float32 rounding of sums of <= 40 terms"""
    from pytorch_geometric_amd.nn import SplineConv
    ks, op = [3, 4], [True, False]
    ei = random_graph(17, 11, 90, 5)
    ei = ei[:, ei[1] != 4]
    g = gen(6 + degree)
    pseudo = torch.rand(ei.size(1), 2, generator=g)
    pseudo[0, 0], pseudo[1, 1], pseudo[2] = 0.0, 1.0, torch.tensor([1.0, 0.0])
    xs, xd = torch.randn(17, 5, generator=g), torch.randn(11, 3, generator=g)
    torch.manual_seed(degree)
    conv = SplineConv((5, 3), 7, dim=2, kernel_size=ks, is_open_spline=op, degree=degree, aggr=aggr)
    conv.bias.data.normal_()
    leaves = [xs.requires_grad_(True), xd.requires_grad_(True), pseudo.requires_grad_(True)]
    params = [conv.weight, conv.lin.weight, conv.bias]
    out = conv((xs, xd), ei, pseudo)
    go = torch.randn(11, 7, generator=g)
    got = torch.autograd.grad(out, leaves + params, go)
    l64 = [t.detach().double().requires_grad_(True) for t in leaves]
    p64 = [t.detach().double().requires_grad_(True) for t in params]
    want = R.layer(p64[0], p64[1], p64[2], l64[0], l64[1], l64[2], ei, 11, ks, op, degree, aggr)
    assert out.shape == (11, 7)
    torch.testing.assert_close(out.double(), want.detach(), atol=2e-5, rtol=2e-5)
    for a, b in zip(got, torch.autograd.grad(want, l64 + p64, go.double())):
        torch.testing.assert_close(a.double(), b, atol=5e-5, rtol=5e-5)


def test_envelope_and_workspace_size():
    """the envelope as the header states it, and the workspace of 2^31 chunks past 32 bits"""
    import ctypes
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd import _build, _native
    assert 'spline.hip' in _build.SOURCES
    for args, ok in (((512, 512, 32, 64), True), ((513, 64, 25, 4), False), ((64, 513, 1, 4), False),
                     ((32, 64, 256, 8), True), ((32, 64, 257, 8), False), ((32, 64, 25, 65), False)):
        assert _native.spline_supported(*args) is ok, args
    size = ctypes.c_size_t(0)
    assert pga.load_library().pygamd_spline_workspace_size(2 ** 31, 64, 25, ctypes.byref(size)) == 0
    assert size.value == 4 * 2 ** 31 * 64 * 25
