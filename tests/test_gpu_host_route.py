"""The generic device route of the layers with a ``propagate`` fallback (``fuse = False``) against
the same layer's host route, which runs the same ``edge_update`` / ``message`` over
``nn/_host.py``; and no ``forward`` writing ``self.fuse`` on the way."""
import copy

import pytest
import torch

import _host_route_cases as C
from _util import assert_close, assert_close_scaled, gen

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64], ids=['int32', 'int64'])
@pytest.mark.parametrize('name', C.NAMES)
def test_generic_device_route_matches_the_host_route(dev, name, dtype):
    host, inputs = C.make(name)
    layer = copy.deepcopy(host).to(dev)
    layer.fuse = False
    writes = C.recording(layer)
    results = []
    for mod, device in ((host, 'cpu'), (layer, dev)):
        leaves = {k: v.clone().to(device).requires_grad_(True) for k, v in inputs.items()}
        outs = C.run(name, mod, leaves, dtype, device)
        grad_outs = [torch.randn(o.shape, generator=gen(41 + i)).to(device)
                     for i, o in enumerate(outs)]
        params = dict(mod.named_parameters())
        grads = torch.autograd.grad(outs, list(leaves.values()) + list(params.values()),
                                    grad_outs, allow_unused=True)
        results.append((outs, dict(zip(list(leaves) + list(params), grads))))
    assert writes == [] and layer.fuse is False
    (ref_outs, ref_grads), (outs, grads) = results
    for i, (o, r) in enumerate(zip(outs, ref_outs)):
        assert_close(o, r, what=f'{name} out[{i}]')
    for key, r in ref_grads.items():
        if r is not None or grads[key] is not None:   # (an unused parameter: None or zeros)
            zero = torch.zeros_like(r if r is not None else grads[key])
            assert_close_scaled(zero if grads[key] is None else grads[key],
                                zero if r is None else r, what=f'{name} grad {key}')
