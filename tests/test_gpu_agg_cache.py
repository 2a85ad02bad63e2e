"""The first-layer aggregation cache of the fused GraphSAGE stack (nn/models/_fused_sage.py) on the
device: from the second step on the first layer reads its aggregated rows back (`save_agg =
AGG_GIVEN`) instead of gathering them, and NOTHING a caller can see changes — every comparison with
the uncached run (`PYGAMD_CACHE_AGG0=0`) is `torch.equal`."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

F_IN = 100


@pytest.fixture
def data(dev):
    from pytorch_geometric_amd.datasets import products_like
    x, y, ei, c = products_like(seed=5, scale=1 / 1024)
    return x.to(dev), y.to(dev), ei.to(dev), c


@pytest.fixture
def cache_env(monkeypatch):
    import pytorch_geometric_amd as pga
    pga.clear_aggregation_cache()
    monkeypatch.delenv('PYGAMD_CACHE_AGG0', raising=False)

    def switch(on: bool):
        monkeypatch.setenv('PYGAMD_CACHE_AGG0', '1' if on else '0')
        pga.clear_aggregation_cache()

    yield switch
    pga.clear_aggregation_cache()


@pytest.fixture
def sink():
    from pytorch_geometric_amd import _native
    log = []
    _native.timing_sink = log
    yield log
    _native.timing_sink = None


def _model(dev, c, aggr='mean'):
    from pytorch_geometric_amd.nn import GraphSAGE
    torch.manual_seed(0)
    return GraphSAGE(F_IN, 256, num_layers=3, out_channels=c, aggr=aggr).to(dev)


def _layer0(log):
    """timing_sink records of the first layer's forward launch (the only one at width 100)"""
    return [info for info, _, _ in log
            if info.get('fused_gemm') and info['F'] == F_IN and not info['fused_gemm']['backward']]


def _train(dev, data, steps, before_step=None):
    """`steps` optimizer steps of a fresh model; per step (loss, out, grads, params)."""
    x, y, ei, c = data
    model = _model(dev, c)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    rec = []
    for it in range(steps):
        if before_step is not None:
            x, ei = before_step(it, x, ei)
        opt.zero_grad(set_to_none=True)
        out = model(x, ei)
        loss = torch.nn.functional.cross_entropy(out, y)
        loss.backward()
        opt.step()
        rec.append([loss.detach().clone(), out.detach().clone()]
                   + [p.grad.clone() for p in model.parameters()]
                   + [p.detach().clone() for p in model.parameters()])
    torch.cuda.synchronize()
    return rec


def _same(a, b):
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        for i, (ta, tb) in enumerate(zip(ra, rb)):
            assert torch.equal(ta, tb), f'step {step}, tensor {i}: cached and uncached runs differ'


def test_three_steps_equal_the_uncached_run_and_skip_the_gather(dev, data, cache_env, sink):
    cache_env(True)
    cached = _train(dev, data, 3)
    launches = _layer0(sink)
    assert len(launches) == 3
    assert launches[0]['nnz'] > 0                              # step 1 gathers and stores
    for info in launches[1:]:                                   # steps 2, 3: rows given
        assert info['nnz'] == 0 and info['n_hub'] == 0
        assert info['fused_gemm']['save_agg'] is True           # (the read of the stored rows)
    # the hidden layers always gather
    hidden = [info for info, _, _ in sink if info.get('fused_gemm') and info['F'] != F_IN]
    assert hidden and all(info['nnz'] > 0 for info in hidden)
    del sink[:]
    cache_env(False)
    plain = _train(dev, data, 3)
    assert all(info['nnz'] > 0 for info in _layer0(sink)) and len(_layer0(sink)) == 3
    _same(cached, plain)


@pytest.mark.parametrize('case', ['inplace', 'new_tensor', 'other_graph'])
def test_invalidation_equals_the_uncached_run(dev, data, cache_env, sink, case):
    x0, _, ei0, _ = data
    ei_other = ei0[:, : ei0.size(1) // 2].contiguous()

    def change(it, x, ei):
        if it != 2:
            return x, ei
        if case == 'inplace':
            return x.add_(1), ei
        if case == 'new_tensor':
            return x * 0.5, ei
        return x, ei_other

    runs = []
    for on in (True, False):
        cache_env(on)
        del sink[:]
        fresh = (x0.clone(), data[1], ei0, data[3])
        runs.append(_train(dev, fresh, 4, change))
        if on:
            modes = [info['nnz'] > 0 for info in _layer0(sink)]
            assert modes == [True, False, True, False]          # gathers again exactly once
    _same(*runs)


def test_an_input_that_takes_a_gradient_bypasses_the_cache(dev, data, cache_env, sink):
    x, y, ei, c = data
    res = []
    for on in (True, False):
        cache_env(on)
        model = _model(dev, c)
        with torch.no_grad():   # (a whole model: stores an entry for x when the cache is on)
            model(x, ei)
        del sink[:]
        xg = x.requires_grad_()
        out = model(xg, ei)
        torch.nn.functional.cross_entropy(out, y).backward()
        assert all(info['nnz'] > 0 for info in _layer0(sink))
        res.append([out.detach().clone(), xg.grad.clone()]
                   + [p.grad.clone() for p in model.parameters()])
        xg.grad = None
        x.requires_grad_(False)
    _same([res[0]], [res[1]])
    assert res[0][1].abs().max().item() > 0


def test_the_reduction_is_part_of_the_key(dev, data, cache_env, sink):
    x, y, ei, c = data
    outs = {}
    for on in (True, False):
        cache_env(on)
        del sink[:]
        for aggr in ('mean', 'sum', 'sum'):
            model = _model(dev, c, aggr)
            with torch.no_grad():
                outs.setdefault((on, aggr), []).append(model(x, ei).clone())
        if on:
            assert [info['nnz'] > 0 for info in _layer0(sink)] == [True, True, False]
    for aggr in ('mean', 'sum'):
        for a, b in zip(outs[(True, aggr)], outs[(False, aggr)]):
            assert torch.equal(a, b)
    assert not torch.equal(outs[(True, 'mean')][0], outs[(True, 'sum')][0])


def test_entry_dies_with_the_input(dev, data, cache_env):
    import pytorch_geometric_amd as pga
    _, y, ei, c = data
    cache_env(True)
    model = _model(dev, c)
    x = data[0].clone()
    n = x.size(0)
    out = model(x, ei)
    torch.nn.functional.cross_entropy(out, y).backward()
    del out
    handle = pga.as_edge_index(ei, n, n).by_dst()
    assert handle._agg0 is not None and handle._agg0[2].shape == (n, F_IN)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    del x
    gc.collect()
    assert handle._agg0 is None
    freed = before - torch.cuda.memory_allocated()
    assert freed >= 2 * n * F_IN * 4, f'input and cached rows not released ({freed} bytes freed)'


def test_layer_by_layer_model_under_no_grad_retains_no_hidden_entry(dev, data, cache_env, sink):
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd.nn import SAGEConv
    x, y, ei, c = data
    n = x.size(0)
    cache_env(True)
    torch.manual_seed(0)
    conv1, conv2 = SAGEConv(F_IN, 128).to(dev), SAGEConv(128, 128).to(dev)

    def net(x):
        return conv2(conv1(x, ei).relu(), ei)

    handle = pga.as_edge_index(ei, n, n).by_dst()
    with torch.no_grad():
        ref = net(x)
        assert handle._agg0 is None                 # a single layer under no_grad never stores
    net(x).sum().backward()                         # a recording call of the first layer does
    assert handle._agg0 is not None and handle._agg0[0]() is x
    torch.cuda.synchronize()
    del sink[:]
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        got = net(x)
    assert handle._agg0[0]() is x and handle._agg0[2].shape == (n, F_IN)
    fused = [info for info, _, _ in sink if info.get('fused_gemm')]
    assert [(info['F'], info['nnz'] > 0) for info in fused] == [(F_IN, False), (128, True)]
    assert torch.equal(got, ref)
    del got
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= before
