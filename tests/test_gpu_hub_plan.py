"""A cached hub plan is launched at the threshold and chunk it was made for, whatever the module
says at launch time.  On the degree-profile graph ``_degree_cases.build(0, 64, 48)`` (about 3 k
nodes, 30 k edges, at least 8 hub rows by destination and by source at (64, 48):
tests/test_degree_cases_host.py) every handle is built with the module at (64, 48); each operator
then runs once there and once with the module at (9, 5) on the SAME handle.  A launch that paired
the cached plan with the module's pair would cover ``5 * n_chunks`` slots of a hub row and leave
the rows between 10 and 64 slots unwritten: the two runs must agree bit for bit, and every launch
record must carry the counts of the (64, 48) plans.  The control builds a fresh handle under
(9, 5): it does pick the new pair up, has another plan and is right on its own."""
import pytest
import torch

import _degree_cases as D
from _util import gen

pytestmark = pytest.mark.gpu

OWN, OTHER = (64, 48), (9, 5)
DTYPES = [torch.int32, torch.int64]


def _module_at(monkeypatch, pair):
    from pytorch_geometric_amd import _native
    monkeypatch.setattr(_native, 'HUB_THRESHOLD', pair[0])
    monkeypatch.setattr(_native, 'HUB_CHUNK', pair[1])


def _handle(dev, index_dtype):
    """the profile graph's handle with both sorted forms and their plans, at the module's pair"""
    import pytorch_geometric_amd as pga
    ei, n, _ = D.build(0, *OWN)
    return pga.EdgeIndex(ei.to(dev).to(index_dtype), (n, n)).fill_cache_()


def _graph_plans(h):
    return [h.by_dst().hub, h.by_src().hub]


# ---- the calls: name -> builder(dev, index_dtype) -> (run() -> tensors, plans() -> HubPlans) ----------
def _spmm_calls(dev, index_dtype, reduces, call):
    h = _handle(dev, index_dtype)
    n = h.num_dst_nodes
    g = gen(700)
    x0, go = torch.randn(n, 24, generator=g).to(dev), torch.randn(n, 24, generator=g).to(dev)

    def run():
        res = []
        for red in reduces:
            x = x0.clone().requires_grad_(True)
            out = call(h, x, red)
            res += [out.detach(), torch.autograd.grad(out, [x], go)[0]]
        return res

    return run, lambda: _graph_plans(h)


def _spmm(dev, index_dtype):
    """utils.spmm (the Python node) sum / mean / max, forward and backward"""
    import pytorch_geometric_amd as pga
    return _spmm_calls(dev, index_dtype, ('sum', 'mean', 'max'), pga.utils.spmm)


def _spmm_node(dev, index_dtype):
    """sum / mean on the route of the conv layers with ``x.requires_grad``: the C++ node where the
    binding is loaded, which takes both plans and ONE pair.  It leaves no launch records (and an
    installed sink keeps the Python node), so this case runs without one."""
    from pytorch_geometric_amd import _compiled
    from pytorch_geometric_amd._functions import spmm_node

    def call(h, x, red):
        out = spmm_node(x, None, h, red, 'coo')
        if _compiled.ops() is not None:       # (both plans at one pair: not the Python node)
            assert 'SpmmFunction' not in type(out.grad_fn).__name__, type(out.grad_fn)
        return out

    return _spmm_calls(dev, index_dtype, ('sum', 'mean'), call)


def _sage_layer(dev, index_dtype):
    """the one-kernel layer at F = Fo = 32 with ``save_agg``: on the compiled route where it is
    loaded (it takes a strided ``agg`` view as well) and, with the binding set aside as in
    tests/test_gpu_binding.py, on the ctypes route into the left half of a wider buffer"""
    from pytorch_geometric_amd import _compiled, _native
    h = _handle(dev, index_dtype)
    fwd, n, F = h.by_dst(), h.num_dst_nodes, 32
    assert _native.sage_layer_forward_supported(F, F, 'mean')
    g = gen(701)
    x = torch.randn(n, F, generator=g).to(dev)
    w = (torch.randn(F, 2 * F, generator=g) * 0.1).to(dev)
    b = torch.randn(F, generator=g).to(dev)

    def layer(strided):
        agg = torch.zeros(n, 2 * F, device=dev)[:, :F] if strided else torch.zeros(n, F, device=dev)
        out = torch.zeros(n, F, device=dev)
        _native.sage_layer_forward(fwd.ptr, fwd.idx, x, x, w, b, 'mean', True, agg, out,
                                   hub=fwd.hub, save_agg=True)
        return [agg.contiguous(), out]

    def run():
        ns = _compiled.ops()
        res = layer(False) + layer(True) if ns is not None else []
        _compiled._state['ns'] = None
        try:
            res += layer(True)
        finally:
            _compiled._state['ns'] = ns
        return res

    return run, lambda: _graph_plans(h)


def _gatv2(dev, index_dtype):
    """H = 2, C = 8: the softmax merge of hub chunks"""
    import test_gpu_gatv2 as M
    h = _handle(dev, index_dtype)
    n = h.num_dst_nodes
    P = M._problem(n, n, D.build(0, *OWN)[0], 2, 8, 702)
    P['graph'] = h

    def run():
        got, graph = M._device_run(P, dev, index_dtype)
        assert graph is h
        return got

    return run, lambda: _graph_plans(h)


def _gine(dev, index_dtype):
    """F = 12, De = 3: the sum merge and the parameter partials"""
    import test_gpu_gine as M
    h = _handle(dev, index_dtype)
    n = h.num_dst_nodes
    P = M._dyadic(n, n, D.build(0, *OWN)[0], 12, 3, 703)
    P['graph'] = h

    def run():
        got, graph = M._device_run(P, dev, index_dtype)
        assert graph is h
        return got

    return run, lambda: _graph_plans(h)


def _film(dev, index_dtype):
    """F = 8, R = 2: the plans of the two pair forms.  Relation 0 holds 85 % of the edges, so its
    (relation, node) pair rows of the longest profile rows stay above 64 slots."""
    import test_gpu_film as M
    ei, n, _ = D.build(0, *OWN)
    et = (torch.rand(ei.size(1), generator=gen(704)) > 0.85).long()
    P = M._problem(n, n, ei, et, 8, 2, 705)

    def run():  # (the forms are built by the first run and kept in P)
        return M._device_run(P, dev, index_dtype)

    def plans():
        forms = P[('forms', index_dtype, False)]
        return [forms.fwd.hub, forms.pairs[0].hub, forms.pairs[1].hub]

    return run, plans


CALLS = {'spmm': _spmm, 'spmm_node': _spmm_node, 'sage_layer': _sage_layer, 'gatv2': _gatv2,
         'gine': _gine, 'film': _film}


def _recorded(monkeypatch, run, record):
    """(what ``run`` returned, the (n_hub, n_chunks | None) of every launch record that has one)"""
    from pytorch_geometric_amd import _native
    sink = [] if record else None
    monkeypatch.setattr(_native, 'timing_sink', sink)
    got = run()
    torch.cuda.synchronize()
    monkeypatch.setattr(_native, 'timing_sink', None)
    return got, [(i['n_hub'], i.get('n_chunks')) for i, _, _ in sink or [] if 'n_hub' in i]


@pytest.mark.parametrize('index_dtype', DTYPES, ids=['int32', 'int64'])
@pytest.mark.parametrize('name', list(CALLS))
def test_cached_plan_runs_at_its_own_settings(dev, monkeypatch, name, index_dtype):
    _module_at(monkeypatch, OWN)
    run, plans = CALLS[name](dev, index_dtype)
    record = name != 'spmm_node'
    first, rec_first = _recorded(monkeypatch, run, record)
    made = plans()
    for plan in made:
        assert (plan.threshold, plan.chunk) == OWN and plan.n_hub >= 8, (name, plan[2:])
    _module_at(monkeypatch, OTHER)
    second, rec_second = _recorded(monkeypatch, run, record)
    assert all(a is b for a, b in zip(plans(), made)), f'{name}: a plan was made again'
    assert len(first) == len(second) and any(t is not None for t in first)
    for k, (a, b) in enumerate(zip(first, second)):
        assert (a is None) == (b is None), (name, k)
        if a is not None:
            assert torch.equal(a, b), \
                f'{name}: result {k} changed with the module at {OTHER} (handle made at {OWN})'
    n_hubs = {p.n_hub for p in made}
    pairs = {(p.n_hub, p.n_chunks) for p in made}
    assert rec_first or not record, f'{name}: no launch record carries a hub count'
    for what, recs in (('first', rec_first), ('second', rec_second)):
        for n_hub, n_chunks in recs:
            assert n_hub in n_hubs, (name, what, n_hub, n_hubs)
            assert n_chunks is None or (n_hub, n_chunks) in pairs, (name, what, n_hub, n_chunks)
    assert rec_second == rec_first


# ---- the control ---------------------------------------------------------------------------------------
_REF = {}


def _sum_reference():
    """x and the float64 and float32 restatements of the sum aggregation, computed once"""
    if not _REF:
        ei, n, _ = D.build(0, *OWN)
        x = torch.randn(n, 24, generator=gen(706))
        _REF['x'] = x
        for dt in (torch.float64, torch.float32):
            _REF[dt] = torch.zeros(n, 24, dtype=dt).index_add_(0, ei[1], x.to(dt)[ei[0]])
        _REF['in_deg'] = D.degrees(ei, n)[0]
    return _REF


@pytest.mark.parametrize('index_dtype', DTYPES, ids=['int32', 'int64'])
def test_fresh_handle_picks_the_module_pair_up(dev, monkeypatch, index_dtype):
    """... so the test above does not pass because nothing reads the module any more"""
    import pytorch_geometric_amd as pga
    _module_at(monkeypatch, OWN)
    cached = _handle(dev, index_dtype)
    _module_at(monkeypatch, OTHER)
    fresh = _handle(dev, index_dtype)
    ref = _sum_reference()
    n = ref['x'].size(0)
    for h, pair in ((fresh, OTHER), (cached, OWN)):
        for csr, deg in zip((h.by_dst(), h.by_src()), D.degrees(D.build(0, *OWN)[0], n)):
            want = D.expected_plan(deg, *pair)
            assert (csr.hub.threshold, csr.hub.chunk) == pair
            assert (csr.hub.n_hub, csr.hub.n_chunks) == (want['n_hub'], want['n_chunks'])
    assert fresh.by_dst().hub.n_hub != cached.by_dst().hub.n_hub
    assert fresh.by_src().hub.n_hub != cached.by_src().hub.n_hub
    for h, what in ((fresh, f'fresh handle at {OTHER}'), (cached, f'cached handle at {OWN}')):
        out = pga.utils.spmm(h, ref['x'].to(dev), 'sum')
        D.assert_rows_close(out, ref[torch.float64], torch.arange(n), ref['in_deg'], tol=D.TOL,
                            ref32=ref[torch.float32], what=f'spmm sum, {what}')
