"""Every row-walking kernel on the degree-profile graph of tests/_degree_cases.py: in- and
out-degrees 0 .. 513 around both slots-in-flight values, the wave width and every lane stride, the
hub threshold on both sides, chunk counts that divide exactly and a last chunk of one slot, hubs
as the first and the last row, adjacent hubs and a hub next to an empty row — by destination for
the forward and by source for the backward — judged PER ROW against the float64 restatements
(``assert_rows_close``: 2e-5 of the row's own scale, the project's figure for these kernels), at
the package's threshold and chunk and at (64, 48) and (9, 5), with both index dtypes.  Each run also
reads the launch records: the plan every kernel was given is the plan the degrees call for.
tests/test_degree_cases_host.py holds the CPU half: the layout, the conditioning and the float32
restatements' own error.  Worst figures per operator: profiles/degree_sweep.md (``-s`` prints
them)."""
import pytest
import torch

import _degree_cases as D
from _util import assert_close

pytestmark = pytest.mark.gpu

DTYPES = [torch.int32, torch.int64]
CASES = [(name, case) for name, op in D.OPERATORS.items() for case in op.cases]
SMALL = [(name, setting) for name, op in D.OPERATORS.items() if op.settings
         for setting in D.SETTINGS]


def _patch(monkeypatch, setting):
    """The package's threshold and chunk for the rest of the test; handles are built after this
    (their plans are cached) and the launches read the same two values."""
    from pytorch_geometric_amd import _native
    if setting is not None:
        monkeypatch.setattr(_native, 'HUB_THRESHOLD', setting[0])
        monkeypatch.setattr(_native, 'HUB_CHUNK', setting[1])
    return _native.HUB_THRESHOLD, _native.HUB_CHUNK


def _check_graph(graph, degs, P, thr, what, placed=True):
    """The handle's two sorted forms have the row lengths ``degs`` (by destination, by source) and,
    where the handle is the profile graph itself (``placed``), the profile where the case says."""
    pl = P['placement']
    for csr, deg, rows, lens, side in ((graph.by_dst(), degs[0], pl['dst_rows'], pl['dst_len'],
                                        'dst'),
                                       (graph.by_src(), degs[1], pl['src_rows'], pl['src_len'],
                                        'src')):
        ptr = csr.ptr.cpu().long()
        assert torch.equal(ptr[1:] - ptr[:-1], deg), f'{what}: {side} degrees'
        if placed:
            D.check_placement(ptr, rows, lens, thr, f'{what} {side}',
                              ordinary_background=thr >= 64)


def _direction(op, rec, i):
    if op.name == 'mixture':      # forward expand, then expand / coef_grad by destination, expand by source
        return 'src' if i == 3 else 'dst'
    return 'src' if rec['op'] in ('backward', 'backward_src') else 'dst'


def _check_records(op, sink, P, thr, chunk, what):
    """n_hub (and n_chunks where the record has it) of every launch of the operator's kind against
    the plan the degrees call for, in its direction"""
    by_dst, by_src = op.plan_degrees(P)
    plans = {'dst': D.expected_plan(by_dst, thr, chunk), 'src': D.expected_plan(by_src, thr, chunk)}
    recs = [i for i, _, _ in sink if i.get('kind') == op.kind]
    seen = set()
    for k, rec in enumerate(recs):
        if 'n_hub' not in rec:
            continue
        side = _direction(op, rec, k)
        seen.add(side)
        assert rec['n_hub'] == plans[side]['n_hub'], (what, rec['op'], side, rec['n_hub'])
        if 'n_chunks' in rec:
            assert rec['n_chunks'] == plans[side]['n_chunks'], (what, rec['op'], side,
                                                                rec['n_chunks'])
    assert seen == {'dst', 'src'}, (what, [r['op'] for r in recs])
    if op.name == 'mixture':
        assert [r['op'] for r in recs] == ['expand', 'expand', 'coef_grad', 'expand'], what
    assert plans['dst']['n_hub'] >= 8 and plans['src']['n_hub'] >= 8


def _run(op, case, dev, monkeypatch, index_dtype, setting):
    from pytorch_geometric_amd import _native
    thr, chunk = _patch(monkeypatch, setting)
    setting = (thr, chunk)
    what = f'{op.name} {case} at {setting} {str(index_dtype)[6:]}'
    P = D.problem(op, case, setting)
    sink = []
    monkeypatch.setattr(_native, 'timing_sink', sink)
    got, graph = op.device(P, case, dev, index_dtype)
    torch.cuda.synchronize()
    monkeypatch.setattr(_native, 'timing_sink', None)
    if op.name == 'han' and case[2] == 'relu':      # both sides under the device's ReLU mask
        mask = (got['out'] > 0).cpu()
        want = op.reference(P, case, torch.float64, mask=mask)
        ref32 = lambda: op.reference(P, case, torch.float32, mask=mask)   # noqa: E731
    else:
        want = D.reference(op, case, torch.float64, setting)
        ref32 = lambda: D.reference(op, case, torch.float32, setting)     # noqa: E731
    if op.kind is not None:
        _check_records(op, sink, P, thr, chunk, what)
    if hasattr(graph, 'by_dst'):           # (the typed SAGE handle is a stacked CSR of its own)
        assert graph.edge_index.dtype == index_dtype
        degs = op.plan_degrees(P)
        _check_graph(graph, degs, P, thr, what, placed=degs[0] is P['in_deg'])
    measure = {}
    try:
        D.judge(op, case, got, want, P, ref32=ref32, measure=measure)
    finally:
        outs = [v for k, v in measure.items() if not k.startswith('grad')] or [(0.0, 0)]
        grads = [v for k, v in measure.items() if k.startswith('grad')] or [(0.0, 0)]
        print(f'\ndegree-sweep | {op.name} | {case} | {setting} | {str(index_dtype)[6:]} | '
              f'{max(outs)[0]:.2e} | {max(outs)[1]} | {max(grads)[0]:.2e} | {max(grads)[1]}')
    if op.name == 'pna':            # an extremum is one of the u: p_dst + u is one rounding
        for s in ('min', 'max'):
            assert_close(got[s], want[s].float(), rtol=1e-6, atol=1e-6, what=f'{what} {s}')


@pytest.mark.parametrize('index_dtype', DTYPES, ids=['int32', 'int64'])
@pytest.mark.parametrize('name,case', CASES, ids=[f'{n}-{c}' for n, c in CASES])
def test_rows_of_every_length(dev, monkeypatch, name, case, index_dtype):
    _run(D.OPERATORS[name], case, dev, monkeypatch, index_dtype, None)


@pytest.mark.parametrize('index_dtype', DTYPES, ids=['int32', 'int64'])
@pytest.mark.parametrize('name,setting', SMALL, ids=[f'{n}-{s}' for n, s in SMALL])
def test_small_threshold_and_chunk(dev, monkeypatch, name, setting, index_dtype):
    """(64, 48): the pair of test_spmm_hub_rows.  (9, 5): a chunk that is no multiple of 2 or 4,
    threshold + 1 slots are exactly two chunks, most background rows are hubs and the chunk
    items' binary search runs over more than a thousand of them."""
    op = D.OPERATORS[name]
    _run(op, op.cases[0], dev, monkeypatch, index_dtype, setting)


# ---- the plan itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', DTYPES, ids=['int32', 'int64'])
@pytest.mark.parametrize('setting', (None, ) + D.SETTINGS)
def test_hub_plan_matches_the_cpu(dev, setting, index_dtype):
    from pytorch_geometric_amd import _native
    thr, chunk = setting or D.native_settings()
    ei, n, _ = D.build(0, thr, chunk)
    for deg in D.degrees(ei, n):
        ptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]).to(index_dtype).to(dev)
        plan = _native.hub_plan(ptr, thr, chunk)
        rows, cptr, n_hub, n_chunks = plan.rows, plan.chunk_ptr, plan.n_hub, plan.n_chunks
        want = D.expected_plan(deg, thr, chunk)
        assert (n_hub, n_chunks) == (want['n_hub'], want['n_chunks'])
        assert rows.dtype == index_dtype and cptr.dtype == index_dtype
        assert torch.equal(rows.cpu().long(), want['hub_rows'])
        assert torch.equal(cptr.cpu().long(), want['hub_chunk_ptr'])
        if (thr, chunk) == (9, 5):        # several tiles of the chunk scan, unequal counts
            assert n_hub > 1024 and (cptr[1:] - cptr[:-1]).unique().numel() > 8
    # and nothing to plan: no hub row
    assert _native.hub_plan(torch.arange(0, 50, 5, device=dev).to(index_dtype), thr, chunk)[2] == 0


# ---- the control: spmm, which already runs on skewed graphs -------------------------------------------
_SPMM = {}


def _spmm_case(F, setting):
    """x, grad_out, weights and the float64 results of sum / mean / min / max / weighted sum"""
    key = (F, setting)
    if key not in _SPMM:
        ei, n, pl = D.build(0, *setting)
        g = torch.Generator().manual_seed(500 + F)
        x, go = torch.randn(n, F, generator=g), torch.randn(n, F, generator=g)
        w = torch.rand(ei.size(1), generator=g)
        P = {'ei': ei, 'n': n, 'x': x, 'go': go, 'w': w, 'placement': pl, 'profile_ei': ei}
        P['in_deg'], P['out_deg'] = D.degrees(ei, n)
        P['want'] = {dt: {red: _spmm_reference(P, red, dt) for red in
                          ('sum', 'mean', 'min', 'max', 'weighted')}
                     for dt in (torch.float64, torch.float32)}
        _SPMM[key] = P
    return _SPMM[key]


def _spmm_reference(P, red, dtype):
    """plain torch: (out, grad_x, grad_w | None); an empty row gives zeros"""
    x = P['x'].to(dtype).requires_grad_(True)
    w = P['w'].to(dtype).requires_grad_(red == 'weighted')
    src, dst, n = P['ei'][0], P['ei'][1], P['n']
    msg = x[src] * w.unsqueeze(-1) if red == 'weighted' else x[src]
    if red in ('sum', 'mean', 'weighted'):
        out = msg.new_zeros(n, x.size(1)).index_add(0, dst, msg)
        if red == 'mean':
            out = out / P['in_deg'].clamp(min=1).to(dtype).unsqueeze(-1)
    else:
        out = msg.new_zeros(n, x.size(1)).scatter_reduce(
            0, dst.view(-1, 1).expand_as(msg), msg, 'a' + red, include_self=False)
    leaves = [x, w] if red == 'weighted' else [x]
    grads = torch.autograd.grad(out, leaves, P['go'].to(dtype))
    return [out.detach(), grads[0], grads[1] if red == 'weighted' else None]


@pytest.mark.parametrize('index_dtype', DTYPES, ids=['int32', 'int64'])
@pytest.mark.parametrize('F,setting', [(47, None), (256, None), (47, (64, 48)), (47, (9, 5))])
def test_spmm_control(dev, monkeypatch, F, setting, index_dtype):
    """min / max select: their outputs are exact.  Parallel edges tie in an extremum; whichever of
    them takes the gradient, it arrives in the one source row."""
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd._functions import SpmmFunction
    thr, chunk = _patch(monkeypatch, setting)
    P = _spmm_case(F, (thr, chunk))
    n = P['n']
    h = pga.EdgeIndex(P['ei'].to(dev).to(index_dtype), (n, n))
    _check_graph(h, (P['in_deg'], P['out_deg']), P, thr, f'spmm {F}')
    plan = D.expected_plan(P['in_deg'], thr, chunk)
    rows, edge_rows = torch.arange(n), P['ei'][1]
    worst = {}
    for red in ('sum', 'mean', 'min', 'max', 'weighted'):
        x = P['x'].to(dev).requires_grad_(True)
        w = P['w'].to(dev).requires_grad_(True)
        sink = []
        monkeypatch.setattr(_native, 'timing_sink', sink)
        if red == 'weighted':
            out = SpmmFunction.apply(x, w, h, 'sum', 'coo')
            grads = list(torch.autograd.grad(out, [x, w], P['go'].to(dev)))
        else:
            out = pga.utils.spmm(h, x, red)
            grads = list(torch.autograd.grad(out, [x], P['go'].to(dev))) + [None]
        torch.cuda.synchronize()
        monkeypatch.setattr(_native, 'timing_sink', None)
        first = [i for i, _, _ in sink if 'reduce' in i][0]
        if red in ('sum', 'mean', 'weighted'):        # (an extremum is not split into chunks)
            assert first['n_hub'] == plan['n_hub'], (red, first)
        w64, w32 = P['want'][torch.float64][red], P['want'][torch.float32][red]
        what = f'spmm {red} F={F} at {(thr, chunk)}'
        tol = 0.0 if red in ('min', 'max') else D.TOL
        for name, g, a, b, row_of, lengths, side in (
                ('out', out, w64[0], w32[0], rows, P['in_deg'], 'destination'),
                ('grad_x', grads[0], w64[1], w32[1], rows, P['out_deg'], 'source'),
                ('grad_w', grads[1], w64[2], w32[2], edge_rows, P['in_deg'],
                 'destination (of the edge)')):
            if a is None:
                continue
            t = tol if name == 'out' else D.TOL
            worst[f'{red} {name}'] = D.worst_ratio(g, a, row_of, lengths)
            try:
                D.assert_rows_close(g, a, row_of, lengths, tol=t, what=f'{what} {name}', side=side)
            except AssertionError:
                if t == 0.0:
                    raise
                D.assert_rows_close(g, a, row_of, lengths, tol=t, ref32=b, what=f'{what} {name}',
                                    side=side)
    outs = [v for k, v in worst.items() if k.endswith('out')]
    grads = [v for k, v in worst.items() if not k.endswith('out')]
    print(f'\ndegree-sweep | spmm | ({F}, ) | {(thr, chunk)} | {str(index_dtype)[6:]} | '
          f'{max(outs)[0]:.2e} | {max(outs)[1]} | {max(grads)[0]:.2e} | {max(grads)[1]}')
