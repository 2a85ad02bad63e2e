"""nn.FiLMConv on the device: the recorded reference cases with their launch counts, the kernels of
csrc/film.hip through the autograd node against the float64 restatement (tests/_film_ref.py, the
UNSPLIT per-relation mask loop) run on the device, an exact test with every pre-activation at 0,
the shapes of rows, long rows through the chunked schedule, bitwise repeatability, the memory
promise, routing, half inputs, out-of-range edge types, the handle cache and the registered
operators.  Nothing here reads the reference tree.

The kernel-level inputs ``beta``, ``gamma`` and ``h`` are drawn from the grid ``k / 8, |k| <= 16``:
``fmaf(gamma, h, beta)`` is then exact in float32 and in float64 alike, the ReLU mask agrees bit
for bit and exact zeros occur (test_kernels_match_float64 asserts that they do).

Figures measured on one gfx950 device are in profiles/film_conv.md."""
import os
import subprocess
import sys

import pytest
import torch

import _film_ref as R
import test_gpu_transformer as T
from _util import assert_close, assert_close_scaled, gen, random_graph

pytestmark = pytest.mark.gpu

NAMES = ('out', 'grad_h', 'grad_g', 'grad_residual')
TOL = 2e-5
FUSED = ('pygamd_film_forward', 'pygamd_film_backward_dst', 'pygamd_film_backward_src')


# ---- the recorded cases ----------------------------------------------------------------------------
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('name', R.CASES)
def test_golden_cases_on_the_device(dev, monkeypatch, name, index_dtype):
    """A fused case: each of the three entry points ONCE whatever R is and nothing else that
    aggregates or gathers over the edges.  ``max`` and ``Tanh``: the generic route, no film call."""
    c = T._counted(monkeypatch, lambda: R.check_class_case(R.load_golden(), name, dev,
                                                           index_dtype=index_dtype))
    if name in R.FUSED_CASES:
        for fn in FUSED:
            assert c.calls.get(fn) == 1, c.calls
        assert not [n for n in c.calls if 'spmm' in n or 'scatter' in n or 'gather' in n], c.calls
    else:
        assert not [n for n in c.calls if 'pygamd_film_' in n], c.calls


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
def test_golden_stack_on_the_device(dev, monkeypatch, index_dtype):
    c = T._counted(monkeypatch, lambda: R.check_stack(R.load_golden(), dev,
                                                      index_dtype=index_dtype))
    for fn in FUSED:
        assert c.calls.get(fn) == 2, c.calls


# ---- problems ---------------------------------------------------------------------------------------
def _grid(shape, g):
    return torch.randint(-16, 17, shape, generator=g).float() / 8


def _problem(n_src, n_dst, ei, et, F, R, seed, g_rows=None):
    """``h [n_src, R F]`` and ``g [g_rows or n_dst, R 2F]`` from the grid, random normal residual
    and grad_out; ``et`` [E] int64 in [0, R) (None with R = 1)"""
    g = gen(seed)
    return {'ei': ei, 'et': et, 'n_src': n_src, 'n_dst': n_dst, 'F': F, 'R': R,
            'h': _grid((n_src, R * F), g), 'g': _grid((g_rows or n_dst, 2 * R * F), g),
            'res': torch.randn(n_dst, F, generator=g), 'go': torch.randn(n_dst, F, generator=g)}


def _reference(P, mean=False, residual=False, relu=True, device='cuda'):
    """the four of NAMES from the float64 restatement run on ``device``, as CPU tensors"""
    h, g, res = [P[n].to(device, torch.float64).requires_grad_(True) for n in ('h', 'g', 'res')]
    et = None if P['et'] is None else P['et'].to(device)
    out = R.film_messages(h, g, res if residual else None, P['ei'].to(device), et, P['R'],
                          P['n_dst'], aggr='mean' if mean else 'add',
                          act=torch.relu if relu else None)
    leaves = [h, g] + ([res] if residual else [])
    grads = list(torch.autograd.grad(out, leaves, P['go'].to(device, torch.float64),
                                     allow_unused=True))
    grads = [torch.zeros_like(t) if gr is None else gr for t, gr in zip(leaves, grads)]
    return [t.detach().cpu() for t in [out] + grads] + ([] if residual else [None])


def _forms(P, dev, index_dtype, mean):
    """the forms as the layer builds them: dropped types, relation sort, handle, pair forms"""
    from pytorch_geometric_amd.nn import FiLMConv
    layer = FiLMConv(1, 1, num_relations=P['R'])
    et = None if P['et'] is None else P['et'].to(dev).to(index_dtype)
    return layer._build_forms(P['ei'].to(dev).to(index_dtype), et, P['n_src'], P['n_dst'], mean)


def _device_run(P, dev, index_dtype=torch.int64, packed=False, mean=False, residual=False,
                relu=True):
    """the same four through the autograd node.  ``packed``: H and G are the column blocks of one
    [N, 3 R F] plane and the gradient is ONE plane of that shape"""
    from pytorch_geometric_amd._functions import FiLMAggregateFunction
    F, R_ = P['F'], P['R']
    if packed:
        assert P['g'].size(0) == P['n_src']
        h = torch.cat([P['h'], P['g']], dim=1).to(dev).requires_grad_(True)
        g = None
    else:
        h, g = P['h'].to(dev).requires_grad_(True), P['g'].to(dev).requires_grad_(True)
    res = P['res'].to(dev).requires_grad_(True) if residual else None
    key = ('forms', index_dtype, mean)
    if key not in P:
        P[key] = _forms(P, dev, index_dtype, mean)
    out = FiLMAggregateFunction.apply(h, g, res, P[key], relu)
    leaves = [t for t in (h, g, res) if t is not None]
    grads = dict(zip([id(t) for t in leaves], torch.autograd.grad(out, leaves, P['go'].to(dev))))
    got = [out.detach()] + [None if t is None else grads[id(t)] for t in (h, g, res)]
    if packed:
        plane = got[1]
        assert plane.shape == (P['n_src'], 3 * R_ * F) and plane.is_contiguous()
        got[1], got[2] = plane[:, :R_ * F], plane[:, R_ * F:]
    return got


def _check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, f'{what}: {name} should be absent'
            continue
        assert g is not None, f'{what}: {name} is missing'
        assert_close_scaled(g, w.float(), tol=TOL, what=f'{what} {name}')


# ---- the kernels against float64 ------------------------------------------------------------------
_UNIFORM = {}


def _uniform_types(R_):
    if R_ == 1:
        return None
    return torch.randint(0, R_, (T._uniform_graph().size(1), ), generator=gen(300 + R_))


def _uniform_case(F, R_):
    """problem and float64 results at one shape, computed once"""
    if (F, R_) not in _UNIFORM:
        P = _problem(2000, 2000, T._uniform_graph(), _uniform_types(R_), F, R_, 500 + F + 7 * R_)
        P['want'] = {(False, False): _reference(P), (True, True): _reference(P, True, True)}
        _UNIFORM[(F, R_)] = P
    return _UNIFORM[(F, R_)]


@pytest.mark.parametrize('R_', [1, 3, 7])
@pytest.mark.parametrize('F', [1, 5, 24, 64, 100, 128, 132, 256, 512])
def test_kernels_match_float64(dev, F, R_):
    """F over the widths at which resgated.hip's lane shape changes (the list of
    tests/test_gpu_resgated.py without an edge term: below one lane group, odd, the float4 widths
    and the limit, which includes 1 and 512) and one, three and seven relations.  Two separate
    contiguous planes with the sum and no residual on int32 indices, then the column blocks of one
    [N, 3 R F] plane, whose gradient is one plane, with the mean and the residual on int64."""
    P = _uniform_case(F, R_)
    got = _device_run(P, dev, index_dtype=torch.int32)
    _check(got, P['want'][(False, False)], f'({F}, {R_})')
    pre = P['g'][P['ei'][1]][:, F:2 * F] * P['h'][P['ei'][0]][:, :F] + P['g'][P['ei'][1]][:, :F]
    if P['et'] is None and F >= 24:
        assert int((pre == 0).sum()) > 0          # exact zeros occur: the mask at 0 is under test
    got = _device_run(P, dev, index_dtype=torch.int64, packed=True, mean=True, residual=True)
    _check(got, P['want'][(True, True)], f'({F}, {R_}) packed, mean, residual')


@pytest.mark.parametrize('F,R_', [(24, 3), (132, 1), (100, 7)])
def test_the_other_pairings_of_layout_epilogue_and_activation(dev, F, R_):
    """separate planes with the mean and the residual, packed with the sum and no residual, each of
    the mean and the residual alone, and no activation (act_mode 0)"""
    P = _uniform_case(F, R_)
    got = _device_run(P, dev, mean=True, residual=True)
    _check(got, P['want'][(True, True)], f'({F}, {R_}) separate, mean, residual')
    got = _device_run(P, dev, packed=True)
    _check(got, P['want'][(False, False)], f'({F}, {R_}) packed')
    for mean, residual in ((True, False), (False, True)):
        got = _device_run(P, dev, mean=mean, residual=residual)
        _check(got, _reference(P, mean, residual), f'({F}, {R_}) mean {mean} residual {residual}')
    for packed, mean in ((False, True), (True, False)):
        got = _device_run(P, dev, packed=packed, mean=mean, residual=True, relu=False)
        _check(got, _reference(P, mean, True, relu=False), f'({F}, {R_}) identity, mean {mean}')


# ---- exact: every pre-activation at 0 --------------------------------------------------------------
@pytest.mark.parametrize('F,R_', [(24, 3), (132, 1)])
def test_every_pre_activation_exactly_zero(dev, F, R_):
    """beta = 0 and h = 0 with gamma from the grid: every pre-activation is exactly 0, where the
    ReLU is 0 and its derivative is 0 (as torch's).  The output is exactly the residual and all
    three gradients are exactly 0, under the sum and the mean, packed or not."""
    P = dict(_uniform_case(F, R_))        # (the same graph: its cached forms serve)
    P['h'] = torch.zeros_like(P['h'])
    g = P['g'].clone().view(2000, R_, 2, F)
    g[:, :, 0] = 0
    P['g'] = g.view(2000, 2 * R_ * F)
    for packed, mean in ((False, False), (True, True)):
        got = _device_run(P, dev, packed=packed, mean=mean, residual=True)
        assert torch.equal(got[0].cpu(), P['res']), 'out is not exactly the residual'
        assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
        assert torch.equal(got[3].cpu(), P['go'])
        got = _device_run(P, dev, packed=packed, mean=mean)
        assert float(got[0].abs().max()) == 0.0


# ---- shapes of rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,R_', [(24, 3), (132, 2)])
def test_destinations_a_prefix_empty_rows_absent_relation_and_no_edges(dev, F, R_):
    """300 destinations, a prefix of 900 sources whose G has 900 rows; relation 1 absent from the
    call; a destination without slots gets exactly its residual (or exactly 0), sources without
    slots, the rows of G beyond the destinations and every block of the absent relation zero
    gradients; a graph without edges."""
    ei = random_graph(900, 300, 5000, 43)
    ei = ei[:, (ei[1] % 7 != 0) & (ei[0] % 5 != 0)]
    et = torch.randint(0, R_, (ei.size(1), ), generator=gen(44))
    et[et == 1] = 0
    P = _problem(900, 300, ei, et, F, R_, 11, g_rows=900)
    empty_dst = torch.bincount(ei[1], minlength=300) == 0
    empty_src = torch.bincount(ei[0], minlength=900) == 0
    assert int(empty_dst.sum()) >= 40 and int(empty_src.sum()) >= 180
    for packed, mean, residual in ((False, False, False), (True, True, True),
                                   (False, True, False), (True, False, True)):
        got = _device_run(P, dev, packed=packed, mean=mean, residual=residual)
        _check(got, _reference(P, mean, residual), f'prefix ({F}, {R_}) {packed} {mean} {residual}')
        assert got[0].shape == (300, F) and got[1].shape == (900, R_ * F)
        assert got[2].shape == (900, 2 * R_ * F)
        rows = got[0].cpu()[empty_dst]
        if residual:
            assert torch.equal(rows, P['res'][empty_dst])              # exactly the residual
            assert torch.equal(got[3].cpu(), P['go'])                  # its gradient: grad_out
        else:
            assert float(rows.abs().max()) == 0.0                      # exact zeros
        assert float(got[2].cpu()[:300][empty_dst].abs().max()) == 0.0
        assert float(got[2][300:].abs().max()) == 0.0
        assert float(got[1].cpu()[empty_src].abs().max()) == 0.0
        assert float(got[1][:, F:2 * F].abs().max()) == 0.0            # relation 1: no edge
        assert float(got[2][:, 2 * F:4 * F].abs().max()) == 0.0
    Z = _problem(50, 40, torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                 F, R_, 12)
    for mean, residual in ((False, False), (True, True)):
        got = _device_run(Z, dev, mean=mean, residual=residual)
        assert torch.equal(got[0].cpu(), Z['res'] if residual else torch.zeros(40, F))
        assert got[1].shape == (50, R_ * F) and got[2].shape == (40, 2 * R_ * F)
        assert all(float(t.abs().max()) == 0.0 for t in got[1:3])


def test_rows_of_1_63_64_65_slots(dev):
    """destination i has (1, 63, 64, 65)[i % 4] slots, relations mixed in every row: the slot loop's
    unrolled body with and without a remainder"""
    n, F, R_ = 64, 24, 3
    deg = torch.tensor([1, 63, 64, 65])[torch.arange(n) % 4]
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (dst.numel(), ), generator=gen(61))
    et = torch.randint(0, R_, (dst.numel(), ), generator=gen(62))
    perm = torch.randperm(dst.numel(), generator=gen(63))
    P = _problem(n, n, torch.stack([src, dst])[:, perm].contiguous(), et[perm], F, R_, 64)
    for packed, mean in ((False, False), (True, True)):
        got = _device_run(P, dev, packed=packed, mean=mean, residual=True)
        _check(got, _reference(P, mean, True), f'rows of 1, 63, 64, 65 slots, mean {mean}')


def _csr_of(P, dev, index_dtype=torch.int64):
    """(rowptr, col, edge_id) of a stable by-destination sort of the edges AS GIVEN"""
    order = torch.argsort(P['ei'][1], stable=True)
    ptr = torch._convert_indices_from_coo_to_csr(P['ei'][1][order], P['n_dst'])
    return (ptr.to(dev).to(index_dtype), P['ei'][0][order].to(dev).to(index_dtype),
            order.to(dev).to(index_dtype))


def _mean_scale(P):
    """1 / |N_r(i)| per edge, on the host"""
    key = P['et'] * P['n_dst'] + P['ei'][1]
    return (1.0 / torch.bincount(key, minlength=P['R'] * P['n_dst'])[key].double()).float()


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
def test_alternating_relations_in_a_row_through_the_operator(dev, monkeypatch, index_dtype):
    """The operator takes the caller's handle as it is: here the slots of every destination
    alternate between relations 0, 1, 2, 0, 1, ... (the edges are NOT sorted by relation), so a
    wave reloads [beta | gamma] at every slot.  The result does not depend on the in-row order;
    each entry point is called once."""
    import pytorch_geometric_amd.ops  # noqa: F401  (registers the operators)
    n, F, R_ = 200, 24, 3
    dst = torch.repeat_interleave(torch.arange(n), 9)
    src = torch.randint(0, n, (dst.numel(), ), generator=gen(71))
    et = torch.arange(dst.numel()) % R_
    P = _problem(n, n, torch.stack([src, dst]), et, F, R_, 72)
    ptr, col, eid = _csr_of(P, dev, index_dtype)
    assert torch.equal(eid.cpu().long(), torch.arange(dst.numel()))     # the row order is the edge order
    rel = et.to(dev).to(torch.int32)
    op = torch.ops.pyg_amd.film_aggregate
    for mean in (False, True):
        scale = _mean_scale(P).to(dev) if mean else None
        h, g, res = [P[k].to(dev).requires_grad_(True) for k in ('h', 'g', 'res')]
        state = {}

        def step():
            out = op(h, g, res, ptr, col, eid, rel, scale, R_, True)
            state['got'] = [out.detach()] + list(torch.autograd.grad(out, [h, g, res],
                                                                     P['go'].to(dev)))

        c = T._counted(monkeypatch, step)
        for fn in FUSED:
            assert c.calls.get(fn) == 1, c.calls
        _check(state['got'], _reference(P, mean, True), f'alternating relations, mean {mean}')


# ---- long rows ------------------------------------------------------------------------------------
THRESHOLD, CHUNK = 512, 128
_LONG = {}


def _long_case():
    """N = 1500, F = 64, R = 3: destination 5 has 700 slots, all of relation 1 (one long (relation,
    destination) pair), destination 11 exactly THRESHOLD + 1 of mixed relations, source 7 has 650
    out-slots of relation 2 (one long (relation, source) pair); the rest is uniform."""
    if not _LONG:
        g = gen(51)
        n, R_ = 1500, 3
        src = torch.randint(0, n, (8000 + 700 + THRESHOLD + 1, ), generator=g)
        src[src == 7] = 8
        src = torch.cat([src, torch.full((650, ), 7)])
        base = torch.randint(0, n, (8000, ), generator=g)
        base[(base == 5) | (base == 11)] = 12
        dst = torch.cat([base, torch.full((700, ), 5), torch.full((THRESHOLD + 1, ), 11),
                         torch.randint(12, n, (650, ), generator=g)])
        et = torch.randint(0, R_, (src.numel(), ), generator=g)
        et[8000:8700] = 1
        et[-650:] = 2
        perm = torch.randperm(src.numel(), generator=g)
        P = _problem(n, n, torch.stack([src, dst])[:, perm].contiguous(), et[perm], 64, R_, 57)
        P['want'] = {False: _reference(P), True: _reference(P, True, True)}
        _LONG['P'] = P
    return {k: v for k, v in _LONG['P'].items() if not isinstance(k, tuple)}


def _lower_the_threshold(monkeypatch):
    """the package's hub threshold and chunk until the test ends (handles made after this)"""
    from pytorch_geometric_amd import _native
    monkeypatch.setattr(_native, 'HUB_THRESHOLD', THRESHOLD)
    monkeypatch.setattr(_native, 'HUB_CHUNK', CHUNK)
    return _native


def _plan(counts):
    """(n_hub, n_chunks) of rows with these slot counts, as the hub plan splits them"""
    long = counts[counts > THRESHOLD]
    return int(long.numel()), int(((long + CHUNK - 1) // CHUNK).sum())


def test_long_rows_match_float64_and_are_chunked(dev, monkeypatch):
    """Rows past the (lowered) threshold are split into chunks whose partials are merged in chunk
    order, in all three launches; the epilogue runs once after the merge: the mean divides once,
    the residual is added once.  ``timing_sink`` shows the plan computed from the degrees."""
    native = _lower_the_threshold(monkeypatch)
    P = _long_case()
    n, R_ = P['n_dst'], P['R']
    src, dst = P['ei']
    plans = {'forward': _plan(torch.bincount(dst, minlength=n)),
             'backward_dst': _plan(torch.bincount(P['et'] * n + dst, minlength=R_ * n)),
             'backward_src': _plan(torch.bincount(P['et'] * n + src, minlength=R_ * n))}
    assert plans['forward'] == (2, -(-700 // CHUNK) + -(-(THRESHOLD + 1) // CHUNK))
    assert plans['backward_dst'] == (1, -(-700 // CHUNK)) and plans['backward_src'][0] == 1
    for mean in (False, True):
        sink = []
        monkeypatch.setattr(native, 'timing_sink', sink)
        got = _device_run(P, dev, mean=mean, residual=mean, packed=mean)
        torch.cuda.synchronize()
        monkeypatch.setattr(native, 'timing_sink', None)
        _check(got, P['want'][mean], f'long rows, mean {mean}')
        info = {i['op']: i for i, _, _ in sink if i.get('kind') == 'film'}
        assert set(info) == set(plans)
        for op, (n_hub, n_chunks) in plans.items():
            assert (info[op]['n_hub'], info[op]['n_chunks']) == (n_hub, n_chunks), (op, info[op])
            assert info[op]['F'] == 64 and info[op]['R'] == R_


def test_two_runs_are_bitwise_identical(dev, monkeypatch):
    """No float atomics anywhere and grids that depend on the problem only: every output and
    gradient repeats bit for bit on random normal inputs, long rows included."""
    _lower_the_threshold(monkeypatch)
    P = _long_case()
    g = gen(58)
    P['h'], P['g'] = torch.randn(P['h'].shape, generator=g), torch.randn(P['g'].shape, generator=g)
    for kw in (dict(), dict(mean=True, residual=True, packed=True)):
        a = _device_run(P, dev, **kw)
        b = _device_run(P, dev, **kw)
        for name, x, y in zip(NAMES, a, b):
            assert (x is None) == (y is None)
            if x is not None:
                assert torch.equal(x, y), f'{name} differs between two runs'
    U = dict(_uniform_case(132, 3))
    a, b = _device_run(U, dev), _device_run(U, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)


# ---- nothing of size E x F -----------------------------------------------------------------------------
def test_keeps_nothing_of_edge_times_width(dev):
    """N = 2048, E = 131072, F = 64, R = 2.  Above the inputs, over forward + backward, the fused
    route allocates node-sized planes only: out (0.5 MiB), the zero-filled [N, 3 R F] gradient
    plane (3 MiB) and the residual's gradient, which is grad_out — about 5 MiB with the
    allocator's rounding, against 32 MiB for a single [E, F] float plane.  The bound, half such a
    plane, follows from that count, not from a measurement."""
    from pytorch_geometric_amd._functions import FiLMAggregateFunction
    N, E, F, R_ = 2048, 131072, 64, 2
    P = {'ei': random_graph(N, N, E, 71), 'et': torch.randint(0, R_, (E, ), generator=gen(70)),
         'n_src': N, 'n_dst': N, 'R': R_}
    forms = _forms(P, dev, torch.int64, True)
    forms.pairs[0].hub, forms.pairs[1].hub, forms.fwd.hub      # (the handles warm)
    g = gen(72)
    plane = torch.randn(N, 3 * R_ * F, generator=g).to(dev).requires_grad_(True)
    res = torch.randn(N, F, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(N, F, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = FiLMAggregateFunction.apply(plane, None, res, forms, True)
    grads = torch.autograd.grad(out, [plane, res], go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f'peak above the inputs: {extra / 2 ** 20:.1f} MiB (one [E, F]: '
          f'{E * F * 4 / 2 ** 20:.0f} MiB)')
    assert extra < E * F * 4 / 2
    assert all(bool(torch.isfinite(t).all()) for t in grads)


# ---- routing --------------------------------------------------------------------------------------------
def _layer64(conv, x, ei, et, **kw):
    state = {k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
    return R.film_layer(state, x, x, ei, et, conv.num_relations, **kw)


def test_routing(dev, monkeypatch):
    """``fuse = False``, ``max``, ``act=Tanh()``, ``target_to_source``, a forward hook on the
    message, a subclass with its own ``message`` (which is used) and more than 512 channels take
    the generic route and match float64; the supported layers take the new route."""
    from pytorch_geometric_amd.nn import FiLMConv

    class _Scaled(FiLMConv):
        def message(self, x_j, beta_i, gamma_i):
            return 0.5 * super().message(x_j, beta_i, gamma_i)

    ei = random_graph(300, 300, 3000, 91)
    et = torch.randint(0, 3, (3000, ), generator=gen(90))
    for what, F, kw in (
            ('fuse = False', 24, {}),
            ('max', 24, dict(aggr='max')),
            ('Tanh', 24, dict(act=torch.nn.Tanh())),
            ('target_to_source', 24, dict(flow='target_to_source')),
            ('message hook', 24, {}),
            ('subclass with its own message', 24, {}),
            ('channels = 520', 520, {}),
            ('supported', 24, {}),
            ('supported, add', 24, dict(aggr='add')),
            ('supported, no activation', 24, dict(act=None))):
        torch.manual_seed(9)
        kind = _Scaled if what.startswith('subclass') else FiLMConv
        conv = kind(16, F, num_relations=3, **kw).to(dev)
        conv.fuse = what != 'fuse = False'
        seen = []
        if what == 'message hook':
            conv.register_message_forward_hook(lambda mod, args, out: seen.append(out.shape[1]))
        x0 = torch.randn(300, 16, generator=gen(92))
        x = x0.to(dev).requires_grad_(True)
        state = {}

        def step():
            state['out'] = conv(x, ei.to(dev), et.to(dev))
            state['grad'] = torch.autograd.grad(state['out'].sum(), [x])

        c = T._counted(monkeypatch, step)
        fused = sorted(n for n in c.calls if n in FUSED)
        if what.startswith('supported'):
            assert fused == sorted(FUSED), (what, c.calls)
        else:
            assert not fused, (what, c.calls)
        if what == 'message hook':
            assert seen == [F, F, F], seen                 # one propagate per relation
        x64 = x0.double().requires_grad_(True)
        act = 'tanh' if what == 'Tanh' else 'none' if 'act' in kw else 'relu'
        want = _layer64(conv, x64, ei, et, aggr=kw.get('aggr', 'mean'), act=act,
                        flow=kw.get('flow', 'source_to_target'))
        if kind is _Scaled:      # (0.5 * message; the skip term is not a message)
            skip = _layer64(conv, x64, ei[:, :0], et[:0], act=act)
            want = 0.5 * (want - skip) + skip
        assert_close_scaled(state['out'], want.detach().float(), tol=TOL, what=f'{what} out')
        assert_close_scaled(state['grad'][0], torch.autograd.grad(want.sum(), [x64])[0].float(),
                            tol=TOL, what=f'{what} grad_x')


def test_float64_tensors_are_never_narrowed(dev, monkeypatch):
    """float64 device tensors do not take the fused route: no film kernel runs and nothing is
    cast down.  On the host the same float64 layer computes in float64 and matches the
    restatement."""
    from pytorch_geometric_amd.nn import FiLMConv
    ei = random_graph(300, 300, 3000, 91)
    et = torch.randint(0, 2, (3000, ), generator=gen(90))
    torch.manual_seed(9)
    conv = FiLMConv(16, 24, num_relations=2).to(dev, torch.float64)
    conv.fuse = True
    x0 = torch.randn(300, 16, generator=gen(93)).double()
    assert conv._fusable(x0.to(dev), x0.to(dev)) is False

    def step():
        try:
            out = conv(x0.to(dev), ei.to(dev), et.to(dev))
        except (ValueError, RuntimeError) as e:    # (the generic device route serves float32)
            assert any(w in str(e) for w in ('float32', 'dtype', 'Float', 'Double')), e
        else:
            assert out.dtype == torch.float64

    c = T._counted(monkeypatch, step)
    assert not [n for n in c.calls if 'pygamd_film_' in n], c.calls
    host = conv.cpu()
    x64 = x0.clone().requires_grad_(True)
    out = host(x64, ei, et)
    assert out.dtype == torch.float64
    want = _layer64(host, x64, ei, et)
    assert float((out - want).detach().abs().max()) <= 1e-12 * float(want.detach().abs().max())


def test_switch_off_in_a_child_process(dev):
    """``PYGAMD_FUSE_FILM=0`` is read at import: a layer made in such a process starts with ``fuse
    = False`` and its forward on the device never reaches the film kernels."""
    code = (
        "import torch\n"
        "from pytorch_geometric_amd import _native\n"
        "from pytorch_geometric_amd.nn import FiLMConv\n"
        "def refuse(*a, **k):\n"
        "    raise AssertionError('the fused route was taken')\n"
        "_native.film_forward = refuse\n"
        "conv = FiLMConv(8, 6, num_relations=2).cuda()\n"
        "assert conv.fuse is False\n"
        "x = torch.randn(50, 8, device='cuda')\n"
        "ei = torch.randint(0, 50, (2, 400), device='cuda')\n"
        "et = torch.randint(0, 2, (400, ), device='cuda')\n"
        "out = conv(x, ei, et)\n"
        "assert out.shape == (50, 6) and bool(torch.isfinite(out).all())\n"
        "print('generic route')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYGAMD_FUSE_FILM='0',
               PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and 'generic route' in res.stdout, res.stderr[-2000:]


def test_half_inputs_are_widened(dev, monkeypatch):
    """float16 and bfloat16 layers take the fused route, compute in float32 and hand the result
    back in their dtype: against the float32 layer whose parameters and inputs hold the SAME
    rounded values, the only difference is the last rounding to the low dtype, one unit in the
    last place of 2^-11 (float16) or 2^-8 (bfloat16) relative to each entry."""
    import copy
    from pytorch_geometric_amd.nn import FiLMConv
    torch.manual_seed(4)
    conv = FiLMConv(16, 24, num_relations=3).to(dev)
    conv.fuse = True
    x = torch.randn(300, 16, generator=gen(94)).to(dev)
    ei = random_graph(300, 300, 3000, 95).to(dev)
    et = torch.randint(0, 3, (3000, ), generator=gen(96)).to(dev)
    for low, ulp in ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)):
        half = copy.deepcopy(conv).to(low)
        wide = copy.deepcopy(half).float()              # the rounded parameters, in float32
        xl = x.to(low)
        want = wide(xl.float(), ei, et)
        state = {}
        c = T._counted(monkeypatch, lambda: state.update(out=half(xl, ei, et)))
        assert c.calls.get('pygamd_film_forward') == 1, (low, c.calls)
        got = state['out']
        assert got.dtype == low
        assert_close(got.float(), want, rtol=ulp, atol=1e-6, what=f'{low}')
        xg = xl.clone().requires_grad_(True)            # the backward takes the fused route too
        c = T._counted(monkeypatch, lambda: half(xg, ei, et).float().sum().backward())
        assert c.calls.get('pygamd_film_backward_dst') == 1, (low, c.calls)
        assert c.calls.get('pygamd_film_backward_src') == 1, (low, c.calls)
        assert xg.grad.dtype == low and bool(torch.isfinite(xg.grad).all())


@pytest.mark.parametrize('aggr', ['mean', 'add'])
def test_out_of_range_edge_types_contribute_nothing(dev, monkeypatch, aggr):
    """types outside [0, R) — negative ones too — are dropped once when the handle is built: the
    fused output and gradient equal, bit for bit, those of the run with these edges removed"""
    from pytorch_geometric_amd.nn import FiLMConv
    torch.manual_seed(5)
    conv = FiLMConv(16, 24, num_relations=3, aggr=aggr).to(dev)
    conv.fuse = True
    ei = random_graph(300, 300, 3000, 97).to(dev)
    et = torch.randint(-1, 5, (3000, ), generator=gen(98)).to(dev)
    keep = (et >= 0) & (et < 3)
    assert 800 < int(keep.sum()) < 2200
    x = torch.randn(300, 16, generator=gen(99)).to(dev)
    got = []
    for e, t in ((ei, et), (ei[:, keep].contiguous(), et[keep].contiguous())):
        xg = x.clone().requires_grad_(True)
        c = T._counted(monkeypatch, lambda: got.append(conv(xg, e, t)))
        assert c.calls.get('pygamd_film_forward') == 1, c.calls
        got.append(torch.autograd.grad(got[-1].sum(), [xg])[0])
    assert torch.equal(got[0], got[2]) and torch.equal(got[1], got[3])
    x64 = x.cpu().double()
    assert_close_scaled(got[0], _layer64(conv, x64, ei.cpu(), et.cpu(), aggr=aggr).float(),
                        tol=TOL, what='out-of-range types against float64')


def test_the_handles_are_cached_on_the_layer(dev, monkeypatch):
    """a second call with the same tensors builds no new sort; a new ``edge_type`` tensor or an
    in-place change does"""
    from pytorch_geometric_amd.nn import FiLMConv
    torch.manual_seed(6)
    conv = FiLMConv(16, 24, num_relations=3).to(dev)
    conv.fuse = True
    ei = random_graph(300, 300, 3000, 97).to(dev)
    et = torch.randint(0, 3, (3000, ), generator=gen(98)).to(dev)
    x = torch.randn(300, 16, generator=gen(99)).to(dev).requires_grad_(True)

    def step():
        conv(x, ei, et).sum().backward()

    first = T._counted(monkeypatch, step)
    assert first.calls.get('pygamd_index_sort', 0) >= 3, first.calls
    forms = conv._film_cache[-1]
    again = T._counted(monkeypatch, step)
    assert 'pygamd_index_sort' not in again.calls, again.calls
    assert not [n for n in again.calls if 'hub_plan' in n or 'minmax' in n], again.calls
    for fn in FUSED:
        assert again.calls.get(fn) == 1, again.calls
    assert conv._film_cache[-1] is forms
    et.add_(0)                                             # an in-place change: a new version
    changed = T._counted(monkeypatch, step)
    assert changed.calls.get('pygamd_index_sort', 0) >= 3 and conv._film_cache[-1] is not forms


# ---- the registered operators -----------------------------------------------------------------------
def test_operator_under_fake_tensors_and_compile(dev):
    import pytorch_geometric_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'film_aggregate' in ops.OPS and 'film_aggregate_backward' in ops.OPS
    op = torch.ops.pyg_amd.film_aggregate
    with FakeTensorMode():
        h = torch.empty(50, 72, device='cuda', requires_grad=True)
        g = torch.empty(12, 144, device='cuda', requires_grad=True)
        plane = torch.empty(12, 216, device='cuda', requires_grad=True)
        res = torch.empty(12, 24, device='cuda')
        ptr = torch.empty(13, dtype=torch.int32, device='cuda')
        col = torch.empty(400, dtype=torch.int32, device='cuda')
        eid = torch.empty(400, dtype=torch.int32, device='cuda')
        rel = torch.empty(400, dtype=torch.int32, device='cuda')
        scale = torch.empty(400, device='cuda')
        for args in ((h, g, res, ptr, col, eid, rel, scale, 3, True),
                     (h, g, None, ptr, col, None, rel, None, 3, False),
                     (plane, None, None, ptr, col, None, rel, None, 3, True)):
            out = op(*args)
            assert out.shape == (12, 24) and out.requires_grad
            assert out.device.type == 'cuda' and out.dtype == torch.float32

    P = _uniform_case(64, 3)
    want = P['want'][(True, True)]
    ptr, col, eid = _csr_of(P, dev)
    rel, scale = P['et'].to(dev).to(torch.int32), _mean_scale(P).to(dev)
    go = P['go'].to(dev)

    def fn(h, g, res):
        return (op(h * 1.0, g, res, ptr, col, eid, rel, scale, 3, True) * go).sum()

    def leaves():
        return [P[n].to(dev).requires_grad_(True) for n in ('h', 'g', 'res')]

    results = []
    for f in (fn, torch.compile(fn, backend='aot_eager', fullgraph=True)):
        ls = leaves()
        y = f(*ls)
        results.append([y.detach()] + list(torch.autograd.grad(y, ls)))
    for x, y in zip(*results):
        assert_close(y, x, what='compiled vs eager')
    ls = [t.detach() for t in leaves()]
    out = op(*ls, ptr, col, eid, rel, scale, 3, True)
    _check([out] + results[0][1:], want, 'operator')
    # edge_id = None: rel and scale follow the slots of col
    assert torch.equal(op(*ls, ptr, col, None, rel[eid], scale[eid], 3, True), out)
    # the packed plane, the sum
    plane = torch.cat([P['h'], P['g']], dim=1).to(dev).requires_grad_(True)
    y = op(plane, None, None, ptr, col, eid, rel, None, 3, True)
    g_plane, = torch.autograd.grad(y, [plane], go)
    _check([y.detach(), g_plane[:, :192], g_plane[:, 192:], None], P['want'][(False, False)],
           'operator, packed')
    with pytest.raises(ValueError, match='rel'):           # a relation the planes do not hold
        op(*ls, ptr, col, eid, rel + 1, scale, 3, True)
    torch.library.opcheck(op, (*leaves(), ptr, col, eid, rel, scale, 3, True))
    torch.library.opcheck(op, (plane.detach().requires_grad_(True), None, None, ptr, col, eid,
                               rel, None, 3, False))
