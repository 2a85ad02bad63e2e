"""The one-pass attention kernels (gatv2.hip, transformer.hip, its edge variant and, through
HGTConv, the transformer kernel on a stacked handle) on masked and non-finite scores: -inf in
every position of the slot order the online-softmax recurrence can tell apart, +inf, NaN, 1e4- and
3e38-magnitude scores, ramps that rescale the accumulator to 0 at every slot, hub rows with fully
masked chunks (tests/_attn_nonfinite_cases.py) — against the restatements
``_transformer_ref.attend``, ``_gatv2_ref.attend`` and ``_transformer_edge_ref.attend_edge`` run on
the CPU in float32, which tests/test_attention_nonfinite_host.py pins to the real reference's
record on such inputs.

The rules are those of tests/test_gpu_nonfinite.py:
  * forward: ``out`` (``z``) and ``alpha`` at ``assert_close``'s 1e-5 — NaN for NaN, exactly 0
    where the reference has exactly 0; the (destination, head) pairs of the 1e4 / 3e38 kinds and
    of the ramps are judged against a float64 evaluation instead (``assert_sum_close``): for
    C = 5 the CPU divides by sqrt(C) where the kernel multiplies by 1 / sqrt(C), an ulp of the
    score apart;
  * backward: per (destination, head), a reference gradient that is finite everywhere must be
    matched — like the values, within 1e-5 of the float64 evaluation or as close to it as twice
    the float32 restatement's own worst error (``assert_sum_close``: rows of 70 slots times 128
    channels are float32 sums on both sides); the two destinations that the edge term masks hold
    1e29-sized gradients in every head (``a[:, 0] = -1e30`` is read by all of them) and are
    judged at 2e-5 of their own scale; hub rows at 2e-5 of the tensor's scale, as the long rows
    of the kernels' own tests.  One that is non-finite anywhere must be non-finite somewhere here
    (``check_backward``).  Every
    gradient row belongs to the destination of its node or of its one edge; ``att``, which all
    destinations share, is compared only when its reference gradient is finite.  In the pairs
    judged against float64 the gradients are bounded, kind by kind, by the reference's own
    float32 error against float64, as ``test_softmax_aggregation_with_a_masked_column`` does —
    and the one entry per row that multiplies ``d s`` by the large input itself (channel 0 of
    ``grad_query`` / ``grad_x_r`` / ``grad_x_l``) by a few float32 ulps of the sum of the
    magnitudes it cancels (``conditioning``; ``assert_sum_close``'s ``abs_sum``);
  * isolation: no float atomics here, so ``out``, ``alpha`` and every gradient row of an ordinary
    (destination, head) are BIT FOR BIT what the same call gives on a copy whose special scores
    are replaced by ``randn``.  Outside this rule: the gradient of the shared ``att``, and
    ``grad_a`` of a special destination's edges (it sums over the heads).
"""
import math

import pytest
import torch

import _attn_nonfinite_cases as A
from _util import assert_close, assert_close_scaled, assert_sum_close, gen
from test_gpu_nonfinite import check_backward, group_all

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
RUNS = {'transformer': ('attend', 'packed', 'score'), 'gatv2': ('attend', 'score'),
        'edge': ('attend', 'score')}
_CACHE = {}


def _case(family, layout, hub=None):
    """the case and its float32 / float64 references, computed once and left alone"""
    key = (family, layout, hub)
    if key not in _CACHE:
        case = A.build(family, *layout, seed=8100 + 7 * sum(layout) + len(family), hub=hub)
        A.check_placements(case, case['perm'], case['ptr'])
        refs = {(score, dt): A.reference(case, score, dt)
                for score in (False, True) for dt in (torch.float32, torch.float64)}
        _CACHE[key] = (case, refs)
    return _CACHE[key]


def device_run(case, T, run, dev, index_dtype):
    """the structure of ``A.reference`` through the autograd nodes, and the handle"""
    from pytorch_geometric_amd import _functions as Fn
    from pytorch_geometric_amd import as_edge_index
    fam, S, C = case['family'], case['n_dst'], case['C']
    score = run == 'score'
    graph = as_edge_index(case['ei'].to(dev).to(index_dtype), case['E'], S)
    ct = {n: t.to(dev) for n, t in A.cotangents(case).items()}
    L = {n: T[n].to(dev).requires_grad_(True) for n in A.LEAVES[fam]}
    scale = 1.0 / math.sqrt(C)
    names = A.SCORE_LEAVES[fam] if score else A.LEAVES[fam]
    outs = []
    if fam == 'gatv2':
        args = (L['x_l'], L['x_r'], L['att'], graph, A.SLOPE, S)
        if score:
            alpha = Fn.Gatv2ScoreFunction.apply(*args)
        else:
            outs = [Fn.Gatv2AttendFunction.apply(*args)]
            alpha = outs[0].grad_fn.saved_tensors[3]
        heads = [ct['go']]
    elif fam == 'transformer':
        if score:
            alpha = Fn.TransformerScoreFunction.apply(L['q'], L['k'], graph, scale, S)
        elif run == 'packed':
            kv = torch.stack([L['k'].detach(), L['v'].detach()], dim=1).requires_grad_(True)
            outs = [Fn.TransformerAttendFunction.apply(L['q'], kv, None, graph, scale, S)]
            alpha = outs[0].grad_fn.saved_tensors[3]
        else:
            outs = [Fn.TransformerAttendFunction.apply(L['q'], L['k'], L['v'], graph, scale, S)]
            alpha = outs[0].grad_fn.saved_tensors[3]
        heads = [ct['go']]
    else:
        if score:
            alpha = Fn.TransformerEdgeScoreFunction.apply(L['q'], L['k'], L['a'], L['b'], graph,
                                                          scale, S)
        else:
            outs = list(Fn.TransformerEdgeAttendFunction.apply(L['q'], L['k'], L['v'], L['a'],
                                                               L['b'], graph, scale, S))
            alpha = outs[0].grad_fn.saved_tensors[5]
        heads = [ct['go'], ct['gz']]
    if score:
        grads = torch.autograd.grad(alpha, [L[n] for n in names], ct['ga'])
    elif run == 'packed':
        g_q, g_kv = torch.autograd.grad(outs, [L['q'], kv], heads)
        grads = [g_q, g_kv[:, 0], g_kv[:, 1]]
    else:
        grads = torch.autograd.grad(outs, [L[n] for n in names], heads)
    torch.cuda.synchronize()
    return {'outs': [o.detach().cpu() for o in outs], 'alpha': alpha.detach().cpu(),
            'grads': {n: g.detach().cpu() for n, g in zip(names, grads)}}, graph


def _kinds_off(case, dst_of_row, got, ref):
    """the kinds of the destinations where ``got`` is not ``ref`` at 1e-5 (for the message)"""
    bad = ~torch.isclose(got, ref, rtol=1e-5, atol=1e-5, equal_nan=True)
    bad = bad.reshape(bad.size(0), -1).any(1)
    return sorted({case['kinds'][int(i)] or f'ordinary destination {int(i)}'
                   for i in dst_of_row[bad]})


def _large_masks(case):
    """kind -> [S, H] bool: the (destination, head) pair judged against float64"""
    out = {}
    for kind, i in A.large_groups(case).items():
        m = torch.zeros(case['n_dst'], case['H'], dtype=torch.bool)
        m[i, case['h']] = True
        out[kind] = m
    return out


def _expand(mask_dh, like):
    """[rows, H] bool -> the shape of ``like`` ([rows, H] or [rows, H, X])"""
    return mask_dh if like.dim() == 2 else mask_dh.unsqueeze(-1).expand_as(like)


def judge_forward(case, got, ref32, ref64, what):
    dst_slot = torch.arange(case['n_dst']).repeat_interleave(case['lens'])
    large = _large_masks(case)
    any_large = torch.zeros(case['n_dst'], case['H'], dtype=torch.bool)
    for m in large.values():
        any_large |= m
    items = [(f'out[{n}]', g, r32, r64, torch.arange(case['n_dst']))
             for n, (g, r32, r64) in enumerate(zip(got['outs'], ref32['outs'], ref64['outs']))]
    items.append(('alpha', got['alpha'], ref32['alpha'], ref64['alpha'], dst_slot))
    for name, g, r32, r64, dst_of_row in items:
        print(f'{what} {name}: NaN here {int(g.isnan().sum())}, NaN in the reference '
              f'{int(r32.isnan().sum())}')
        skip = _expand(any_large[dst_of_row], g)
        off = _kinds_off(case, dst_of_row, torch.where(skip, r32, g), r32)
        assert_close(torch.where(skip, r32, g), r32, what=f'{what} {name} (kinds off: {off})')
        for kind, m in large.items():
            sel = _expand(m[dst_of_row], g)
            assert_sum_close(g[sel], r32[sel], r64[sel], what=f'{what} {name} {kind} vs fp64')
    zero = ref32['alpha'] == 0
    assert bool((got['alpha'][zero] == 0).all()), \
        f'{what}: {int((got["alpha"][zero] != 0).sum())} coefficients are exactly 0 in the ' \
        f'reference and not here'


def conditioning(case, ref64, score):
    """leaf -> a leaf-shaped tensor, 0 except at the ill-conditioned entries of the pairs judged
    against float64, where it holds the sum of magnitudes that entry cancels.  ``d s[k] = alpha[k]
    (d alpha[k] - D)`` carries a float32 error of an ulp of ``alpha (|d alpha| + |D|)``; one entry
    per row multiplies it by the large input (1e4 ... 3e38):
      * transformer: ``grad_query[i, h, 0] = scale sum_k d s[k] key[k, h, 0]``;
      * GATv2 (not in score mode): ``d alpha = <grad_out, x_l[k]>`` and ``D = <grad_out, out>``
        themselves hold the large channel, and channel 0 of ``grad_x_r[i]`` and of every
        ``grad_x_l[k]`` is ``att[h, 0] d s``.
    Everything comes from the inputs and the float64 evaluation, nothing from the device."""
    fam, h, T = case['family'], case['h'], case['T']
    ct = {n: t.double() for n, t in A.cotangents(case).items()}
    out = {n: torch.zeros(T[n].shape, dtype=torch.float64) for n in ('q', 'x_r', 'x_l') if n in T}
    for i in A.large_groups(case).values():
        lo, hi = int(case['ptr'][i]), int(case['ptr'][i + 1])
        j = case['slot_src'][lo:hi]
        alpha = ref64['alpha'][lo:hi, h]
        if fam == 'gatv2':
            if score:
                continue
            g = ct['go'][i, h].abs()
            mass = (g * (T['x_l'][j, h].double().abs() + ref64['outs'][0][i, h].abs())).sum(-1)
            S = float(T['att'][h, 0].abs()) * float((alpha * mass).sum())
            out['x_r'][i, h, 0] = S
            out['x_l'][j, h, 0] = S
            continue
        if score:
            da = ct['ga'][lo:hi, h]
            D = (alpha * da).sum()
        else:
            da = (ct['go'][i, h] * T['v'][j, h].double()).sum(-1)
            D = (ct['go'][i, h] * ref64['outs'][0][i, h]).sum()
            if fam == 'edge':
                da = da + (ct['gz'][i, h] * T['a'][case['perm'][lo:hi]].double()).sum(-1)
                D = D + (ct['gz'][i, h] * ref64['outs'][1][i, h]).sum()
        key0 = T['k'][j, h, 0].double().abs()
        out['q'][i, h, 0] = float((alpha * (da.abs() + D.abs()) * key0).sum()) / math.sqrt(case['C'])
    return out


def judge_backward(case, got, ref32, ref64, what, close=None):
    large = _large_masks(case)
    S = case['n_dst']
    cond = conditioning(case, ref64, score=not got['outs']) if large else {}
    failures = []

    def attempt(fn, *args, **kw):   # every tensor and kind is judged, also behind one that fails
        try:
            fn(*args, **kw)
        except AssertionError as exc:
            failures.append(str(exc)[:300])
    for name, g in got['grads'].items():
        r32, r64 = ref32['grads'][name], ref64['grads'][name]
        assert g.shape == r32.shape, (what, name)
        if name == 'att':
            if bool(r32.isfinite().all()):
                assert_close(g, r32, what=f'{what} grad att')
            continue
        g2, index = A.per_head(case, name, g)
        r2, _ = A.per_head(case, name, r32)
        e2, _ = A.per_head(case, name, r64)
        done = torch.zeros_like(g2, dtype=torch.bool)
        c2 = A.per_head(case, name, cond[name])[0] if name in cond else torch.zeros_like(e2)
        for kind, m in large.items():
            # grad_a sums over the heads: every row of that destination
            sel = m.any(1, keepdim=True)[index] if name == 'a' else m[index]
            fin = sel & r2.isfinite() & e2.isfinite()
            print(f'{what} grad {name} {kind}: max err vs fp64 here '
                  f'{float((g2[fin] - e2[fin]).abs().max()) if fin.any() else 0:.3e}, of the '
                  f'reference {float((r2[fin] - e2[fin]).abs().max()) if fin.any() else 0:.3e}, '
                  f'largest cancelled sum {float(c2[fin].max()) if fin.any() else 0:.3e}')
            attempt(assert_sum_close, g2[fin], r2[fin], e2[fin], abs_sum=c2[fin],
                    what=f'{what} grad {name} {kind} vs fp64')
            assert bool(g2[sel & r2.isfinite()].isfinite().all()), (what, name, kind)
            done |= sel & r2.isfinite()
        if close is not None:
            attempt(close, torch.where(done, r2, g2), r2, index, S, f'{what} grad {name}')
            continue
        # the pairs whose reference gradient is finite everywhere: against float64, like the values
        ok = group_all(r2.isfinite(), index, S)[index] & e2.isfinite() & ~done
        em = torch.isin(index, torch.tensor(case.get('edge_masked_dsts', []), dtype=torch.long))
        em = em.view(-1, 1).expand_as(ok)
        attempt(assert_sum_close, g2[ok & ~em], r2[ok & ~em], e2[ok & ~em],
                what=f'{what} grad {name} vs fp64')
        if bool((ok & em).any()):   # a[:, 0] = -1e30 reaches every head of these rows: ~1e29
            attempt(assert_close_scaled, g2[ok & em], e2[ok & em].float(), tol=2e-5,
                    what=f'{what} grad {name}, destinations masked by the edge term')
        attempt(check_backward, torch.where(done | ok, r2, g2), r2, index, S,
                f'{what} grad {name}')
    assert not failures, ' | '.join(failures)


def judge_isolation(case, got, clean, what):
    keep = ~case['special']                                    # [S, H]
    dst_slot = torch.arange(case['n_dst']).repeat_interleave(case['lens'])
    for n, (a, b) in enumerate(zip(got['outs'], clean['outs'])):
        k = _expand(keep, a)
        assert torch.equal(a[k], b[k]), f'{what}: ordinary rows of out[{n}] moved'
    k = keep[dst_slot]
    assert torch.equal(got['alpha'][k], clean['alpha'][k]), f'{what}: ordinary coefficients moved'
    for name, a in got['grads'].items():
        if name == 'att':
            continue
        b = clean['grads'][name]
        rows = A.rows_to_dst(case, name)
        k = keep.all(1)[rows].unsqueeze(-1).expand_as(a) if name == 'a' else _expand(keep[rows], a)
        assert torch.equal(a[k], b[k]), f'{what}: ordinary rows of grad {name} moved'


def _params():
    out = []
    for fam in A.FAMILIES:
        for lay in (A.EDGE_LAYOUTS if fam == 'edge' else A.LAYOUTS):
            out.append(pytest.param(fam, lay, id=f'{fam}-{"x".join(map(str, lay))}'))
    return out


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('family,layout', _params())
def test_kernels_on_masked_and_nonfinite_scores(dev, family, layout, index_dtype):
    """Every autograd node of the family, forward and backward, under the three rules of the
    module docstring; every run is judged, also behind one that fails."""
    case, refs = _case(family, layout)
    failures = []
    for run in RUNS[family]:
        what = f'{family} {layout} {index_dtype} {run}'
        score = run == 'score'
        got, graph = device_run(case, case['T'], run, dev, index_dtype)
        fwd = graph.by_dst()
        A.check_placements(case, fwd.perm, fwd.ptr)            # the slot order the kernel walked
        clean, _ = device_run(case, case['clean'], run, dev, index_dtype)
        for judge, args in ((judge_forward, (refs[score, torch.float32],
                                             refs[score, torch.float64])),
                            (judge_backward, (refs[score, torch.float32],
                                              refs[score, torch.float64])),
                            (judge_isolation, (clean, ))):
            try:
                judge(case, got, *args, what)
            except AssertionError as exc:
                failures.append(f'{judge.__name__}: {str(exc)[:400]}')
    assert not failures, ' || '.join(failures)


# ---- hub rows ---------------------------------------------------------------------------------------
def _scaled_rule(got, ref, index, S, what):
    """``check_backward`` with the long rows' closeness: 2e-5 of the tensor's scale
    (``test_long_rows_match_float64``) instead of 1e-5 per element"""
    index = index.long()
    seg_ok = group_all(ref.isfinite(), index, S)
    ok = seg_ok[index]
    assert_close_scaled(torch.where(ok, got, 0), torch.where(ok, ref, 0), tol=2e-5,
                        what=f'{what} (finite part)')
    missing = ~seg_ok & group_all(got.isfinite(), index, S)
    assert not missing.any(), (f'{what}: {int(missing.sum())} (destination, head) pairs have a '
                               f'non-finite reference gradient and a finite one here: '
                               f'{missing.nonzero()[:4].tolist()}')


HUB_LAYOUTS = {'transformer': (4, 16), 'gatv2': (4, 16), 'edge': (2, 32, 16)}


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('family', A.FAMILIES)
def test_hub_rows_with_masked_chunks(dev, monkeypatch, family, index_dtype):
    """Three destinations above the hub threshold, in head H // 2: (a) all of chunk 0 masked, (b)
    a middle chunk, the partial last chunk and slot 0 of another chunk, (c) every slot (the
    reference gives NaN).  The sums have ~1.5 thousand terms: values are judged against float64
    (``assert_sum_close``), gradients at 2e-5 of their scale, as the long rows elsewhere."""
    from pytorch_geometric_amd import _native
    thr, chunk = _native.HUB_THRESHOLD, _native.HUB_CHUNK
    case, refs = _case(family, HUB_LAYOUTS[family], hub=(thr, chunk))
    L = thr + 1 + 2 * chunk
    hubs = [case['kinds'].index(k) for k in ('hub_a', 'hub_b', 'hub_c')]
    assert [int(case['lens'][i]) for i in hubs] == [L] * 3 and 4000 <= case['E'] <= 5000
    dst_slot = torch.arange(case['n_dst']).repeat_interleave(case['lens'])
    failures = []
    for run in RUNS[family]:
        what = f'hub {family} {index_dtype} {run}'
        score = run == 'score'
        sink = []
        monkeypatch.setattr(_native, 'timing_sink', sink)
        got, graph = device_run(case, case['T'], run, dev, index_dtype)
        monkeypatch.setattr(_native, 'timing_sink', None)
        A.check_placements(case, graph.by_dst().perm, graph.by_dst().ptr)
        info = {i['op']: i for i, _, _ in sink if i.get('kind') in ('transformer', 'gatv2')}
        by_dst = [i for op, i in info.items() if 'src' not in op]
        assert len(by_dst) == 2, list(info)
        for i in by_dst:    # the chunked schedule ran (GATv2's backward record has no n_chunks)
            assert i['n_hub'] == 3 and i.get('n_chunks', 3 * -(-L // chunk)) == \
                3 * -(-L // chunk), (what, i)
        assert any('n_chunks' in i for i in by_dst), what
        assert all(i['n_hub'] == 0 for op, i in info.items() if 'src' in op), what
        clean, _ = device_run(case, case['clean'], run, dev, index_dtype)
        r32, r64 = refs[score, torch.float32], refs[score, torch.float64]
        try:
            items = [(f'out[{n}]', g, a, b, torch.arange(case['n_dst'])) for n, (g, a, b) in
                     enumerate(zip(got['outs'], r32['outs'], r64['outs']))]
            items.append(('alpha', got['alpha'], r32['alpha'], r64['alpha'], dst_slot))
            for name, g, a, b, dst_of_row in items:
                print(f'{what} {name}: NaN here {int(g.isnan().sum())}, NaN in the reference '
                      f'{int(a.isnan().sum())}')
                off = _kinds_off(case, dst_of_row, g.nan_to_num(nan=7.), a.nan_to_num(nan=7.))
                assert torch.equal(g.isnan(), a.isnan()), f'{what} {name}: NaN pattern ({off})'
                fin = a.isfinite() & b.isfinite()
                assert_sum_close(g[fin], a[fin], b[fin], what=f'{what} {name} vs fp64')
            zero = r32['alpha'] == 0
            assert int(zero.sum()) >= 2 * chunk and bool((got['alpha'][zero] == 0).all()), \
                f'{what}: masked coefficients are not exactly 0'
            c = hubs[2]
            assert bool(got['alpha'][dst_slot == c, case['h']].isnan().all()), what
            judge_backward(case, got, r32, r64, what, close=_scaled_rule)
            judge_isolation(case, got, clean, what)
        except AssertionError as exc:
            failures.append(f'{what}: {str(exc)[:400]}')
    assert not failures, ' || '.join(failures)


# ---- one row, one head ------------------------------------------------------------------------------
TABLE = {  # id -> (scores of the row's slots, expected coefficients)
    '[-inf, 0]': ([-INF, 0.], [0., 1.]),
    '[0, -inf]': ([0., -INF], [1., 0.]),
    '[-inf, -inf]': ([-INF, -INF], [NAN, NAN]),
    '[-inf]': ([-INF], [NAN]),
    '[1, +inf]': ([1., INF], [NAN, NAN]),
    '[1, nan]': ([1., NAN], [NAN, NAN]),
    '[-inf, nan]': ([-INF, NAN], [NAN, NAN]),
    '[+inf, -inf, .25]': ([INF, -INF, .25], [NAN, NAN, NAN]),
    'no slots': ([], []),
}


def table_case(family, scores):
    """Destination 0 is the row of the table: one head of C = 4 channels (an exact scale), one
    source per slot.  Destination 1 has one ordinary edge, so that the kernels run on 'no slots'
    too."""
    g = gen(len(scores))
    n, C, De = len(scores), 4, 3
    E = n + 1
    if family == 'gatv2':
        T = {'x_l': torch.randn(E, 1, C, generator=g), 'x_r': torch.randn(2, 1, C, generator=g),
             'att': torch.tensor([[1., 0., 0., 0.]])}
        T['x_r'][0, 0, 0] = 0.
    else:
        T = {'q': torch.randn(2, 1, C, generator=g), 'k': torch.randn(E, 1, C, generator=g),
             'v': torch.randn(E, 1, C, generator=g)}
        T['q'][0, 0] = torch.tensor([1., 0., 0., 0.])
        if family == 'edge':
            T['b'] = torch.randn(2, 1, De, generator=g)
            T['b'][0] = 0.
            T['a'] = torch.randn(E, De, generator=g)
    for t, s in enumerate(scores):
        T['x_l' if family == 'gatv2' else 'k'][t, 0, 0] = A.carry(s, family, C)[0]
    ei = torch.stack([torch.arange(E), torch.tensor([0] * n + [1])])
    return dict(family=family, H=1, C=C, De=De if family == 'edge' else None, h=0,
                kinds=['row', ''], lens=torch.tensor([n, 1]), ptr=torch.tensor([0, n, E]), ei=ei,
                perm=torch.arange(E), n_dst=2, E=E, T=T, seed=E)


def same(got, want):
    return torch.equal(got.isnan(), want.isnan()) and \
        torch.equal(got.nan_to_num(nan=0.), want.nan_to_num(nan=0.))


@pytest.mark.parametrize('entry', list(TABLE))
def test_table_of_coefficients(dev, entry):
    """One row, one head, the expected coefficients written out: asserted of the float32
    restatement on the CPU (also in tests/test_attention_nonfinite_host.py), then of every autograd
    node; ``out`` follows the restatement (NaN for an all-masked row, 0 without slots)."""
    scores, want = TABLE[entry]
    n = len(scores)
    want = torch.tensor(want).view(-1, 1)
    for family in A.FAMILIES:
        case = table_case(family, scores)
        ref = A.reference(case, False, torch.float32)
        assert same(ref['alpha'][:n], want), (entry, family, 'the restatement', ref['alpha'])
        for run in RUNS[family]:
            what = f'{entry} {family} {run}'
            got, graph = device_run(case, case['T'], run, dev, torch.int64)
            assert torch.equal(graph.by_dst().perm.cpu().long(), case['perm']), what
            assert same(got['alpha'][:n], want), (what, got['alpha'].view(-1).tolist())
            assert_close(got['alpha'], ref['alpha'], what=f'{what} alpha')
            for o, r in zip(got['outs'], ref['outs']):
                assert_close(o, r, what=f'{what} out')
                assert n > 0 or float(o[0].abs().max()) == 0.0, f'{what}: out of the empty row'


# ---- the layers end to end ----------------------------------------------------------------------------
def _scaled(got, ref, what):
    assert_close_scaled(got, ref, what=what)


@pytest.mark.parametrize('fuse', [True, False])
@pytest.mark.parametrize('name', A.LAYER_CASES)
def test_layers_with_masked_sources(dev, name, fuse):
    """TransformerConv, TransformerConv(edge_dim, fuse_edge=True), GATv2Conv and a two-edge-type
    HGTConv whose masked sources belong to one edge type, where head 1's score of every 7th source
    overflows to -inf through the weights (``test_gat_conv_with_masked_sources`` for the newer
    layers): those edges get coefficient exactly 0, every output and gradient stays finite and
    matches the restatement, which tests/test_attention_nonfinite_host.py pins to the real
    reference's record of these cases.  Gradients that pass through the 1e30 weight, and the
    weights' column that multiplies the 1e10 input, are judged on their own."""
    from pytorch_geometric_amd import nn
    rec = A.load_layer_golden()['cases'][name]
    # on the CPU, before the device is consulted
    ref_out, ref_alpha, ref_grads = A.layer_restatement(name, rec)
    for t in (ref_out.values() if name == 'hgt' else [ref_out]):
        assert bool(t.isfinite().all())
    assert all(bool(g.isfinite().all()) for g in ref_grads.values())
    if name != 'hgt':
        ref_ei = rec['attention'][0]
        src_masked = rec['masked'][ref_ei[0]]
        assert bool(src_masked.any()) and bool((ref_alpha[src_masked, 1] == 0).all())
    if name == 'transformer_edge':   # the node the fused-edge kernels implement says the same
        node_out, node_alpha, node_grads = A.layer_restatement(name, rec, via_node=True)
        assert bool(node_out.isfinite().all()) and bool((node_alpha[src_masked, 1] == 0).all())
        assert all(bool(g.isfinite().all()) for g in node_grads.values())

    layer = getattr(nn, rec['cls'])(**rec['kwargs'])
    assert list(layer.state_dict()) == list(rec['state']), name
    layer.load_state_dict(rec['state'])
    layer = layer.to(dev).eval()
    layer.fuse = fuse
    if name == 'transformer_edge':
        layer.fuse_edge = True
    what = f'{rec["cls"]} ({name}) fuse={fuse}'
    inputs = {k: v.to(dev).requires_grad_(True) for k, v in A.layer_inputs(rec).items()}

    def call(**kw):
        if name == 'hgt':
            return layer(inputs, {et: ei.to(dev) for et, ei in rec['edge_index_dict'].items()})
        if name == 'gatv2':
            return layer(inputs['x'], rec['edge_index'].to(dev), **kw)
        return layer(inputs['x'], rec['edge_index'].to(dev), inputs.get('edge_attr'), **kw)

    out = call()
    params = dict(layer.named_parameters())
    names = list(ref_grads)
    leaves = [inputs[n] if n in inputs else params[n] for n in names]
    if name == 'hgt':
        assert list(out) == list(ref_out)
        outs, heads = list(out.values()), [rec['grad_out'][t].to(dev) for t in out]
        for t in out:
            assert_close(out[t], ref_out[t], what=f'{what} out[{t}]')
    else:
        outs, heads = [out], [rec['grad_out'].to(dev)]
        assert_close(out, ref_out, what=f'{what} out')
    grads = dict(zip(names, torch.autograd.grad(outs, leaves, heads)))
    A.judge_layer_grads(grads, ref_grads, rec['group'], _scaled, assert_close_scaled, what)
    if name != 'hgt':   # the coefficients themselves (the score-mode route when fused)
        out2, (got_ei, alpha) = call(return_attention_weights=True)
        assert torch.equal(got_ei.cpu().long(), ref_ei)
        assert_close(alpha, ref_alpha, what=f'{what} attention weights')
        assert bool((alpha.cpu()[src_masked, 1] == 0).all()), f'{what}: masked coefficients'
        assert_close(out2, ref_out, what=f'{what} out beside the attention weights')
