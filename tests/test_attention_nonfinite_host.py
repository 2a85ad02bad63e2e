"""Masked and non-finite attention scores, everything that needs no device: the layout of the cases
the GPU tests run (tests/_attn_nonfinite_cases.py: slot placements, intended scores, "the
reference is finite where claimed"), the table of one-row answers, and the pin that entitles
tests/test_gpu_attention_nonfinite.py to use the project's restatements as the reference on such
inputs: ``_transformer_ref.conv``, ``_gatv2_ref.conv``, ``_hgt_ref.conv`` and
``_transformer_edge_ref.attend_edge`` against the real reference's record
(tests/golden/golden_attn_nonfinite_v1.pt)."""
import os

import pytest
import torch

import _attn_nonfinite_cases as A
import _nonfinite_cases as NF
from _util import assert_close, assert_close_scaled
from test_gpu_nonfinite import check_backward

INF, NAN = float('inf'), float('nan')


def _params():
    out = []
    for fam in A.FAMILIES:
        for lay in (A.EDGE_LAYOUTS if fam == 'edge' else A.LAYOUTS):
            out.append(pytest.param(fam, lay, id=f'{fam}-{"x".join(map(str, lay))}'))
    return out


def _neg_inf_slots(case, kind):
    i = case['kinds'].index(kind)
    return [t for t, s in enumerate(case['scores'][i]) if s == -INF], int(case['lens'][i])


@pytest.mark.parametrize('family,layout', _params())
def test_case_layout(family, layout):
    case = A.build(family, *layout, seed=5)
    H, C = layout[:2]
    A.check_placements(case, case['perm'], case['ptr'])
    assert 50 <= case['n_dst'] <= 80 and 200 <= case['E'] <= 500
    assert not torch.equal(case['perm'], torch.arange(case['E'])), 'the COO order is shuffled'
    assert case['h'] == H // 2
    want = [k for k, _ in NF.KINDS] + [k for k, _ in A.EXTRA]
    if family == 'edge':
        want += [k for k, _, _ in A.EDGE_MASKED]
    assert [k for k in case['kinds'] if k] == want
    assert all(not case['kinds'][i + 1] for i, k in enumerate(case['kinds'][:-1]) if k), \
        'special destinations must not touch'
    # the placements the recurrence can tell apart, for groups of 2 and of 4 slots
    assert _neg_inf_slots(case, 'neginf_slot0') == ([0], 6)
    assert _neg_inf_slots(case, 'neginf_group2') == ([0, 1], 6)
    assert _neg_inf_slots(case, 'neginf_group4') == ([0, 1, 2, 3], 7)
    assert _neg_inf_slots(case, 'neginf_last') == ([4], 5)
    assert _neg_inf_slots(case, 'neginf_but_last') == (list(range(6)), 7)
    up = case['scores'][case['kinds'].index('ramp_up')]
    down = case['scores'][case['kinds'].index('ramp_down')]
    assert all(b - a > 199 for a, b in zip(up, up[1:])) and down == up[::-1]
    if family == 'edge':
        assert _neg_inf_slots(case, 'edge_masked') == ([0, 2], 5)
        assert _neg_inf_slots(case, 'edge_group4') == ([0, 1, 2, 3], 7)
        assert not bool(case['T']['a'].isinf().any() | case['T']['a'].isnan().any())
    # exact where the scale is exact; 3e38 survives only for C = 1
    masked = case['scores'][case['kinds'].index('masked')]
    big = case['scores'][case['kinds'].index('big_pos')]
    if C in (1, 4, 16, 64) or family == 'gatv2':
        assert masked == [-INF, 0.5, -INF, -1.25, 2.0] and big == [1e4, 1e4 - 1]
    else:
        assert masked[0] == masked[2] == -INF and abs(masked[4] - 2.0) < 1e-6
    span = case['scores'][case['kinds'].index('span')]
    assert span[0] > 1e37 and span[1] < -1e37
    # the restatement: finite wherever nothing special was put; a masked edge gets exactly 0
    for score in (False, True):
        ref = A.reference(case, score, torch.float32)
        dst_slot = torch.arange(case['n_dst']).repeat_interleave(case['lens'])
        keep = ~case['special']
        assert bool(ref['alpha'][keep[dst_slot]].isfinite().all())
        for o in ref['outs']:
            assert bool(o[keep].isfinite().all())
        for kind in ('masked', 'masked_long', 'neginf_slot0', 'neginf_group2', 'neginf_group4',
                     'neginf_last', 'neginf_but_last') + \
                (('edge_masked', 'edge_group4') if family == 'edge' else ()):
            i = case['kinds'].index(kind)
            lo = int(case['ptr'][i])
            a = ref['alpha'][lo:lo + int(case['lens'][i]), case['h']]
            m = torch.tensor([s == -INF for s in case['scores'][i]])
            assert bool((a[m] == 0).all()) and bool((a[~m] > 0).all()), kind
            assert abs(float(a.sum()) - 1) < 1e-5, kind
        for kind in ('neginf_1', 'neginf_2', 'neginf_70', 'posinf', 'posinf_2', 'posinf_neginf',
                     'nan'):
            i = case['kinds'].index(kind)
            lo = int(case['ptr'][i])
            assert bool(ref['alpha'][lo:lo + int(case['lens'][i]), case['h']].isnan().all()), kind


@pytest.mark.parametrize('family', A.FAMILIES)
def test_hub_case_layout(family):
    from pytorch_geometric_amd import _native
    thr, chunk = _native.HUB_THRESHOLD, _native.HUB_CHUNK
    lay = {'transformer': (4, 16), 'gatv2': (4, 16), 'edge': (2, 32, 16)}[family]
    case = A.build(family, *lay, seed=6, hub=(thr, chunk))
    A.check_placements(case, case['perm'], case['ptr'])
    L = thr + 1 + 2 * chunk
    assert 4000 <= case['E'] <= 5000 and lay[0] * lay[1] <= 64
    masks = A.hub_masks(thr, chunk)
    n_chunks = -(-L // chunk)
    per_chunk = lambda m: [sum(m[c * chunk:(c + 1) * chunk]) for c in range(n_chunks)]  # noqa: E731
    assert per_chunk(masks['hub_a']) == [chunk] + [0] * (n_chunks - 1)
    b = per_chunk(masks['hub_b'])
    assert b[n_chunks // 2] == chunk and b[-1] == L - (n_chunks - 1) * chunk and b[1] == 1 \
        and masks['hub_b'][chunk] and sum(b) == chunk + b[-1] + 1
    assert all(masks['hub_c']) and len(masks['hub_c']) == L
    for kind in masks:
        assert int(case['lens'][case['kinds'].index(kind)]) == L > thr


def test_table_of_coefficients_of_the_restatements():
    """the CPU half of ``test_gpu_attention_nonfinite.test_table_of_coefficients``"""
    import test_gpu_attention_nonfinite as G
    assert len(G.TABLE) == 9
    for entry, (scores, want) in G.TABLE.items():
        want = torch.tensor(want).view(-1, 1)
        for family in A.FAMILIES:
            case = G.table_case(family, scores)
            A.check_placements(dict(case, special=torch.tensor([[True], [False]]),
                                    scores={0: [A.carry(s, family, 4)[1] for s in scores]}),
                               case['perm'], case['ptr'])
            ref = A.reference(case, False, torch.float32)
            assert G.same(ref['alpha'][:len(scores)], want), (entry, family, ref['alpha'])
            if not scores:
                assert all(float(o[0].abs().max()) == 0.0 for o in ref['outs'])
            if entry == '[-inf, -inf]':   # an all-masked row is NaN in out (and z) as well
                assert all(bool(o[0].isnan().all()) for o in ref['outs'])


# ---- the restatements against the real reference's record ------------------------------------------
def test_layer_golden_file_is_what_the_tests_expect():
    G = A.load_layer_golden()
    assert tuple(G['cases']) == A.LAYER_CASES
    for name, rec in G['cases'].items():
        assert int(rec['masked'].sum()) == 9 and not bool(rec['masked'][0])
        grads = A.layer_reference_grads(rec)
        assert set(rec['group']) == set(grads)
        assert all(bool(g.isfinite().all()) for g in grads.values()), name
        assert any(bool((m == 2).any()) for m in rec['group'].values())
        if name != 'hgt':
            ei, alpha = rec['attention']
            m = rec['masked'][ei[0]]
            assert bool((alpha[m, 1] == 0).all()) and bool((alpha[~m, 1] > 0).any())
            assert bool(rec['out'].isfinite().all())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                        'golden_attn_nonfinite_v1.pt')
    assert os.path.getsize(path) < 2 ** 20


def _close(got, ref, what):
    """the backward rule of tests/test_gpu_nonfinite.py on one group of entries"""
    check_backward(got.reshape(-1, 1), ref.reshape(-1, 1), torch.zeros(got.numel()), 1, what)


@pytest.mark.parametrize('name,via_node', [(n, False) for n in A.LAYER_CASES] +
                         [('transformer_edge', True)])
def test_restatements_match_the_reference_on_masked_scores(name, via_node):
    rec = A.load_layer_golden()['cases'][name]
    out, alpha, grads = A.layer_restatement(name, rec, via_node=via_node)
    what = f'{name}{" via attend_edge" if via_node else ""}'
    if name == 'hgt':
        assert list(out) == list(rec['out'])
        for t in out:
            assert bool(out[t].isfinite().all())
            assert_close(out[t], rec['out'][t], what=f'{what} out[{t}]')
    else:
        assert bool(out.isfinite().all())
        assert_close(out, rec['out'], what=f'{what} out')
        assert_close(alpha, rec['attention'][1], what=f'{what} attention')
        m = rec['masked'][rec['attention'][0][0]]
        assert bool((alpha[m, 1] == 0).all()), 'a masked edge gets exactly 0'
    assert all(bool(g.isfinite().all()) for g in grads.values()), what
    A.judge_layer_grads(grads, A.layer_reference_grads(rec), rec['group'], _close,
                        assert_close_scaled, what)
