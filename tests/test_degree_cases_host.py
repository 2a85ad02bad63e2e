"""The degree-profile case of the row-length sweep (tests/_degree_cases.py) on the CPU: the graph
has the degrees and placements it promises, the plan the device must produce is what the degrees
say, every operator's float32 restatement stays within HALF the sweep's per-row bound of its own
float64 run on this graph (so the kernels keep as much room as the reference uses), the
conditioning the operators' test files rely on holds here too, and the per-row judge catches what
the per-tensor one cannot.  The GPU half is tests/test_gpu_degree_sweep.py."""
import pytest
import torch

import _degree_cases as D
from _util import assert_close_scaled

DEFAULT = (1024, 256)
ALL_SETTINGS = (None, ) + D.SETTINGS


def _setting(setting):
    return setting or D.native_settings()


def _ptr(deg):
    return torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])


# ---- the graph ------------------------------------------------------------------------------------------
def test_profile_lengths_at_the_defaults():
    ordinary, hubs = D.profile(*DEFAULT)
    assert len(ordinary) + len(hubs) == 37 and sum(ordinary) + sum(hubs) == 16125
    assert ordinary[-2:] == [1023, 1024] and hubs == [1025, 1026, 1027, 1279, 1280, 1281, 2048, 2049]
    # both slots-in-flight values and their neighbours, the wave width, the lane strides
    assert {1, 2, 3, 4, 5, 63, 64, 65}.issubset(ordinary)


@pytest.mark.parametrize('setting', ALL_SETTINGS)
def test_graph_has_the_profile_in_both_directions(setting):
    thr, chunk = _setting(setting)
    ei, n, pl = D.build(0, thr, chunk)
    assert ei.dtype == torch.int64 and n == pl['P'] + D.N_BACKGROUND
    ordinary, hubs = D.profile(thr, chunk)
    assert sorted(pl['dst_len'].tolist()) == sorted(ordinary + hubs)
    assert sorted(pl['src_len'].tolist()) == sorted(ordinary + hubs)
    assert ei.size(1) == D.E_BACKGROUND + 2 * sum(ordinary + hubs)
    # handed over in no order: the stable sort is what by_dst() / by_src() promise
    assert not bool((ei[1][1:] >= ei[1][:-1]).all()) and not bool((ei[0][1:] >= ei[0][:-1]).all())
    in_deg, out_deg = D.degrees(ei, n)
    for row, deg, rows, lens, what in ((1, in_deg, pl['dst_rows'], pl['dst_len'], 'by destination'),
                                       (0, out_deg, pl['src_rows'], pl['src_len'], 'by source')):
        order = torch.sort(ei[row], stable=True).indices
        ptr = torch._convert_indices_from_coo_to_csr(ei[row][order], n)
        assert torch.equal(ptr, _ptr(deg))
        D.check_placement(ptr, rows, lens, thr, what, ordinary_background=thr >= 64)
    # neither profile disturbs the other: a profile row's edges all end in the background
    lo, hi = pl['background']
    is_profile = torch.zeros(n, dtype=torch.bool)
    is_profile[pl['dst_rows']] = True
    assert not bool((is_profile[ei[0]] & is_profile[ei[1]]).any())
    assert int(is_profile.sum()) == pl['P'] and not bool(is_profile[lo:hi].any())
    if (thr, chunk) == DEFAULT:
        assert n == 3037 and ei.size(1) == 56250
        assert int(in_deg[lo:hi].max()) <= 29 and int(out_deg[lo:hi].max()) <= 29


@pytest.mark.parametrize('setting', ALL_SETTINGS)
def test_expected_plan(setting):
    thr, chunk = _setting(setting)
    ei, n, pl = D.build(0, thr, chunk)
    for deg in D.degrees(ei, n):
        plan = D.expected_plan(deg, thr, chunk)
        rows = [r for r in range(n) if int(deg[r]) > thr]
        assert plan['hub_rows'].tolist() == rows and plan['n_hub'] == len(rows)
        counts = [-(-int(deg[r]) // chunk) for r in rows]
        assert plan['n_chunks'] == sum(counts) and plan['hub_chunk_ptr'][-1] == sum(counts)
        assert (plan['hub_chunk_ptr'][1:] - plan['hub_chunk_ptr'][:-1]).tolist() == counts
        if (thr, chunk) == DEFAULT:
            assert plan['n_hub'] == 8 and plan['n_chunks'] == 48
        if (thr, chunk) == (9, 5):
            # more hubs than one tile of the chunk scan, with unequal chunk counts; threshold + 1
            # slots are exactly two chunks
            assert plan['n_hub'] > 1024 and len(set(counts)) > 8 and -(-(thr + 1) // chunk) == 2
    ordinary, hubs = D.profile(*DEFAULT)
    assert [-(-h // 256) for h in hubs] == [5, 5, 5, 5, 5, 6, 8, 9]   # exact multiples: 1280, 2048
    assert [h % 256 for h in hubs].count(1) == 3 and [h % 256 for h in hubs].count(0) == 2


# ---- the restatements alone stay inside half the bound -----------------------------------------------
CASES = [(name, case) for name, op in D.OPERATORS.items() for case in op.cases]


@pytest.mark.parametrize('name,case', CASES, ids=[f'{n}-{c}' for n, c in CASES])
def test_float32_restatement_is_within_half_the_bound(name, case):
    """Every operator and layout of the sweep, without the ``ref32`` clause.  Inputs that had to be
    conditioned for this (``Operator.conditioned``): GEN (the file's dyadic grid with x, edge_attr
    and b divided by 4: at the grid's magnitudes the restatement's sequential float32 sums over
    2049 positive terms are off by up to 1.5e-5 of the row's scale), GATv2 (dyadic x_l, x_r: see
    ``test_no_leaky_relu_argument_near_the_kink``) and HAN (pinned seeds).  PNA passes on the
    random-normal inputs of its long-row test.  GINE runs on its dyadic grid: float32 and float64
    agree bit for bit."""
    op = D.OPERATORS[name]
    P = D.problem(op, case)
    want64 = D.reference(op, case, torch.float64)
    want32 = D.reference(op, case, torch.float32)
    measure = {}
    D.judge(op, case, want32, want64, P, tol=D.TOL / 2, measure=measure, rows_only=True)
    assert measure, 'nothing was judged'
    print(name, case, {k: f'{v[0]:.1e} at {v[1]}' for k, v in measure.items()})


@pytest.mark.parametrize('setting', D.SETTINGS)
@pytest.mark.parametrize('name', [n for n, op in D.OPERATORS.items() if op.settings])
def test_float32_restatement_at_the_small_settings(name, setting):
    """the one layout per operator that the sweep runs at (64, 48) and (9, 5): another graph.  (The
    typed SAGE aggregation has no hub plan and does not read the threshold.)"""
    op = D.OPERATORS[name]
    case = op.cases[0]
    P = D.problem(op, case, setting)
    D.judge(op, case, D.reference(op, case, torch.float32, setting),
            D.reference(op, case, torch.float64, setting), P, tol=D.TOL / 2, rows_only=True)


# ---- conditioning ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setting', ALL_SETTINGS)
def test_no_leaky_relu_argument_near_the_kink(setting):
    """GATv2 evaluates LeakyReLU per (edge, head, channel): up to 2.9e7 arguments, which no seed
    keeps 1e-6 * max|arg| from 0 on normal inputs (163 expected inside at (4, 128)), so x_l and x_r
    lie on a dyadic grid whose sums are odd multiples of 1/16.  HAN evaluates it per (edge, head):
    seeds are pinned."""
    cases = D.OPERATORS['gatv2'].cases if setting is None else D.OPERATORS['gatv2'].cases[:1]
    for case in cases:
        P = D.problem(D.OPERATORS['gatv2'], case, setting)
        assert D.leaky_margin(P) >= 1e-3, case
        pre = P['x_l'][P['ei'][0]] + P['x_r'][P['ei'][1]]
        assert torch.equal(pre.double(), P['x_l'].double()[P['ei'][0]] + P['x_r'].double()[P['ei'][1]])
    han = D.OPERATORS['han']
    for case in (han.cases if setting is None else han.cases[:1]):
        P = D.problem(han, case, setting)
        assert P['leaky_margin'] >= 1e-6, (case, P['leaky_margin'])
        if _setting(setting)[1] in (256, 48, 5):
            assert P['seed'] == D.HAN_SEEDS[(case[0], case[1], _setting(setting)[0])]


def test_pna_has_no_ties_and_no_variance_near_zero():
    """Random normal inputs: no two SOURCES tie in a min or max.  (Parallel edges do — a 2049-slot
    row draws its sources from 3000 nodes — where there is no edge term, but their shares of the
    gradient meet again in the one source row.)  The restatement's per-row error is what
    ``test_float32_restatement_is_within_half_the_bound`` holds the pinned seeds to."""
    import test_gpu_pna as M
    for case in D.OPERATORS['pna'].cases:
        P = D.problem(D.OPERATORS['pna'], case)
        if case[1]:
            assert M._max_ties(P) == 1, case
        else:
            assert M._max_ties(dict(P, ei=torch.unique(P['ei'], dim=1))) == 1, case


def test_dyadic_sums_stay_exact_at_2049_slots():
    """GINE is judged with ``torch.equal``: ``_dyadic`` asserts the 2^24 bound from the graph's
    largest in- and out-degree, which here is the 2049-slot row; float32 == float64 bit for bit."""
    import test_gpu_gine as M
    op = D.OPERATORS['gine']
    assert op.exact
    for case in op.cases:
        P = D.problem(op, case)
        assert int(P['in_deg'].max()) == 2049 and int(P['out_deg'].max()) == 2049
        e_max = 2 + 1 / 16 if case[1] == 0 else case[1] + 1 + 1 / 16
        assert (2049 * (2 + e_max) + 2.5) * 32 < 2 ** 24 and 2049 * 2 * 8 < 2 ** 24
        want64, want32 = D.reference(op, case, torch.float64), D.reference(op, case, torch.float32)
        for name in M.NAMES:
            if want64[name] is not None:
                assert torch.equal(want64[name], want32[name]), (case, name)


# ---- the judge is sensitive ----------------------------------------------------------------------------
def _sum_case():
    ei, n, pl = D.build(0, *DEFAULT)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, 64, generator=g)
    in_deg, _ = D.degrees(ei, n)
    order = torch.sort(ei[1], stable=True).indices
    src, dst = ei[0][order], ei[1][order]                        # slot order
    slot = torch.arange(dst.numel()) - _ptr(in_deg)[dst]         # position inside the row
    return x, src, dst, slot, in_deg, n


def _sum(x, src, dst, n, keep=None):
    if keep is not None:
        src, dst = src[keep], dst[keep]
    return torch.zeros(n, x.size(1), dtype=x.dtype).index_add_(0, dst, x[src])


def test_judge_catches_a_dropped_tail_slot():
    x, src, dst, slot, in_deg, n = _sum_case()
    want = _sum(x.double(), src, dst, n)
    rows = torch.arange(n)
    D.assert_rows_close(_sum(x, src, dst, n), want, rows, in_deg)            # the honest sum passes
    last_of_1_mod_4 = (in_deg[dst] % 4 == 1) & (slot == in_deg[dst] - 1)
    with pytest.raises(AssertionError) as e:
        D.assert_rows_close(_sum(x, src, dst, n, ~last_of_1_mod_4), want, rows, in_deg, what='tail')
    text = str(e.value)
    named = [int(t) for t in text.split('each: ')[1].replace(',', ' ').split() if t.isdigit()]
    lengths = [L for L in named if L % 4 == 1]
    assert 'destination' in text and {1, 5, 9, 17, 33, 65, 129, 257, 513, 1025, 1281, 2049} \
        .issubset(lengths), text
    assert all(int(in_deg[r]) % 4 == 1 for r in range(n) if f'(row {r}:' in text)


def test_judge_catches_a_dropped_last_chunk():
    x, src, dst, slot, in_deg, n = _sum_case()
    want = _sum(x.double(), src, dst, n)
    thr, chunk = DEFAULT
    hub = in_deg[dst] > thr
    last_chunk = hub & (slot // chunk == (in_deg[dst] - 1) // chunk)
    with pytest.raises(AssertionError) as e:
        D.assert_rows_close(_sum(x, src, dst, n, ~last_chunk), want, torch.arange(n), in_deg,
                            what='chunk', side='source')
    text = str(e.value)
    assert 'source' in text and text.startswith('chunk: 8 of 3037')
    for L in D.profile(*DEFAULT)[1]:
        assert f'{L} (row' in text, (L, text)     # 1025 and 2049: a last chunk of ONE slot


def test_judge_catches_four_ulp_in_the_one_slot_row_and_the_tensor_judge_does_not():
    x, src, dst, slot, in_deg, n = _sum_case()
    want = _sum(x.double(), src, dst, n)
    got = _sum(x, src, dst, n)
    """4 ulp of the tensor's largest sum (a 2049-slot row: 4 * 2^-16 = 6.1e-5) is rounding noise at
    the scale the per-tensor judge divides by, 3.8e-7 of it, and 2e-5 to 6e-5 of a 1-slot row."""
    one = int(torch.nonzero(in_deg == 1)[0])
    top = want.abs().max().float()
    assert int(in_deg[one]) == 1 and 128 <= float(top) < 256
    ulp = float(torch.nextafter(top, torch.tensor(float('inf'))) - top)
    assert ulp == 2.0 ** -16 and float(want[one].abs().max()) < 4 * ulp / 2e-5 / 1.05
    noisy = got.clone()
    noisy[one, 0] += 4 * ulp
    assert_close_scaled(noisy, want.float(), tol=2e-5, what='per tensor')
    with pytest.raises(AssertionError) as e:
        D.assert_rows_close(noisy, want, torch.arange(n), in_deg, what='noise')
    text = str(e.value)
    assert text.startswith('noise: 1 of 3037 destination rows') and 'each: 1 (row' in text, text


def test_judge_rules():
    lengths = torch.tensor([3, 1])
    rows = torch.tensor([0, 0, 1])
    ref = torch.tensor([[100.0], [1.0], [0.5]], dtype=torch.float64)
    ok = ref.clone()
    ok[1] += 1e-3                           # row 0: its own scale is 100
    ok[2] += 1e-5                           # row 1: the scale is max(1, 0.5) = 1
    D.assert_rows_close(ok.float(), ref, rows, lengths)
    bad = ref.clone()
    bad[2] += 1e-4
    with pytest.raises(AssertionError, match=r'1 of 2 destination rows'):
        D.assert_rows_close(bad.float(), ref, rows, lengths)
    # the ref32 clause: twice the float32 restatement's own error on that row
    ref32 = ref.clone()
    ref32[2] += 6e-5
    D.assert_rows_close(bad.float(), ref, rows, lengths, ref32=ref32)
    ref32[2] = ref[2] + 4e-5
    with pytest.raises(AssertionError):
        D.assert_rows_close(bad.float(), ref, rows, lengths, ref32=ref32)
    # non-finite where the reference is finite never passes, whatever ref32 says
    nan = ref.clone().float()
    nan[0] = float('nan')
    with pytest.raises(AssertionError, match='3 \\(row 0: inf'):
        D.assert_rows_close(nan, ref, rows, lengths, ref32=nan)
    assert D.worst_ratio(bad.float(), ref, rows, lengths)[1] == 1
