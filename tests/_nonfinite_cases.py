"""Layout of the non-finite softmax / logsumexp / extremum cases: shared by
tests/golden/make_golden_nonfinite.py (which runs the real reference on it), the oracle pin in
tests/test_oracle_golden.py and tests/test_gpu_nonfinite.py.

One input per width H: segments of rows, most of them ordinary ``randn``, every third one
"special".  A special segment carries its values in ONE head column (``special_col(H)``); its
other columns are ordinary.  The narrow power-of-two route of csrc/softmax.hip packs ``KSEG_PER``
consecutive segments into one wave (first ``KSEG_KEEP`` passes of 64 / H rows in registers): the
stride of 3 and a per-width shift put the special segments on every in-wave position, the last
special segment sits in the final, partly filled wave and is longer than the register-held part.
"""
INF = float('inf')
NAN = float('nan')

WAVE = 64
KSEG_PER = 4     # csrc/softmax.hip kSegPer
KSEG_KEEP = 2    # csrc/softmax.hip kSegKeep
WIDTHS = (1, 2, 8, 3, 64, 100)
STRIDE = 3       # one special segment, then STRIDE - 1 ordinary ones

# name -> values of the special column (None: built per width, see special_values)
KINDS = (
    ('neginf_1', [-INF]),
    ('neginf_2', [-INF, -INF]),
    ('neginf_70', [-INF] * 70),
    ('masked', [-INF, 0.5, -INF, -1.25, 2.0]),
    ('posinf', [1.0, INF]),
    ('posinf_2', [INF, 0.5, INF]),
    ('posinf_neginf', [INF, -INF, 0.25]),
    ('nan', [0.5, NAN, -1.0, 2.0]),
    ('big_pos', [1e4, 1e4 - 1]),
    ('big_neg', [-1e4, -1e4 + 1]),
    ('span', [3e38, -3e38]),
    ('subnormal', [1e-40, -3e-41, 5e-39]),
    ('zeros', [-0.0, 0.0]),
    ('empty', []),
    ('masked_long', None),
)
# kinds whose values are finite but far from 1: judged against a float64 evaluation
LARGE = ('big_pos', 'big_neg', 'span')


def is_pow2(H):
    return H > 0 and (H & (H - 1)) == 0


def narrow(H):
    return H <= WAVE and is_pow2(H)


def special_col(H):
    return H // 2


def kept_cols(H):
    """Columns the fixture stores (inputs and reference results): all of them up to 3, else the
    special column and its two neighbours.  Every call here is column-wise independent, so the
    other columns of a wide input (``full``) do not enter these results; the tests check them
    against the oracle."""
    c = special_col(H)
    return list(range(H)) if H <= 3 else [c - 1, c, c + 1]


def full(stored, H, cols, seed):
    """[rows, len(cols)] stored columns -> the [rows, H] tensor the calls run on: ordinary
    ``randn`` columns around the stored ones."""
    import torch
    out = torch.randn(stored.size(0), H, generator=torch.Generator().manual_seed(seed)) * 3
    out[:, cols] = stored
    return out


def long_len(H):
    """Rows of 'masked_long': more than the register-held KSEG_KEEP passes of 64 / H rows."""
    return (KSEG_KEEP * WAVE // H if narrow(H) else 2) + 3


def special_values(kind, H):
    vals = dict(KINDS)[kind]
    if vals is None:  # masked_long: -inf on every other row, small finite values between
        vals = [-INF if k % 2 == 0 else 0.25 * ((k % 7) - 3) for k in range(long_len(H))]
    return list(vals)


def layout(H):
    """[(kind or '', length)] per segment."""
    shift = (WIDTHS.index(H) if H in WIDTHS else H) % KSEG_PER
    segs = [('', 1 + (i * 7) % 3) for i in range(shift)]
    for j, (kind, _) in enumerate(KINDS):
        segs.append((kind, len(special_values(kind, H))))
        if j + 1 < len(KINDS):
            segs += [('', 1 + (j * 5 + i) % 3) for i in range(STRIDE - 1)]
    while len(segs) % KSEG_PER == 0:  # the last wave stays partly filled
        segs.insert(len(segs) - 1, ('', 2))
    return segs


def check_layout(H, kinds, ptr):
    """The placement the isolation tests rely on (asserted wherever the fixture is loaded)."""
    S = len(kinds)
    special = [i for i, k in enumerate(kinds) if k]
    assert sorted(kinds[i] for i in special) == sorted(k for k, _ in KINDS)
    assert {i % KSEG_PER for i in special} == set(range(KSEG_PER))
    assert S % KSEG_PER != 0 and special[-1] == S - 1, 'no special segment in a partial last wave'
    lens = [int(ptr[i + 1]) - int(ptr[i]) for i in range(S)]
    if narrow(H):
        assert max(lens[i] for i in special) > KSEG_KEEP * WAVE // H
    assert all(kinds[i + 1] == '' for i in special[:-1]), 'special segments must not touch'


def load():
    import os
    import torch
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                        'golden_nonfinite_v1.pt')
    return torch.load(path, map_location='cpu', weights_only=False)
