"""The degree-profile graph and the per-row judge of the row-length sweep: shared by
tests/test_degree_cases_host.py, which asserts the layout and the judge on the CPU, and
tests/test_gpu_degree_sweep.py, which runs every row-walking kernel on it.

Every one-pass operator walks a CSR row (or one chunk of a long one) with one wave, ``U`` slots at
a time (U = 2 or 4), lane-strided where a head takes several lanes, and splits rows of more than
``HUB_THRESHOLD`` slots into ``HUB_CHUNK``-slot chunks that are merged in chunk order; the backward
does the same by source.  ``profile`` lists the 37 row lengths at which any of this can go wrong;
``build`` makes a graph whose in-degrees AND out-degrees both take exactly these lengths, in
pinned placements, on top of a uniform background.

Node layout (``n = P + background``, P = 37).  In BOTH sorted orders a hub has to be row 0 of the
handle and also the highest-numbered row that has any slot, so a profile block can neither be
contiguous nor differ between the two directions: the profile rows are the nodes ``0 .. P-2`` and
``n-1`` with the background between them, and node ``i`` of them has the in-degree ``dst_len[i]``
and the out-degree ``src_len[i]``, two independent shuffles of the profile.  Profile rows draw
their sources from the background and send to the background only, so neither profile disturbs
the other.

The judge, ``assert_rows_close``, measures every row (destination, source, or the destination of
an edge) against its own magnitude, so that a 2049-slot row does not set the scale for a 1-slot
one."""
import torch

ORDINARY = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256,
            257, 511, 512, 513)
TOL = 2e-5                      # the project's figure for the one-pass kernels, here per row
N_BACKGROUND, E_BACKGROUND = 3000, 24000
SETTINGS = ((64, 48), (9, 5))   # the small (threshold, chunk) pairs of the sweep


def native_settings():
    from pytorch_geometric_amd import _native
    return _native.HUB_THRESHOLD, _native.HUB_CHUNK


def profile(thr=None, chunk=None):
    """(ordinary lengths, hub lengths) at a threshold and chunk (default: the package's)"""
    if thr is None:
        thr, chunk = native_settings()
    ordinary = list(ORDINARY) + [thr - 1, thr]
    hubs = [thr + 1, thr + 2, thr + 3, thr + chunk - 1, thr + chunk, thr + chunk + 1, 2 * thr,
            2 * thr + 1]
    return ordinary, hubs


def _placed(g, ordinary, hubs):
    """The profile in its row order: a hub first, a hub last, 'hub, hub, 0' somewhere between, the
    rest shuffled."""
    hubs = [hubs[i] for i in torch.randperm(len(hubs), generator=g).tolist()]
    first, last, pair, free = hubs[0], hubs[1], hubs[2:4], hubs[4:]
    rest = [x for x in ordinary if x != 0] + free
    rest = [rest[i] for i in torch.randperm(len(rest), generator=g).tolist()]
    at = int(torch.randint(0, len(rest) + 1, (1, ), generator=g))
    return [first] + rest[:at] + pair + [0] + rest[at:] + [last]


_BUILT = {}


def build(seed=0, thr=None, chunk=None):
    """``(edge_index [2, E] int64 in shuffled COO order, n, placement)``.  ``placement``: 'dst_rows'
    / 'src_rows' (node ids of the profile rows, ascending), 'dst_len' / 'src_len' (their lengths
    in that order), 'P', 'background' (first, end) and the (thr, chunk) the profile was made for.
    Built once per argument set and never modified."""
    if thr is None:
        thr, chunk = native_settings()
    key = (seed, thr, chunk)
    if key in _BUILT:
        return _BUILT[key]
    g = torch.Generator().manual_seed(seed)
    ordinary, hubs = profile(thr, chunk)
    P = len(ordinary) + len(hubs)
    n = P + N_BACKGROUND
    lo, hi = P - 1, n - 1                                        # the background nodes
    dst_rows = src_rows = list(range(0, P - 1)) + [n - 1]
    dst_len, src_len = _placed(g, ordinary, hubs), _placed(g, ordinary, hubs)

    def bg(k):
        return torch.randint(lo, hi, (k, ), generator=g)

    src = [bg(E_BACKGROUND)] + [bg(L) for L in dst_len] + \
        [torch.full((L, ), r) for r, L in zip(src_rows, src_len)]
    dst = [bg(E_BACKGROUND)] + [torch.full((L, ), r) for r, L in zip(dst_rows, dst_len)] + \
        [bg(L) for L in src_len]
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    ei = ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()
    placement = {'P': P, 'dst_rows': torch.tensor(dst_rows), 'src_rows': torch.tensor(src_rows),
                 'dst_len': torch.tensor(dst_len), 'src_len': torch.tensor(src_len),
                 'background': (lo, hi), 'thr': thr, 'chunk': chunk}
    _BUILT[key] = (ei, n, placement)
    return _BUILT[key]


def degrees(ei, n):
    """(in-degree, out-degree) of every node"""
    return torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)


def check_placement(ptr, rows, lens, thr, what, ordinary_background=True):
    """The pinned placements on a row pointer ``ptr`` (by destination or by source) whose profile
    rows are ``rows`` with the lengths ``lens``; ``ordinary_background``: every other row stays
    below the threshold (not so at a threshold of 9, where most background rows are hubs)."""
    ptr = ptr.cpu().long()
    deg = ptr[1:] - ptr[:-1]
    assert torch.equal(deg[rows], lens), f'{what}: the profile rows do not have the profile lengths'
    hub = deg > thr
    with_slots = torch.nonzero(deg > 0).flatten()
    assert bool(hub[0]), f'{what}: row 0 is not a hub'
    assert bool(hub[with_slots[-1]]), f'{what}: the last row that has a slot is not a hub'
    pair = torch.nonzero(hub[:-2] & hub[1:-1] & (deg[2:] == 0)).flatten()
    assert pair.numel() >= 1, f'{what}: no two adjacent hubs followed by an empty row'
    if ordinary_background:
        others = torch.ones_like(hub)
        others[rows] = False
        assert int(deg[others].max()) < thr, f'{what}: a background row reaches the threshold'


def expected_plan(deg, thr, chunk):
    """The hub plan of rows with the lengths ``deg`` on the CPU: hub rows (more than ``thr`` slots)
    in ascending order, the exclusive scan of their chunk counts with the total appended."""
    deg = deg.cpu().long()
    rows = torch.nonzero(deg > thr).flatten()
    counts = (deg[rows] + chunk - 1) // chunk
    cptr = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])
    return {'hub_rows': rows, 'hub_chunk_ptr': cptr, 'n_hub': int(rows.numel()),
            'n_chunks': int(counts.sum())}


# ---- the judge -------------------------------------------------------------------------------------
def row_errors(got, ref64, row_of, n_rows):
    """(err, scale) per row: the largest |got - ref64| and max(1, largest |ref64|) over the
    elements whose leading index belongs to the row; rows without an element: (0, 1).  A non-finite
    ``got`` where the reference is finite gives an infinite error."""
    got = got.detach().cpu().double()
    ref64 = ref64.detach().cpu().double()
    assert got.shape == ref64.shape, f'shape {tuple(got.shape)} vs {tuple(ref64.shape)}'
    assert bool(torch.isfinite(ref64).all()), 'the float64 evaluation is not finite'
    lead = got.size(0)
    assert row_of.numel() == lead, 'one group per leading index'
    d = (got - ref64).abs().nan_to_num(nan=float('inf'), posinf=float('inf')).reshape(lead, -1)
    m = ref64.abs().reshape(lead, -1)
    d = d.max(1).values if d.size(1) else torch.zeros(lead, dtype=torch.float64)
    m = m.max(1).values if m.size(1) else torch.zeros(lead, dtype=torch.float64)
    row_of = row_of.cpu().long()
    err = torch.zeros(n_rows, dtype=torch.float64).scatter_reduce(0, row_of, d, 'amax')
    scale = torch.ones(n_rows, dtype=torch.float64).scatter_reduce(0, row_of, m, 'amax')
    return err, scale


def worst_ratio(got, ref64, row_of, lengths):
    """(largest err / scale over the rows, the length of the row that has it)"""
    err, scale = row_errors(got, ref64, row_of, lengths.numel())
    ratio = err / scale
    i = int(ratio.argmax()) if ratio.numel() else 0
    return (float(ratio[i]), int(lengths[i])) if ratio.numel() else (0.0, 0)


def assert_rows_close(got, ref64, row_of, lengths, tol=TOL, ref32=None, what='', side='destination'):
    """Every row of ``got`` within ``tol * max(1, max |ref64|)`` of ``ref64``, error and magnitude
    taken over that row alone.  ``row_of [leading size]``: the row every leading index belongs to;
    ``lengths [rows]``: the slots of every row (for the message).  With ``ref32`` (the float32
    restatement) a row also passes at twice that restatement's own error on the row — the rule of
    ``_util.assert_sum_close``.  A non-finite value where the reference is finite never passes."""
    n_rows = lengths.numel()
    err, scale = row_errors(got, ref64, row_of, n_rows)
    bound = tol * scale
    if ref32 is not None:
        err32, _ = row_errors(ref32, ref64, row_of, n_rows)
        bound = torch.maximum(bound, 2 * err32)
    bad = torch.nonzero(~((err <= bound) & torch.isfinite(err))).flatten()
    if bad.numel():
        ratio = err / scale
        by_len = {}
        for r in bad.tolist():
            L = int(lengths[r])
            if L not in by_len or float(ratio[r]) > by_len[L][1]:
                by_len[L] = (r, float(ratio[r]))
        shown = ', '.join(f'{L} (row {r}: {q:.2e})' for L, (r, q) in sorted(by_len.items())[:24])
        raise AssertionError(
            f'{what}: {bad.numel()} of {n_rows} {side} rows off at {tol:g} of their own scale; '
            f'lengths of the failing {side} rows with the worst err / scale at each: {shown}')


# ---- the operators -----------------------------------------------------------------------------------
# One entry per row-walking operator: its cases (layouts and variants), the problem on the profile
# graph (built by the operator's own test module), the restatement in a dtype on the CPU and the run
# through the autograd node on the device, both as {name: tensor | None}, and for every name the
# side its leading index belongs to: 'dst', 'src', 'edge' (an [E, ...] tensor in COO order, grouped
# by the edge's destination) or None (a parameter gradient: no row structure).  The typed operators
# name further sides of their stacked graphs and map them in ``group``.
class Operator:
    kind = None           # 'kind' of the launch records
    exact = False         # dyadic inputs: judged with torch.equal, float32 == float64
    conditioned = ''      # what was done to the inputs so that the restatement is well conditioned
    settings = True       # the kernels read the hub threshold and chunk

    def group(self, P, side):
        return group_of(P, side)

    def plan_degrees(self, P):
        """(slots of every row of the by-destination handle, of the by-source handle)"""
        return P['in_deg'], P['out_deg']

    def key(self, case):
        """the part of a case that sets the problem (variants of one problem share it)"""
        return case

    def judge_global(self, name, got, want, P, case):
        from _util import assert_close_scaled
        assert_close_scaled(got, want.float(), tol=TOL, what=f'{self.name} {case} {name}')


class _Gatv2(Operator):
    name, kind = 'gatv2', 'gatv2'
    cases = [(3, 5, ''), (4, 16, ''), (4, 128, ''), (4, 16, 'score')]
    sides = {'out': 'dst', 'alpha': 'edge', 'grad_x_l': 'src', 'grad_x_r': 'dst', 'grad_att': None}
    conditioned = ('x_l = round(8 randn) / 8 + 1/16 and x_r = round(8 randn) / 8: every LeakyReLU '
                   'argument is an odd multiple of 1/16 (no seed keeps up to 2.9e7 normal arguments '
                   'from the kink)')

    def key(self, case):
        return case[:2]

    def problem(self, key, ei, n, placement):
        import test_gpu_gatv2 as M
        P = M._problem(n, n, ei, key[0], key[1], 100 + key[0] * key[1])
        P['x_l'] = (P['x_l'] * 8).round() / 8 + 1 / 16
        P['x_r'] = (P['x_r'] * 8).round() / 8
        return P

    def reference(self, P, case, dtype):
        import test_gpu_gatv2 as M
        return dict(zip(self.sides, M._reference(P, dtype)))

    def device(self, P, case, dev, index_dtype):
        import test_gpu_gatv2 as M
        got, graph = M._device_run(P, dev, index_dtype, score=case[2] == 'score')
        return dict(zip(self.sides, got)), graph


def leaky_margin(P):
    """smallest |argument| of GATv2's LeakyReLU over the largest"""
    pre = (P['x_l'][P['ei'][0]] + P['x_r'][P['ei'][1]]).abs()
    return float(pre.min() / pre.max())


class _Transformer(Operator):
    name, kind = 'transformer', 'transformer'
    cases = [(3, 5, ''), (4, 16, ''), (4, 128, ''), (4, 16, 'packed'), (4, 16, 'score')]
    sides = {'out': 'dst', 'alpha': 'edge', 'grad_query': 'dst', 'grad_key': 'src',
             'grad_value': 'src'}

    def key(self, case):
        return case[:2]

    def problem(self, key, ei, n, placement):
        import test_gpu_transformer as M
        return M._problem(n, n, ei, key[0], key[1], 100 + key[0] * key[1])

    def reference(self, P, case, dtype):
        import test_gpu_transformer as M
        return dict(zip(self.sides, M._reference(P, dtype)))

    def device(self, P, case, dev, index_dtype):
        import test_gpu_transformer as M
        got, graph = M._device_run(P, dev, index_dtype, score=case[2] == 'score',
                                   packed=case[2] == 'packed')
        return dict(zip(self.sides, got)), graph


class _TransformerEdge(Operator):
    name, kind = 'transformer_edge', 'transformer'
    cases = [(3, 5, 3), (2, 32, 16)]
    sides = {'out_nodes': 'dst', 'z': 'dst', 'alpha': 'edge', 'grad_query': 'dst',
             'grad_key': 'src', 'grad_value': 'src', 'grad_b': 'dst', 'grad_edge_attr': 'edge'}

    def problem(self, key, ei, n, placement):
        import test_gpu_transformer_edge as M
        return M._problem(n, n, ei, *key, 200 + key[0] * key[1] + key[2])

    def reference(self, P, case, dtype):
        import test_gpu_transformer_edge as M
        return dict(zip(self.sides, M._reference(P, dtype)))

    def device(self, P, case, dev, index_dtype):
        import test_gpu_transformer_edge as M
        got, graph = M._device_run(P, dev, index_dtype)
        return dict(zip(self.sides, got)), graph


class _Gine(Operator):
    name, kind, exact = 'gine', 'gine', True
    cases = [(5, 0), (64, 0), (5, 3), (64, 3)]          # De = 0: the wide mode; De = 3: linear
    sides = {'out': 'dst', 'grad_x_src': 'src', 'grad_x_root': 'dst', 'grad_eps': None,
             'grad_edge_attr': 'edge', 'grad_W': None, 'grad_b': None}

    def problem(self, key, ei, n, placement):
        import test_gpu_gine as M
        return M._dyadic(n, n, ei, key[0], key[1], 300 + key[0] + 7 * key[1])

    def reference(self, P, case, dtype):
        import test_gpu_gine as M
        return dict(zip(self.sides, M._reference(P, dtype=dtype)))

    def device(self, P, case, dev, index_dtype):
        import test_gpu_gine as M
        got, graph = M._device_run(P, dev, index_dtype)
        return dict(zip(self.sides, got)), graph

    def judge_global(self, name, got, want, P, case):
        assert torch.equal(got.cpu(), want.float()), f'gine {case} {name} is not exact'


class _Pna(Operator):
    name, kind = 'pna', 'pna'
    cases = [(5, 0), (64, 0), (5, 3), (64, 3)]
    sides = {'mean': 'dst', 'min': 'dst', 'max': 'dst', 'std': 'dst', 'grad_p_src': 'src',
             'grad_p_dst': 'dst', 'grad_edge_attr': 'edge', 'grad_Wc': None}

    # var = mean(x^2) - mean(x)^2 cancels where the few slots of a short row lie close together, and
    # the gradient of std carries that error: seeds at which the float32 restatement stays below
    # 5e-6 per row ((64, 0): 8.7e-6, the best of twenty), by (W, De, threshold)
    SEEDS = {(5, 0, 1024): 402, (64, 0, 1024): 403, (5, 3, 1024): 400, (64, 3, 1024): 404,
             (5, 0, 64): 416, (5, 0, 9): 419}
    conditioned = 'seeds pinned in _Pna.SEEDS (std near cancellation in short rows)'

    def problem(self, key, ei, n, placement):
        import test_gpu_pna as M
        seed = self.SEEDS.get((key[0], key[1], placement['thr']), 400 + key[0] + 7 * key[1])
        return M._random(n, n, ei, key[0], key[1], seed)

    @staticmethod
    def _flat(res):
        import test_gpu_pna as M
        out = dict(zip(M.FOUR, res['out']))
        out.update({k: res[k] for k in M.GRADS})
        return out

    def reference(self, P, case, dtype):
        import test_gpu_pna as M
        return self._flat(M._reference(P, M.FOUR, dtype))

    def device(self, P, case, dev, index_dtype):
        import test_gpu_pna as M
        got, graph = M._device_run(P, dev, M.FOUR, index_dtype)
        return self._flat(got), graph


class _Gen(Operator):
    name, kind = 'gen', 'gen'
    cases = [(F, De, t) for F in (5, 64) for De in (0, 3) for t in ('1', 'learn')]
    sides = {'out': 'dst', 'grad_x_src': 'src', 'grad_edge_attr': 'edge', 'grad_W': None,
             'grad_b': None, 'grad_t': None}
    conditioned = ("the file's dyadic grid, on which no ReLU argument is zero or inexact, with x, "
                   "edge_attr and b divided by 4: at the grid's own magnitudes the float32 "
                   "restatement's sequential sums over 2049 positive terms are off by 1.0e-5 to "
                   "1.5e-5 of the row's scale (out, t = 1 and t learned), above half the bound")

    def key(self, case):
        return case[:2]

    def problem(self, key, ei, n, placement):
        import test_gpu_gen as M
        P = M._problem(n, n, ei, key[0], key[1], 300 + key[0] + 7 * key[1])
        for k in ('x', 'a', 'b'):          # a power of two: still exact, still never zero
            if P[k] is not None:
                P[k] = P[k] / 4
        return P

    def reference(self, P, case, dtype, device='cpu'):
        import test_gpu_gen as M
        return dict(zip(self.sides, M._reference(P, *M._t(case[2], case[0]), dtype=dtype,
                                                 device=device)))

    def device(self, P, case, dev, index_dtype):
        import test_gpu_gen as M
        got, graph = M._device_run(P, dev, *M._t(case[2], case[0]), index_dtype=index_dtype)
        return dict(zip(self.sides, got)), graph

    def judge_global(self, name, got, want, P, case):
        import test_gpu_gen as M
        if name != 'grad_t':
            return Operator.judge_global(self, name, got, want, P, case)
        t = M._t(case[2], case[0])[0]
        M._check([None] * 5 + [got], [None] * 5 + [want], P, t, f'gen {case}')


class _ResGated(Operator):
    name, kind = 'resgated', 'resgated'
    cases = [(5, 0), (132, 0), (5, 3), (132, 3)]
    sides = {'out': 'dst', 'grad_k': 'dst', 'grad_q': 'src', 'grad_v': 'src',
             'grad_edge_attr': 'edge', 'grad_Wg': None, 'grad_Wv': None}

    def problem(self, key, ei, n, placement):
        import test_gpu_resgated as M
        return M._problem(n, n, ei, key[0], key[1], 300 + key[0] + 7 * key[1])

    def reference(self, P, case, dtype, device='cpu'):
        import test_gpu_resgated as M
        return dict(zip(self.sides, M._reference(P, dtype, device)))

    def device(self, P, case, dev, index_dtype):
        import test_gpu_resgated as M
        got, graph = M._device_run(P, dev, index_dtype)
        return dict(zip(self.sides, got)), graph


class _Mixture(Operator):
    """(F, K, M): F = 64 is one element per lane, F = 256 four; K = 3 and 5 are no powers of two.
    ``out = Z W`` goes through the GEMM, so the row of ``out`` is judged behind it."""
    name, kind = 'mixture', 'mixture'
    cases = [(64, 3, 24), (256, 5, 40)]
    sides = {'out': 'dst', 'grad_x': 'src', 'grad_coef': 'edge', 'grad_weight': None}

    def problem(self, key, ei, n, placement):
        import test_gpu_mixture as M
        return M._problem(n, n, ei, *key, 700 + key[0] + 5 * key[1] + key[2])

    def reference(self, P, case, dtype, device='cpu'):
        import test_gpu_mixture as M
        return dict(zip(self.sides, M._reference(P, dtype, device)))

    def device(self, P, case, dev, index_dtype):
        import test_gpu_mixture as M
        got, graph = M._device_run(P, dev, index_dtype=index_dtype)
        return dict(zip(self.sides, got)), graph

    def judge_global(self, name, got, want, P, case):
        # the rule of test_gpu_mixture._check: 2e-5 of the scale or 4 x the float32 restatement
        err = float((got.detach().cpu().double() - want.double()).abs().max())
        scale = max(float(want.abs().max()), 1.0)
        if not err <= TOL * scale:
            ref32 = self.reference(P, case, torch.float32)[name]
            floor = 4 * float((ref32.double() - want.double()).abs().max())
            assert err <= floor, f'mixture {case} {name}: {err:.3e} vs {max(TOL * scale, floor):.3e}'


# ---- the typed operators: the profile graph is the SECOND edge type; the first is uniform among the
# background nodes, so that the profile's block of stacked rows does not start at row 0 and the
# profile rows keep their exact lengths where a destination's row spans the edge types (HGT)
UNI, PRO = 'uni', 'pro'
E_UNIFORM = 8000


def uniform_background(placement, seed):
    lo, hi = placement['background']
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(lo, hi, (E_UNIFORM, ), generator=g),
                        torch.randint(lo, hi, (E_UNIFORM, ), generator=g)])


# seeds at which every LeakyReLU argument of HAN keeps 1e-6 * max|arg| from 0 (asserted on the CPU)
HAN_SEEDS = {(2, 8, 1024): 12, (2, 8, 64): 12, (2, 8, 9): 13, (4, 128, 1024): 11}   # (H, D, threshold)


class _Han(Operator):
    """relu = False: everything elementwise; 'relu': the fused ReLU under one mask for both sides
    (the device's on the device, the float64 run's on the host)."""
    name, kind = 'han', 'han'
    cases = [(2, 8, ''), (4, 128, ''), (2, 8, 'relu')]
    sides = {'out': 'dst', 'alpha': 'edge', 'grad_x': 'node', 'grad_a_src': 'src',
             'grad_a_dst': 'dst'}
    conditioned = 'seeds pinned in HAN_SEEDS (LeakyReLU arguments away from the kink)'

    def key(self, case):
        return case[:2]

    def problem(self, key, ei, n, placement):
        import test_gpu_han as M
        thr, chunk = placement['thr'], placement['chunk']
        seed = HAN_SEEDS.get((key[0], key[1], thr), 11)
        ets = [(('a', UNI, 'a'), 0), (('a', PRO, 'a'), 0)]
        uni = uniform_background(placement, 5)
        for seed in range(seed, seed + 50):   # (the pinned seed holds at the default chunk; with
            # another PYGAMD_HUB_CHUNK the profile, and so the graph, is another one)
            P = M._typed_problem(key[0], key[1], seed, sizes={'a': n}, edges=ets, ei=[uni, ei])
            if P['leaky_margin'] >= 1e-6:
                break
        P['seed'] = seed
        P['out_deg_pro'] = torch.bincount(ei[0], minlength=n)
        return P

    def reference(self, P, case, dtype, mask=None):
        import test_gpu_han as M
        relu = case[2] == 'relu'
        if relu and mask is None:
            mask = M._reference(P, True)[0] > 0
        res = M._reference(P, relu, mask=mask, dtype=dtype)
        return dict(zip(self.sides, [r.detach() for r in res]))

    def device(self, P, case, dev, index_dtype):
        import test_gpu_han as M
        Q = dict(P, ei=[e.to(index_dtype) for e in P['ei']])
        res = M._device(Q, dev, case[2] == 'relu')
        graph = res[-1]
        alpha = torch.empty_like(res[1])
        alpha[graph.by_dst().perm.long()] = res[1]
        return dict(zip(self.sides, (res[0], alpha) + tuple(res[2:5]))), graph

    def plan_degrees(self, P):
        st = P['st']
        return (torch.bincount(P['row'], minlength=st.num_rows),
                torch.bincount(P['col'], minlength=st.num_cols))

    def group(self, P, side):
        by_dst, by_src = self.plan_degrees(P)
        if side == 'dst':
            return torch.arange(by_dst.numel()), by_dst, 'stacked destination'
        if side == 'src':
            return torch.arange(by_src.numel()), by_src, 'stacked source'
        if side == 'node':
            return torch.arange(P['n']), P['out_deg_pro'], 'source (profile edge type)'
        return P['row'], by_dst, 'stacked destination (of the edge)'


class _Hgt(Operator):
    """The whole layer (relation transform, the attention node on the stacked graph, GELU, output
    projection, skip) with separate source and destination node types, so that grad_x['s'] is a
    by-source quantity and grad_x['d'] a by-destination one."""
    name, kind = 'hgt', 'transformer'
    cases = [(2, 8)]
    sides = {'out': 'dst', 'grad_x_s': 'src', 'grad_x_d': 'dst'}
    ETS = [('s', UNI, 'd'), ('s', PRO, 'd')]

    def kwargs(self, key):
        return dict(in_channels={'s': 12, 'd': key[0] * key[1]}, out_channels=key[0] * key[1],
                    metadata=(['s', 'd'], self.ETS), heads=key[0])

    def layer(self, key):
        from pytorch_geometric_amd.nn import HGTConv
        torch.manual_seed(3)
        layer = HGTConv(**self.kwargs(key))
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for p in list(layer.skip.values()) + list(layer.p_rel.values()):
                p.copy_(torch.randn(p.shape, generator=g))
        return layer

    def problem(self, key, ei, n, placement):
        g = torch.Generator().manual_seed(31)
        W = key[0] * key[1]
        uni = uniform_background(placement, 6)
        return {'key': key, 'x': {'s': torch.randn(n, 12, generator=g),
                                  'd': torch.randn(n, W, generator=g)},
                'go': torch.randn(n, W, generator=g), 'ei': dict(zip(self.ETS, [uni, ei])),
                'state': {k: v.detach().clone() for k, v in self.layer(key).state_dict().items()},
                'deg': [degrees(uni, n), degrees(ei, n)]}

    def reference(self, P, case, dtype):
        import _hgt_ref as R
        p = {k: v.to(dtype).requires_grad_(True) for k, v in P['state'].items()}
        x = {t: v.to(dtype).requires_grad_(True) for t, v in P['x'].items()}
        out = R.conv(x, P['ei'], p, **self.kwargs(P['key']))['d']
        grads = torch.autograd.grad((out * P['go'].to(dtype)).sum(), list(x.values()) +
                                    list(p.values()), allow_unused=True)
        res = {'out': out.detach(), 'grad_x_s': grads[0], 'grad_x_d': grads[1]}
        res.update({f'param {k}': g for k, g in zip(p, grads[2:])})
        return res

    def device(self, P, case, dev, index_dtype):
        from pytorch_geometric_amd import _hgt
        layer = self.layer(P['key'])
        layer.load_state_dict(P['state'])
        layer = layer.to(dev)
        x = {t: v.to(dev).requires_grad_(True) for t, v in P['x'].items()}
        ei = {et: e.to(dev).to(index_dtype) for et, e in P['ei'].items()}
        out = layer(x, ei)['d']
        params = dict(layer.named_parameters())
        grads = torch.autograd.grad((out * P['go'].to(dev)).sum(), list(x.values()) +
                                    list(params.values()), allow_unused=True)
        res = {'out': out.detach(), 'grad_x_s': grads[0], 'grad_x_d': grads[1]}
        res.update({f'param {k}': g for k, g in zip(params, grads[2:])})
        n = P['n']
        st = _hgt.Stacking({'s': n, 'd': n}, self.ETS)
        return res, _hgt.stacked_graph(st, [ei[et] for et in self.ETS])

    def plan_degrees(self, P):
        (in_u, out_u), (in_p, out_p) = P['deg']
        return torch.cat([torch.zeros_like(in_u), in_u + in_p]), torch.cat([out_u, out_p])

    def group(self, P, side):
        (in_u, out_u), (in_p, out_p) = P['deg']
        rows = torch.arange(P['n'])
        if side == 'dst':
            return rows, in_u + in_p, 'destination'
        return rows, out_u + out_p, 'source'


class _TypedSage(Operator):
    """The typed aggregation kernels themselves (csrc/hetero_conv.hip): one wave walks a row of
    any length, there is no hub plan, no launch record and nothing the small thresholds change.
    Fw = 16: uniform type summed, profile type averaged; Fw = 100: the other way round."""
    name, kind, settings = 'typed_sage', None, False
    cases = [(16, ), (100, )]
    sides = {'out_uni': 'dst_uni', 'out_pro': 'dst', 'grad_x': 'src'}
    ETS = [('a', UNI, 'a'), ('a', PRO, 'a')]

    def problem(self, key, ei, n, placement):
        g = torch.Generator().manual_seed(60 + key[0])
        uni = uniform_background(placement, 7)
        return {'Fw': key[0], 'x': torch.randn(n, key[0], generator=g),
                'go': [torch.randn(n, key[0], generator=g) for _ in range(2)],
                'eis': [uni, ei], 'means': [key[0] != 16, key[0] == 16],
                'deg': [degrees(uni, n), degrees(ei, n)]}

    def reference(self, P, case, dtype):
        import _hetero_conv_ref as R
        x = P['x'].to(dtype).requires_grad_(True)
        aggs = [R.aggregate(x, e, P['n'], 'mean' if m else 'sum')
                for e, m in zip(P['eis'], P['means'])]
        total = sum((a * g.to(dtype)).sum() for a, g in zip(aggs, P['go']))
        return {'out_uni': aggs[0].detach(), 'out_pro': aggs[1].detach(),
                'grad_x': torch.autograd.grad(total, x)[0]}

    def device(self, P, case, dev, index_dtype):
        from pytorch_geometric_amd import _native
        from pytorch_geometric_amd._hetero import HeteroGraph
        n, Fw = P['n'], P['Fw']
        eis = [e.to(index_dtype).to(dev) for e in P['eis']]
        h = HeteroGraph(self.ETS, eis, [n, n], [n, n])
        x = P['x'].to(dev)
        outs = [torch.full((n, Fw), float('nan'), device=dev) for _ in range(2)]
        _native.hetero_spmm(h.rowptr, h.col, h.row_begin, [x, x], outs, P['means'])
        rowptr_t, col_t = h.transposed()
        assert h.src_types == ['a']
        gx = [torch.full((n, Fw), float('nan'), device=dev)]
        _native.hetero_spmm_backward(rowptr_t, col_t, h.rowptr, h.row_begin,
                                     [g.to(dev) for g in P['go']], P['means'], h.src_begin, gx)
        return {'out_uni': outs[0], 'out_pro': outs[1], 'grad_x': gx[0]}, h

    def group(self, P, side):
        (in_u, out_u), (in_p, out_p) = P['deg']
        rows = torch.arange(P['n'])
        if side == 'dst_uni':
            return rows, in_u, 'destination (uniform edge type)'
        if side == 'dst':
            return rows, in_p, 'destination'
        return rows, out_u + out_p, 'source'


OPERATORS = {op.name: op for op in (_Gatv2(), _Transformer(), _TransformerEdge(), _Gine(), _Pna(),
                                    _Gen(), _ResGated(), _Mixture(), _Han(), _Hgt(),
                                    _TypedSage())}

_PROBLEMS, _REFS = {}, {}


def problem(op, case, setting=None):
    """The operator's problem at a case on the profile graph of a (threshold, chunk) setting
    (None: the package's); built once, with 'n', 'placement', 'in_deg' and 'out_deg' added."""
    thr, chunk = setting or native_settings()
    k = (op.name, op.key(case), thr, chunk)
    if k not in _PROBLEMS:
        ei, n, placement = build(0, thr, chunk)
        P = op.problem(op.key(case), ei, n, placement)
        P['n'], P['placement'], P['profile_ei'] = n, placement, ei
        P['in_deg'], P['out_deg'] = degrees(ei, n)
        _PROBLEMS[k] = P
    return _PROBLEMS[k]


def reference(op, case, dtype, setting=None):
    """The restatement's results on that problem in ``dtype`` on the CPU; computed once."""
    thr, chunk = setting or native_settings()
    variant = case if op.name in ('gen', 'han') else op.key(case)   # variants of the reference
    k = (op.name, variant, thr, chunk, dtype)
    if k not in _REFS:
        _REFS[k] = op.reference(problem(op, case, setting), case, dtype)
    return _REFS[k]


def group_of(P, side):
    """(row of every leading index, slots of every row, the side's name) of a side"""
    rows = torch.arange(P['n'])
    if side == 'dst':
        return rows, P['in_deg'], 'destination'
    if side == 'src':
        return rows, P['out_deg'], 'source'
    return P['ei'][1], P['in_deg'], 'destination (of the edge)'


def judge(op, case, got, want64, P, tol=TOL, ref32=None, measure=None, rows_only=False):
    """Every tensor of ``got`` against ``want64``: per row where it has a side, by the operator's
    own rule where it has none.  ``ref32``: a callable that gives the float32 restatement's results,
    asked only when a row misses ``tol``.  ``measure``: a dict that takes name -> (worst err /
    scale, the row length there).  ``rows_only``: leave the tensors without a side out."""
    for name, w in want64.items():
        side = op.sides.get(name)
        if w is None:
            assert got[name] is None or not bool(got[name].any()), \
                f'{op.name} {case}: {name} should be absent'
            continue
        g = got[name]
        assert g is not None, f'{op.name} {case}: {name} is missing'
        w = w.reshape(g.shape)
        if side is None:
            if not rows_only:
                op.judge_global(name, g, w, P, case)
            continue
        row_of, lengths, side_name = op.group(P, side)
        what = f'{op.name} {case} {name}'
        if measure is not None:
            measure[name] = worst_ratio(g, w, row_of, lengths)
        exact = op.exact
        try:
            assert_rows_close(g, w, row_of, lengths, tol=0.0 if exact else tol, what=what,
                              side=side_name)
        except AssertionError:
            if exact or ref32 is None:
                raise
            assert_rows_close(g, w, row_of, lengths, tol=tol, ref32=ref32()[name].reshape(g.shape),
                              what=what, side=side_name)
