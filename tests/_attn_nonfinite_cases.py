"""Layout of the masked / non-finite score cases of the one-pass attention kernels (gatv2.hip,
transformer.hip and its edge variant): shared by tests/test_attention_nonfinite_host.py, which
asserts the layout on the CPU, and tests/test_gpu_attention_nonfinite.py.

Destination rows are segments; every edge has a source node of its own, so one row of ``key``
(transformer) or ``x_l`` (GATv2) sets one score.  Head ``H // 2`` of a special destination carries
that kind's values, one per SLOT of the by-destination order; every other head and every other
destination is ordinary ``randn``.  The score is carried by a one-hot query (transformer: the
special head of the special destination) or a one-hot ``att`` (GATv2: the special head, which all
destinations share), so that the float32 restatement's score is set by that one input: ``carry``
returns the input and the score it gives, which ``check_placements`` asserts bit for bit.

The kinds are those of tests/_nonfinite_cases.py plus the placements the online-softmax recurrence
can tell apart (``EXTRA``).  The recurrence works on groups of U slots, U = 2 or 4 by lane shape
(``SlotsInFlight`` / ``InFlight``): rather than restate the shape choice here, both group sizes
get a kind of their own.

The edges are handed over in shuffled COO order.  The slot order is that of a stable sort by
destination — what ``EdgeIndex.by_dst()`` promises; ``check_placements`` takes the permutation it
is given (the planned one on the CPU, ``graph.by_dst().perm`` on the device) and asserts every
intended score on it."""
import math

import torch
import torch.nn.functional as F

import _nonfinite_cases as NF

INF, NAN = NF.INF, NF.NAN
SLOPE = 0.2
F32_MAX = 3.4028234e38

EXTRA = (
    ('neginf_slot0', [-INF, 0.3, -0.7, 1.1, 0.2, -0.4]),
    ('neginf_group2', [-INF, -INF, 0.3, -0.7, 1.1, 0.2]),           # the whole first group, U = 2
    ('neginf_group4', [-INF, -INF, -INF, -INF, 0.3, -0.7, 1.1]),    # the whole first group, U = 4
    ('neginf_last', [0.3, -0.7, 1.1, 0.2, -INF]),
    ('neginf_but_last', [-INF] * 6 + [0.5]),
    ('ramp_up', [200. * t for t in range(7)]),       # every slot rescales the accumulator to 0
    ('ramp_down', [200. * (6 - t) for t in range(7)]),
)
# the mask comes from the edge term <b, a> (edge variant only): masked slots per kind
EDGE_MASKED = (('edge_masked', 5, (0, 2)), ('edge_group4', 7, (0, 1, 2, 3)))
# finite but far from 1: judged against a float64 evaluation
LARGE = NF.LARGE + ('ramp_up', 'ramp_down')

LAYOUTS = [(1, 8), (3, 5), (4, 16), (8, 32), (4, 128)]       # every lane shape of choose_shape
EDGE_LAYOUTS = [(3, 5, 3), (2, 32, 16)]
FAMILIES = ('transformer', 'gatv2', 'edge')


def kinds_of(family, H):
    out = [(k, NF.special_values(k, H)) for k, _ in NF.KINDS] + [(k, list(v)) for k, v in EXTRA]
    if family == 'edge':
        out += [(k, [NAN] * n) for k, n, _ in EDGE_MASKED]   # (values unused: see build)
    return out


def f32(x):
    return torch.tensor([x], dtype=torch.float32)


def score_of(family, C):
    """float32 [1] input of the special channel -> float32 [1] score, by the expression of the
    restatement of that family."""
    if family == 'transformer':
        return lambda x: x / math.sqrt(C)
    if family == 'edge':
        return lambda x: (1.0 / math.sqrt(C)) * x
    return lambda x: F.leaky_relu(x, SLOPE)


def carry(want, family, C):
    """(input, score): the float32 input for the score ``want`` and the score ``score_of`` gives
    it: ``want`` itself where the scale is exact (C a power of 4, infinities, NaN, zeros), else
    within an ulp of it (not every float32 is a quotient by sqrt(5)).  Where the input would
    overflow (3e38 with C > 1: 3e38 * sqrt(C); -3e38 / slope) the input is +-3e38, the largest
    magnitude that survives."""
    f = score_of(family, C)
    w = f32(want)
    if not bool(w.isfinite()):
        assert bool(f(w).isnan()) if bool(w.isnan()) else bool(f(w) == w)
        return float(w), float(w)
    if family == 'gatv2':
        first = want / SLOPE if want < 0 else want
    else:
        first = want * math.sqrt(C)
    if abs(first) > F32_MAX:
        x = f32(math.copysign(3e38, want))
        return float(x), float(f(x))
    x = f32(first)
    return float(x), float(f(x))


def build(family, H, C, De=None, seed=0, hub=None):
    """One case.  ``hub = (threshold, chunk)``: the hub graph of three long destinations instead
    of the kinds (see ``hub_masks``)."""
    g = torch.Generator().manual_seed(seed)
    h = H // 2
    if hub is None:
        segs = []
        for j, (kind, vals) in enumerate(kinds_of(family, H)):
            segs.append((kind, len(vals)))
            segs += [('', 1 + (j * 5 + i) % 6) for i in range(2)]
        values = dict(kinds_of(family, H))
    else:
        L = hub[0] + 1 + 2 * hub[1]
        segs = [('', 3), ('hub_a', L), ('', 5), ('', 0), ('hub_b', L), ('', 2), ('hub_c', L)]
        segs += [('', 1 + i % 6) for i in range(12)]
        values = {k: [-INF if m else None for m in mask]
                  for k, mask in hub_masks(hub[0], hub[1]).items()}
    kinds = [k for k, _ in segs]
    lens = torch.tensor([n for _, n in segs])
    S, E = len(segs), int(lens.sum())
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])
    dst_sorted = torch.arange(S).repeat_interleave(lens)
    order = torch.randperm(E, generator=g)                    # edges in no particular order
    ei = torch.stack([torch.randperm(E, generator=g), dst_sorted[order]])
    perm = torch.sort(ei[1], stable=True).indices             # slot -> COO position
    slot_src = ei[0][perm]

    T = {}
    if family == 'gatv2':
        T['x_l'] = torch.randn(E, H, C, generator=g)
        T['x_r'] = torch.randn(S, H, C, generator=g)
        T['att'] = torch.randn(H, C, generator=g)
        T['att'][h] = 0.
        T['att'][h, 0] = 1.                                   # one-hot: every destination's head h
        carrier = 'x_l'
    else:
        T['q'] = torch.randn(S, H, C, generator=g)
        T['k'] = torch.randn(E, H, C, generator=g)
        T['v'] = torch.randn(E, H, C, generator=g)
        carrier = 'k'
        if family == 'edge':
            T['b'] = torch.randn(S, H, De, generator=g) / math.sqrt(De)
            T['a'] = torch.randn(E, De, generator=g)          # COO order
    edge_masked = dict((k, m) for k, _, m in EDGE_MASKED)
    special = torch.zeros(S, H, dtype=torch.bool)             # outside the isolation rule
    scores = {}
    for i, kind in enumerate(kinds):
        if not kind:
            continue
        lo, hi = int(ptr[i]), int(ptr[i + 1])
        if kind in edge_masked:
            # b = 0 in the other heads (an exact 0 term); a[:, 0] = 0 on the unmasked slots.  All
            # heads read a, so the whole destination is outside the isolation rule.
            special[i] = True
            T['b'][i] = 0.
            T['b'][i, h, 0] = 1e30
            T['a'][perm[lo:hi], 0] = 0.
            continue
        special[i, h] = True
        if family == 'gatv2':
            T['x_r'][i, h, 0] = 0.
        else:
            T['q'][i, h] = 0.
            T['q'][i, h, 0] = 1.
            if family == 'edge':
                T['b'][i, h] = 0.
    clean = {n: t.clone() for n, t in T.items()}
    for i, kind in enumerate(kinds):
        if not kind:
            continue
        lo = int(ptr[i])
        if kind in edge_masked:
            for t in edge_masked[kind]:
                T['a'][perm[lo + t], 0] = -1e30               # 1e30 * -1e30 overflows: -inf
            scores[i] = [-INF if t in edge_masked[kind] else None for t in range(int(lens[i]))]
            continue
        scores[i] = []
        for t, want in enumerate(values[kind]):
            if want is None:                                  # (hub rows) an ordinary slot
                scores[i].append(None)
                continue
            x, s = carry(want, family, C)
            T[carrier][slot_src[lo + t], h, 0] = x
            scores[i].append(s)
    return dict(family=family, H=H, C=C, De=De, h=h, kinds=kinds, lens=lens, ptr=ptr, ei=ei,
                perm=perm, slot_src=slot_src, n_dst=S, E=E, T=T, clean=clean, special=special,
                scores=scores, seed=seed,
                edge_masked_dsts=[i for i, k in enumerate(kinds) if k in edge_masked])


def hub_masks(threshold, chunk):
    """kind -> [masked?] per slot of a destination with threshold + 1 + 2 * chunk slots"""
    L = threshold + 1 + 2 * chunk
    n_chunks = -(-L // chunk)
    assert n_chunks >= 5 and L % chunk != 0, 'needs a middle chunk and a partial last one'
    mid, other = n_chunks // 2, 1
    a = [t < chunk for t in range(L)]
    b = [t // chunk in (mid, n_chunks - 1) or t == other * chunk for t in range(L)]
    return {'hub_a': a, 'hub_b': b, 'hub_c': [True] * L}


def ref_scores(case, T=None):
    """[E, H] raw scores in COO order, by the expressions of the float32 restatements"""
    T = case['T'] if T is None else T
    src, dst = case['ei'][0], case['ei'][1]
    H, C = case['H'], case['C']
    if case['family'] == 'gatv2':
        pre = T['x_l'][src] + T['x_r'][dst]
        return (T['att'].reshape(1, H, C) * F.leaky_relu(pre, SLOPE)).sum(-1)
    if case['family'] == 'transformer':
        return (T['q'][dst] * T['k'][src]).sum(-1) / math.sqrt(C)
    return (1.0 / math.sqrt(C)) * (T['q'][dst] * T['k'][src]).sum(-1) + \
        (T['b'][dst] * T['a'].unsqueeze(1)).sum(-1)


def check_placements(case, perm, ptr=None):
    """Every intended score sits in its slot of the order ``perm`` (slot -> COO position), bit for
    bit and NaN for NaN; the special head of every other slot is finite."""
    perm = perm.cpu().long()
    if ptr is not None:
        assert torch.equal(ptr.cpu().long(), case['ptr']), 'destination pointer'
    assert torch.equal(case['ei'][1][perm], torch.arange(case['n_dst']).repeat_interleave(
        case['lens'])), 'not a by-destination order'
    s = ref_scores(case)[perm]
    h = case['h']
    for i, want in case['scores'].items():
        lo = int(case['ptr'][i])
        assert len(want) == int(case['lens'][i])
        got = s[lo:lo + len(want), h]
        free = torch.tensor([w is None for w in want], dtype=torch.bool)
        w = torch.tensor([0. if x is None else x for x in want], dtype=torch.float32)
        assert bool(got[free].isfinite().all()), (case['kinds'][i], 'an ordinary slot is not finite')
        got, w = got[~free], w[~free]
        assert torch.equal(got.isnan(), w.isnan()) and \
            torch.equal(got.nan_to_num(nan=0.), w.nan_to_num(nan=0.)), (case['kinds'][i], got, w)
    other = torch.ones_like(s, dtype=torch.bool)
    other[:, h] = ~case['special'][:, h][case['ei'][1][perm]]
    assert bool(s[other].isfinite().all()), 'an ordinary score is not finite'


def large_groups(case):
    """kind -> destination, for the kinds judged against float64"""
    return {k: i for i, k in enumerate(case['kinds']) if k in LARGE}


# ---- the reference runs -----------------------------------------------------------------------------
LEAVES = {'transformer': ('q', 'k', 'v'), 'gatv2': ('x_l', 'x_r', 'att'),
          'edge': ('q', 'k', 'v', 'b', 'a')}
SCORE_LEAVES = {'transformer': ('q', 'k'), 'gatv2': ('x_l', 'x_r', 'att'),
                'edge': ('q', 'k', 'b', 'a')}


def cotangents(case):
    """fixed ``grad_out [S, H, C]``, ``grad_z [S, H, De]`` and ``grad_alpha [E, H]`` (slot order)"""
    g = torch.Generator().manual_seed(case['seed'] + 1)
    S, E, H, C = case['n_dst'], case['E'], case['H'], case['C']
    return {'go': torch.randn(S, H, C, generator=g),
            'gz': torch.randn(S, H, case['De'] or 1, generator=g),
            'ga': torch.randn(E, H, generator=g)}


def reference(case, score, dtype, T=None):
    """The restatements (``_transformer_ref.attend``, ``_gatv2_ref.attend``,
    ``_transformer_edge_ref.attend_edge``) on the CPU in ``dtype``: {'outs': [out (, z)], 'alpha':
    [E, H] in slot order, 'grads': {leaf: gradient}}.  ``score``: the coefficients are the result
    and ``grad_alpha`` the cotangent."""
    import _gatv2_ref as RG
    import _transformer_edge_ref as RE
    import _transformer_ref as RT
    fam = case['family']
    T = case['T'] if T is None else T
    L = {n: T[n].to(dtype).clone().requires_grad_(True) for n in LEAVES[fam]}
    ct = {n: t.to(dtype) for n, t in cotangents(case).items()}
    ei, S = case['ei'], case['n_dst']
    if fam == 'transformer':
        out, alpha = RT.attend(L['q'], L['k'], L['v'], ei, S)
        outs, heads = [out], [ct['go']]
    elif fam == 'gatv2':
        out, alpha = RG.attend(L['x_l'], L['x_r'], L['att'], ei, S, SLOPE)
        outs, heads = [out], [ct['go']]
    else:
        out, z, alpha = RE.attend_edge(L['q'], L['k'], L['v'], L['a'], L['b'], ei, S)
        outs, heads = [out, z], [ct['go'], ct['gz']]
    alpha = alpha[case['perm']]
    if score:
        names = SCORE_LEAVES[fam]
        grads = torch.autograd.grad(alpha, [L[n] for n in names], ct['ga'])
        outs = []
    else:
        names = LEAVES[fam]
        grads = torch.autograd.grad(outs, [L[n] for n in names], heads)
    return {'outs': [o.detach() for o in outs], 'alpha': alpha.detach(),
            'grads': dict(zip(names, [g.detach() for g in grads]))}


def rows_to_dst(case, name):
    """the destination every row of leaf ``name`` (and of its gradient) belongs to; None: shared"""
    if name in ('q', 'x_r', 'b'):
        return torch.arange(case['n_dst'])
    if name in ('k', 'v', 'x_l'):
        out = torch.empty(case['E'], dtype=torch.long)
        out[case['ei'][0]] = case['ei'][1]
        return out
    if name == 'a':
        return case['ei'][1]
    return None


def per_head(case, name, t):
    """a leaf-shaped tensor as ([rows', H'], destination of every row'): one column per head, so
    that a (destination, head) pair is a (group, column) pair.  ``a [E, De]`` is summed over the
    heads: one column."""
    index = rows_to_dst(case, name)
    if name == 'a':
        return t.reshape(-1, 1), index.repeat_interleave(t.size(1))
    inner = t.size(2)
    return t.permute(0, 2, 1).reshape(-1, t.size(1)), index.repeat_interleave(inner)


# ---- the layer-level cases (tests/golden/golden_attn_nonfinite_v1.pt) -------------------------------
LAYER_CASES = ('transformer', 'transformer_edge', 'gatv2', 'hgt')
_GOLDEN = []


def load_layer_golden():
    """The real reference's TransformerConv (with and without ``edge_dim``), GATv2Conv and
    HGTConv where head 1's score of every 7th source overflows to -inf through the weights
    (tests/golden/make_golden_attn_nonfinite.py); loaded once and never modified."""
    import os
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_attn_nonfinite_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def layer_inputs(rec):
    """name -> float input tensor, in the order of ``rec['grad_inputs']``"""
    if 'x_dict' in rec:
        return dict(rec['x_dict'])
    out = {'x': rec['x']}
    if rec.get('edge_attr') is not None:
        out['edge_attr'] = rec['edge_attr']
    return out


def layer_restatement(name, rec, via_node=False):
    """The project's restatement of the layer on the recorded inputs and state dict, float32 on the
    CPU: (out, alpha in the recorded edge order | None, {input / parameter: gradient}).
    ``via_node`` (transformer_edge): through ``_transformer_edge_ref.attend_edge``, the node the
    fused-edge kernels implement, instead of ``_transformer_ref.conv``."""
    import _gatv2_ref as RG
    import _hgt_ref as RH
    import _transformer_edge_ref as RE
    import _transformer_ref as RT
    x = {k: v.clone().requires_grad_(True) for k, v in layer_inputs(rec).items()}
    p = {k: v.clone().requires_grad_(True) for k, v in rec['state'].items()}
    kw = {k: v for k, v in rec['kwargs'].items() if k != 'in_channels'}
    alpha = None
    if name == 'hgt':
        out = RH.conv(x, rec['edge_index_dict'], p, **kw)
        outs, heads = [out[t] for t in rec['out']], [rec['grad_out'][t] for t in rec['out']]
    else:
        ei = rec['edge_index']
        if name == 'gatv2':
            out, used, alpha = RG.conv(x['x'], ei, p, **kw)
            assert torch.equal(used, rec['attention'][0]), 'edge list with self-loops'
        elif via_node:
            H, C = kw['heads'], kw['out_channels']
            lin = lambda n: x['x'] @ p[f'{n}.weight'].t() + p[f'{n}.bias']  # noqa: E731
            q, k, v = [lin(n).view(-1, H, C) for n in ('lin_query', 'lin_key', 'lin_value')]
            w3 = p['lin_edge.weight'].view(H, C, -1)
            b = torch.einsum('nhc,hcd->nhd', q, w3) * (1.0 / math.sqrt(C))
            o, z, alpha = RE.attend_edge(q, k, v, x['edge_attr'], b, ei, q.size(0))
            out = (o + torch.einsum('nhd,hcd->nhc', z, w3)).reshape(-1, H * C) + lin('lin_skip')
        else:
            out, alpha = RT.conv(x['x'], ei, p, edge_attr=x.get('edge_attr'), **kw)
        outs, heads = [out], [rec['grad_out']]
    names = list(x) + list(rec['grad_params'])
    leaves = list(x.values()) + [p[n] for n in rec['grad_params']]
    grads = torch.autograd.grad(outs, leaves, heads)
    out = {t: o.detach() for t, o in out.items()} if name == 'hgt' else out.detach()
    return out, None if alpha is None else alpha.detach(), dict(zip(names, grads))


def layer_reference_grads(rec):
    return {**rec['grad_inputs'], **rec['grad_params']}


def judge_layer_grads(got, ref, group, close, close_scaled, what):
    """Gradients of a layer-level case against ``ref`` (name -> tensor), by the groups the record
    stores per tensor: 0 (of order 1): ``close`` per tensor; 1 (the weights' column 0, ~1e10):
    ``close_scaled`` per tensor, on its own; 2 (behind the 1e30 weight, ~1e29 and, where the
    softmax's sum of d s cancels, rounding noise of that size): ``close_scaled`` on all of them
    together; 3 (such noise times the 1e10 input): finite."""
    assert set(got) == set(ref), (what, set(got) ^ set(ref))
    big_got, big_ref = [], []
    for name, r in ref.items():
        g, grp = got[name].detach().cpu(), group[name]
        assert g.shape == r.shape, (what, name)
        close(g[grp == 0], r[grp == 0], f'{what} grad {name}')
        if bool((grp == 1).any()):
            close_scaled(g[grp == 1], r[grp == 1], what=f'{what} grad {name}, column 0')
        assert bool(g[grp == 3].isfinite().all()), f'{what} grad {name}'
        big_got.append(g[grp == 2])
        big_ref.append(r[grp == 2])
    close_scaled(torch.cat(big_got), torch.cat(big_ref),
                 what=f'{what} gradients behind the 1e30 weight')
