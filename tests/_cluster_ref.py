"""The float64 restatement of the geometric searches (``fps``, ``knn``, ``radius``) and the checks
that measure a float32 search against it.  Plain torch on the CPU; the float32 inputs are promoted
to float64, where the sums of squared differences are exact to about 2^-52.

Ordering rules (the package's): ``knn`` ascending by (distance, index), ``radius`` strict ``dist2 <
r2`` with ``r2 = float32(r)^2``, ascending index, the first ``cap`` kept; ``fps`` greedy, ties to
the lowest index, a picked point never again.

Bounds — derived, not measured.  A float32 sum of ``F`` squared differences in the difference form
has only positive terms: each difference, each product and each of the ``F - 1`` additions rounds
once, so the relative error is below ``(F + 2) * 2^-24`` and ``TAU = (F + 4) * 2^-23`` holds more
than twice that — the slack that lets a rank-wise comparison (two perturbed values) stay inside
``TAU``.  The cosine distance divides a dot product with cancellation by two norms: ``(2 F + 8) *
2^-23`` ABSOLUTE.
"""
import math
import os

import torch

from tests._util import assert_close_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tau(F: int) -> float:
    return (F + 4) * 2.0 ** -23


def tau_cos(F: int) -> float:
    return (2 * F + 8) * 2.0 ** -23


def batch_of(sizes, dtype=torch.int64):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dtype)


def dist64(xe, yc, cosine=False):
    """``[c, n]`` float64 distances of query rows ``yc`` to candidate rows ``xe``."""
    xe, yc = xe.double().cpu(), yc.double().cpu()
    if cosine:
        dot = yc @ xe.t()
        return 1 - dot / (yc.norm(dim=1)[:, None] * xe.norm(dim=1)[None, :])
    if xe.size(1) <= 8:
        return ((yc[:, None, :] - xe[None, :, :]) ** 2).sum(-1)
    D = torch.zeros(yc.size(0), xe.size(0), dtype=torch.float64)
    for c in range(xe.size(1)):          # wide rows: no [c, n, F] cube
        D += (yc[:, c, None] - xe[None, :, c]) ** 2
    return D


def _examples(sizes_x, sizes_y):
    xb = yb = 0
    for nx, ny in zip(sizes_x, sizes_y):
        yield xb, nx, yb, ny
        xb, yb = xb + nx, yb + ny


def _masked(x, y, xb, nx, yb, ny, cosine, exclude):
    """distances with the excluded candidate at +inf, and the candidate count per query"""
    D = dist64(x[xb:xb + nx], y[yb:yb + ny], cosine)
    cand = torch.full((ny, ), nx, dtype=torch.int64)
    if exclude:
        own = torch.arange(yb, yb + ny) - xb
        hit = (own >= 0) & (own < nx)
        D[torch.arange(ny)[hit], own[hit]] = float('inf')
        cand = cand - hit.long()
    return D, cand


def knn_oracle(x, y, k, sizes_x, sizes_y, cosine=False, exclude=False):
    """``[2, E]``: the query in row 0, its neighbours in row 1, by (distance, index)."""
    rows, cols = [], []
    for xb, nx, yb, ny in _examples(sizes_x, sizes_y):
        if nx == 0 or ny == 0:
            continue
        D, cand = _masked(x, y, xb, nx, yb, ny, cosine, exclude)
        oi = torch.sort(D, dim=1, stable=True).indices
        for i in range(ny):
            c = min(k, int(cand[i]))
            rows.append(torch.full((c, ), yb + i, dtype=torch.int64))
            cols.append(oi[i, :c] + xb)
    if not rows:
        return torch.empty(2, 0, dtype=torch.int64)
    return torch.stack([torch.cat(rows), torch.cat(cols)])


def _per_query(result, M, width):
    """padded ``[M, width]`` table (-1) and counts of a ``[2, E]`` result sorted by query"""
    row, col = result[0].cpu().long(), result[1].cpu().long()
    assert bool((row[1:] >= row[:-1]).all()), 'the result is not sorted by query'
    assert row.numel() == 0 or (int(row.min()) >= 0 and int(row.max()) < M)
    count = torch.bincount(row, minlength=M)
    assert int(count.max()) <= width if M else True, 'a query has more neighbours than allowed'
    pos = torch.arange(row.numel()) - (count.cumsum(0) - count)[row]
    table = torch.full((M, max(width, 1)), -1, dtype=torch.int64)
    table[row, pos] = col
    return table, count


def check_knn(result, x, y, k, sizes_x, sizes_y, cosine=False, exclude=False):
    """Checks a ``[2, E]`` knn result for EVERY query (see the module docstring and the list in
    the function body) and returns the share of decided queries."""
    x, y = x.detach().cpu(), y.detach().cpu()
    M, F = y.size(0), x.size(1)
    table, count = _per_query(result, M, k)
    decided = total = 0
    for xb, nx, yb, ny in _examples(sizes_x, sizes_y):
        if ny == 0:
            continue
        total += ny
        if nx == 0:
            assert int(count[yb:yb + ny].sum()) == 0, 'neighbours from another example'
            decided += ny
            continue
        D, cand = _masked(x, y, xb, nx, yb, ny, cosine, exclude)
        want = cand.clamp(max=k)
        # 2. the count is min(k, candidates)
        assert torch.equal(count[yb:yb + ny], want), 'count != min(k, candidates)'
        kk = min(k, nx)
        got = table[yb:yb + ny, :kk]
        live = torch.arange(kk)[None, :] < want[:, None]
        # 1. in the example, unique, never the query itself
        assert bool(((got >= xb) & (got < xb + nx))[live].all()), 'index outside the example'
        srt = torch.sort(torch.where(live, got, -1 - torch.arange(kk)[None, :]), dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all()), 'an index twice'
        if exclude:
            assert bool((got != torch.arange(yb, yb + ny)[:, None])[live].all()), 'the query itself'
        od, oi = torch.sort(D, dim=1, stable=True)
        pad = torch.full((ny, 1), float('inf'), dtype=torch.float64)
        od1 = torch.cat([od, pad], dim=1)[:, :kk + 1]
        tol = torch.full_like(od1, tau_cos(F)) if cosine else tau(F) * od1
        # 3. rank by rank within the bound of the oracle's distance
        gd = D.gather(1, (got - xb).clamp(min=0))
        off = ((gd - od1[:, :kk]).abs() > tol[:, :kk]) & live
        assert not bool(off.any()), (f'{int(off.sum())} ranks off by up to '
                                     f'{float((gd - od1[:, :kk]).abs()[off].max()):.3e}')
        # 4. decided queries: every gap up to rank k (and to k + 1 when there is one) exceeds
        #    the bound -> exactly the oracle's indices
        pair = torch.arange(kk)[None, :] + 1 < (cand[:, None]).clamp(max=k + 1)
        gap_ok = (od1[:, 1:] - od1[:, :kk]) > tol[:, 1:]
        dec = (gap_ok | ~pair).all(dim=1)
        same = ((got == oi[:, :kk] + xb) | ~live).all(dim=1)
        assert bool(same[dec].all()), f'{int((~same & dec).sum())} decided queries differ'
        decided += int(dec.sum())
    return decided / max(total, 1)


def radius_oracle(x, y, r, sizes_x, sizes_y, cap, exclude=False):
    r2 = float(torch.tensor(float(r), dtype=torch.float32).square())
    rows, cols = [], []
    for xb, nx, yb, ny in _examples(sizes_x, sizes_y):
        if nx == 0 or ny == 0:
            continue
        D, _ = _masked(x, y, xb, nx, yb, ny, False, exclude)
        inside = D < r2
        inside &= inside.cumsum(1) <= cap
        rr, cc = inside.nonzero(as_tuple=True)
        rows.append(rr + yb)
        cols.append(cc + xb)
    if not rows:
        return torch.empty(2, 0, dtype=torch.int64)
    return torch.stack([torch.cat(rows), torch.cat(cols)])


def check_radius(result, x, y, r, sizes_x, sizes_y, cap, exclude=False):
    """Every returned pair within ``r2 (1 + tau)``; every candidate within ``r2 (1 - tau)`` that
    precedes the cap present; ascending indices; at most ``cap``, the first ones.  Returns
    ``(capped queries, empty queries)``."""
    x, y = x.detach().cpu(), y.detach().cpu()
    M, F = y.size(0), x.size(1)
    r2 = float(torch.tensor(float(r), dtype=torch.float32).square())
    table, count = _per_query(result, M, cap)
    capped = empty = 0
    for xb, nx, yb, ny in _examples(sizes_x, sizes_y):
        if ny == 0:
            continue
        if nx == 0:
            assert int(count[yb:yb + ny].sum()) == 0
            empty += ny
            continue
        D, _ = _masked(x, y, xb, nx, yb, ny, False, exclude)
        cnt = count[yb:yb + ny]
        got = table[yb:yb + ny]
        live = torch.arange(got.size(1))[None, :] < cnt[:, None]
        assert bool(((got >= xb) & (got < xb + nx))[live].all()), 'index outside the example'
        both = live[:, 1:] & live[:, :-1]
        assert bool((got[:, 1:] > got[:, :-1])[both].all()), 'indices not ascending'
        member = torch.zeros(ny, nx, dtype=torch.bool)
        qi, si = live.nonzero(as_tuple=True)
        member[qi, got[qi, si] - xb] = True
        assert not bool((member & ~(D < r2 * (1 + tau(F)))).any()), 'a pair beyond r2 (1 + tau)'
        # the sure candidates up to the last returned index (all of them below the cap)
        last = torch.where(cnt >= cap, got.gather(1, (cnt - 1).clamp(min=0)[:, None])[:, 0] - xb,
                           torch.full_like(cnt, nx))
        sure = (D < r2 * (1 - tau(F))) & (torch.arange(nx)[None, :] <= last[:, None])
        assert not bool((sure & ~member).any()), 'a candidate within r2 (1 - tau) is missing'
        capped += int((cnt >= cap).sum())
        empty += int((cnt == 0).sum())
    return capped, empty


def fps_picks(sizes, ratio):
    return [math.ceil(ratio * n) for n in sizes]


def fps_oracle(x, sizes, ratio, starts=None):
    """greedy farthest point sampling in float64; ``starts``: global first picks (default: the
    first row of every example)"""
    x = x.detach().double().cpu()
    out, base = [], 0
    for e, n in enumerate(sizes):
        m = math.ceil(ratio * n)
        if m > 0:
            pts = x[base:base + n]
            md = torch.full((n, ), float('inf'), dtype=torch.float64)
            last = 0 if starts is None else int(starts[e]) - base
            for it in range(m):
                out.append(base + last)
                md = torch.minimum(md, ((pts - pts[last]) ** 2).sum(-1))
                md[last] = -1.0
                last = int((md == md.max()).to(torch.uint8).argmax())
        base += n
    return torch.tensor(out, dtype=torch.int64)


def check_fps(result, x, sizes, ratio, random_start=False):
    """Step by step along the RESULT's own run: (1) the pick's float64 minimum distance is within
    tau of the maximum over the points not picked yet, and no index comes twice; (2) the picks
    equal the greedy oracle's exactly up to the first step whose top-two margin is below tau.
    Returns the number of steps compared exactly."""
    x = x.detach().double().cpu()
    res = result.detach().cpu().long()
    F = x.size(1)
    picks = fps_picks(sizes, ratio)
    assert res.numel() == sum(picks), f'{res.numel()} picks, expected {sum(picks)}'
    exact = base = at = 0
    for n, m in zip(sizes, picks):
        mine = res[at:at + m] - base
        at += m
        if m == 0:
            base += n
            continue
        assert int(mine.min()) >= 0 and int(mine.max()) < n, 'a pick outside its example'
        assert mine.unique().numel() == m, 'an index twice'
        if not random_start:
            assert int(mine[0]) == 0, 'random_start=False starts at row 0 of the example'
        pts = x[base:base + n]
        md = torch.full((n, ), float('inf'), dtype=torch.float64)
        sure = True
        for it in range(m - 1):
            last = int(mine[it])
            md = torch.minimum(md, ((pts - pts[last]) ** 2).sum(-1))
            md[last] = -1.0
            top = float(md.max())
            nxt = int(mine[it + 1])
            assert float(md[nxt]) >= top * (1 - tau(F)), (
                f'step {it + 1}: picked a point at {float(md[nxt]):.6e}, the maximum is {top:.6e}')
            if sure:
                best = int((md == top).to(torch.uint8).argmax())
                rest = md.clone()
                rest[best] = -1.0
                if top - float(rest.max()) <= tau(F) * top:
                    sure = False       # a near-tie: from here on only (1) is checked
                else:
                    assert nxt == best, f'step {it + 1}: pick {nxt}, the oracle picks {best}'
                    exact += 1
        base += n
    return exact


# ---- the golden layer cases ------------------------------------------------------------------------
_G = None


def load_golden():
    global _G
    if _G is None:
        _G = torch.load(os.path.join(ROOT, 'tests', 'golden', 'golden_point_cloud_v1.pt'),
                        weights_only=True)
    return _G


def tol_of(ref_err: float) -> float:
    """twice the reference's own float32 error (another order of summation), at least 2e-5"""
    return max(2e-5, 2.0 * ref_err)


def mlp(n_in, hidden, n_out):
    return torch.nn.Sequential(torch.nn.Linear(n_in, hidden), torch.nn.ReLU(),
                               torch.nn.Linear(hidden, n_out))


def make_layer(case, dynamic=False):
    import pytorch_geometric_amd.nn as pnn
    G = load_golden()
    hidden = G['meta']['hidden']
    if case['kind'] == 'edge_conv':
        net = mlp(2 * G['pos'].size(1), hidden, G['grad_out'].size(1))
        layer = (pnn.DynamicEdgeConv(net, G['meta']['k'], aggr=case['aggr']) if dynamic
                 else pnn.EdgeConv(net, aggr=case['aggr']))
    else:
        n_mid = case['state']['global_nn.0.weight'].size(1)
        layer = pnn.PointNetConv(
            mlp(G['feat'].size(1) + G['pos'].size(1), hidden, n_mid),
            torch.nn.Sequential(torch.nn.Linear(n_mid, G['grad_out_global'].size(1))),
            add_self_loops=case['add_self_loops'], aggr=case['aggr'])
    assert list(layer.state_dict().keys()) == case['keys']
    layer.load_state_dict(case['state'])
    return layer


def check_golden_case(name, device, index_dtype=torch.int64, dynamic=False):
    """forward and every gradient of a golden case at the tolerance of the recorded float32
    error; ``dynamic``: ``DynamicEdgeConv(k)`` on the clouds instead of ``EdgeConv`` on the graph"""
    G = load_golden()
    case = G['cases'][name]
    layer = make_layer(case, dynamic).to(device)
    pos = G['pos'].clone().to(device).requires_grad_(True)
    inputs = {'x': pos}
    if case['kind'] == 'edge_conv':
        if dynamic:
            out = layer(pos, G['batch'].to(device=device, dtype=index_dtype))
        else:
            out = layer(pos, G['edge_index'].to(device=device, dtype=index_dtype))
        out.backward(G['grad_out'].to(device))
    else:
        feat = G['feat'].clone().to(device).requires_grad_(True)
        inputs = {'x': feat, 'pos': pos}
        out = layer(feat, pos, G['edge_index_no_loop'].to(device=device, dtype=index_dtype))
        out.backward(G['grad_out_global'].to(device))
    got = {'out': out}
    got.update({f'grad.{k}': v.grad for k, v in inputs.items()})
    got.update({f'grad_params.{n}': p.grad for n, p in layer.named_parameters()})
    want = {'out': case['out']}
    want.update({f'grad.{k}': v for k, v in case['grad'].items()})
    want.update({f'grad_params.{n}': g for n, g in case['grad_params'].items()})
    assert set(got) == set(want)
    for key in want:
        tol = tol_of(case['ref_err'][key])
        err = float((got[key].detach().double().cpu() - want[key].double()).abs().max())
        print(f'{name} {key}: err {err:.2e} tol {tol:.2e} (scaled)')
        assert_close_scaled(got[key].double(), want[key].double(), tol=tol, what=f'{name} {key}')
    return layer
