"""The backward of every one-pass operator family, written once for its two autograd routes: the
``torch.autograd.Function`` classes of ``_functions.py`` on the cached sorted forms of an
``EdgeIndex`` and the ``torch.ops.pyg_amd.*_backward`` operators of ``ops.py`` on ``(rowptr, col[,
edge_id])``.  A route hands over its :class:`Slots`, flat 2-D tensors and the gradients it wants."""
import functools
import math

import torch

from . import _native


def _rows(t):
    """[n, ...] -> [n, prod(...)] (also for empty tensors, where reshape(n, -1) is ambiguous)."""
    return t.reshape(t.size(0), math.prod(t.shape[1:]))


class _Form:
    """One sorted form given as its tensors; the hub plan is made when it is first read."""

    def __init__(self, ptr, idx, perm=None):
        self.ptr, self.idx, self.perm, self.n_rows = ptr, idx, perm, ptr.numel() - 1

    @functools.cached_property
    def hub(self):
        return _native.hub_plan(self.ptr)


class Slots:
    """The slots of a graph by destination (``fwd``: ``ptr``, ``idx``, ``hub``, ``n_rows``) and,
    built when first asked for, by source.  Each route keeps ITS by-source form: for an edge list
    not sorted by destination the two order the slots of a source differently (last-bit sums)."""

    def __init__(self, fwd, graph=None, n_src=0, edge_id=None):
        self.fwd, self._graph, self._n_src, self._edge_id = fwd, graph, n_src, edge_id

    @classmethod
    def of_graph(cls, graph):  # the cached sorted forms, hub plans and slot map of an EdgeIndex
        return cls(graph.by_dst(), graph=graph)

    @classmethod
    def of_csr(cls, rowptr, col, n_src, edge_id=None):  # edge_id: slot -> edge (None: identity)
        return cls(_Form(rowptr, col), n_src=n_src, edge_id=edge_id)

    @functools.cached_property
    def _sorted(self):
        """The by-source form of a CSR pair: a stable sort of ``col``, whose permutation (``perm``,
        int64) IS the map from by-source slots to the pair's own slots."""
        ptr, col = self.fwd.ptr, self.fwd.idx
        dst = _native.ptr2index(ptr, col.numel())
        src_sorted, perm = _native.index_sort(col, max_value=max(self._n_src - 1, 0))
        return _Form(_native.index2ptr(src_sorted, self._n_src), _native.permute_index(dst, perm),
                     perm)

    def by_src(self):
        """``ptr``, ``idx`` and ``hub`` of the same slots sorted by source"""
        return self._sorted if self._graph is None else self._graph.by_src()

    def slot_map(self):
        """by-source slot -> by-destination slot: where the attention kernels find ``alpha``"""
        if self._graph is not None:
            return self._graph.src_slot_to_dst_slot()
        return _native.cast_index(self._sorted.perm, self.fwd.idx.dtype)

    def edge_id(self):
        """by-destination slot -> the caller's edge (None: the slots are the edges)"""
        return self.fwd.perm if self._graph is not None else self._edge_id

    def edge_id_t(self):
        """by-source slot -> the caller's edge"""
        if self._graph is not None:
            return self._graph.by_src().perm
        if self._edge_id is None:
            return self.slot_map()
        return _native.permute_index(self._edge_id, self._sorted.perm)


def gatv2_backward(slots, x_l, x_r, att, alpha, H, C, slope, *, grad_out=None, out=None,
                   grad_alpha=None, want_x_l=True):
    """``(grad_x_l | None, grad_x_r, grad_att)``, flat: one launch by destination, then one by
    source (grad_x_l).  ``grad_alpha`` given = score mode, otherwise ``grad_out`` and ``out``."""
    fwd = slots.fwd
    grad_s, g_r, g_att = _native.gatv2_backward_dst(
        fwd.ptr, fwd.idx, x_l, x_r, att, alpha, H, C, slope, grad_out=grad_out, out=out,
        grad_alpha=grad_alpha, hub=fwd.hub)
    g_l = None
    if want_x_l:
        bwd = slots.by_src()
        g_l = _native.gatv2_backward_src(bwd.ptr, bwd.idx, slots.slot_map(), x_l, x_r, att, alpha,
                                         grad_s, H, C, slope, grad_out=grad_out,
                                         n_dst=fwd.n_rows, hub=bwd.hub)
    return g_l, g_r, g_att


def han_check_types(types, n_rows, n_cols, n_x):
    """``types = (row_begin [T + 1], src_begin [T + 1], val_shift [T])`` of a stacked HAN call
    (sequences of ints): the row blocks tile the handle's rows, the column blocks its columns, and
    every column block lands inside ``x_all`` — the bounds the kernels rely on."""
    row_begin, src_begin, val_shift = types
    T = len(val_shift)
    ok = (T >= 1 and len(row_begin) == len(src_begin) == T + 1 and row_begin[0] == 0
          and src_begin[0] == 0 and row_begin[-1] == n_rows and src_begin[-1] == n_cols)
    for e in range(T if ok else 0):
        ok = ok and (row_begin[e] <= row_begin[e + 1] and src_begin[e] <= src_begin[e + 1]
                     and src_begin[e] + val_shift[e] >= 0
                     and src_begin[e + 1] + val_shift[e] <= n_x)
    if not ok:
        raise ValueError("'row_begin' / 'src_begin' / 'val_shift' do not describe the stacked "
                         f"graph ({n_rows} rows, {n_cols} columns) over {n_x} feature rows")


def han_backward(slots, types, x_all, a_src, a_dst, alpha, out, grad_out, H, C, slope, relu, *,
                 want_x=True, want_a_src=True):
    """``(grad_x_all | None, grad_a_src | None, grad_a_dst)``, flat: one launch by destination,
    then one by source whose ``[n_cols, H * C]`` blocks are added into the node types' rows of
    ``x_all`` in edge-type order."""
    row_begin, src_begin, val_shift = types
    fwd = slots.fwd
    grad_s, g_dst = _native.han_backward_dst(
        fwd.ptr, fwd.idx, row_begin, val_shift, x_all, a_src, a_dst, alpha, grad_out, out, H, C,
        slope, relu, hub=fwd.hub)
    g_x = g_src = None
    if want_x or want_a_src:
        bwd = slots.by_src()
        g_src, g_xv = _native.han_backward_src(bwd.ptr, bwd.idx, slots.slot_map(), alpha, grad_s,
                                               grad_out, out, H, C, relu, hub=bwd.hub)
        if want_x:
            g_x = torch.zeros_like(x_all)
            for e, shift in enumerate(val_shift):
                lo, hi = src_begin[e], src_begin[e + 1]
                if hi > lo:
                    g_x[lo + shift:hi + shift] += g_xv[lo:hi]
    return g_x, g_src if want_a_src else None, g_dst


def transformer_backward(slots, query, key, value, alpha, H, C, scale, *, grad_out=None, out=None,
                         grad_alpha=None, edge_attr=None, bias=None, grad_z=None, z=None,
                         want_key=True, want_value=True, want_edge_attr=True, packed=False):
    """``(grad_query, grad_key, grad_value, grad_bias, grad_edge_attr)``, flat, None where not
    computed: one launch by destination, then one by source (grad_key and, unless in score mode,
    grad_value; ``packed``: both in one buffer).  ``grad_alpha`` given = score mode.  ``edge_attr``
    (slot order) given = the edge variant: its by-destination launch also returns grad_bias and, if
    wanted, grad_edge_attr in slot order; the by-source launch reads d s and alpha alone."""
    fwd = slots.fwd
    g_b = g_a = None
    if edge_attr is None:
        grad_s, g_q = _native.transformer_backward_dst(
            fwd.ptr, fwd.idx, query, key, value, alpha, H, C, scale, grad_out=grad_out, out=out,
            grad_alpha=grad_alpha, hub=fwd.hub)
    else:
        grad_s, g_q, g_b, g_a = _native.transformer_edge_backward_dst(
            fwd.ptr, fwd.idx, query, key, value, edge_attr, bias, alpha, H, C, scale,
            grad_out=grad_out, out=out, grad_z=grad_z, z=z, grad_alpha=grad_alpha,
            want_grad_edge_attr=want_edge_attr, hub=fwd.hub)
    g_k = g_v = None
    if want_key or (grad_alpha is None and want_value):
        bwd = slots.by_src()
        g_k, g_v = _native.transformer_backward_src(
            bwd.ptr, bwd.idx, slots.slot_map(), query, alpha, grad_s, H, C, scale,
            grad_out=grad_out, n_dst=fwd.n_rows, hub=bwd.hub, packed=packed)
    return g_q, g_k, g_v, g_b, g_a


def gine_backward(slots, x_src, x_root, eps, edge_attr, weight, bias, grad_out, *, want_x_src=True,
                  want_root=True, want_eps=True, want_edge_attr=True, want_weight=True,
                  want_bias=True):
    """``(grad_x_src, grad_x_root, grad_eps, grad_edge_attr, grad_weight, grad_bias)``, None where
    not wanted or not given: one launch by source and the self term elementwise."""
    g_x = g_a = g_w = g_b = g_root = g_eps = None
    if want_x_src or want_edge_attr or want_weight or want_bias:
        bwd = slots.by_src()
        g_x, g_a, g_w, g_b = _native.gine_backward(
            bwd.ptr, bwd.idx, slots.edge_id_t(), x_src, edge_attr, weight, bias, grad_out,
            want_grad_edge_attr=want_edge_attr, hub=bwd.hub)
    if x_root is not None:
        n = slots.fwd.n_rows
        if want_root:
            g_root = grad_out * (1.0 if eps is None else 1.0 + eps.reshape(()))
            if x_root.size(0) != n:  # destinations are a prefix: the rest takes no gradient
                full = grad_out.new_zeros(x_root.shape)
                full[:n] = g_root
                g_root = full
        if eps is not None and want_eps:
            # row sums in fp32, their total in fp64: one rounding of the whole inner product
            g_eps = ((grad_out * x_root[:n]).sum(dim=1).double().sum().to(eps.dtype)
                     .reshape(eps.shape))
    return (g_x if want_x_src else None, g_root, g_eps, g_a if want_edge_attr else None,
            g_w if want_weight else None, g_b if want_bias else None)


def pna_coefficients(saved, deg, stats, grads):
    """The packed coefficient rows ``[n_dst, 6, W]`` (A, B, Gmin, Gmax, min u, max u) the backward
    kernel of csrc/pna.hip reads, from the forward's saved planes, the degrees ``deg [n_dst]`` and
    the incoming gradients of ``stats`` (None: zero).  Per slot the kernel forms ``grad_u = A +
    B u + Gmin [u == min u] + Gmax [u == max u]``: ``B = g_std / (d std)`` (0 where std was
    masked), ``A = g_mean / d - B mean_u``, ``Gmin = g_min / cnt_min`` (an even split among
    ties, as ``scatter_reduce``), ``Gmax`` alike; all 0 for ``d = 0``."""
    mean_u, min_u, max_u, std, cnt_min, cnt_max = saved.unbind(0)
    g = dict(zip(stats, grads))
    d = deg.to(torch.float32).view(-1, 1)
    has = d > 0
    zero = torch.zeros_like(mean_u)
    B = zero
    if g.get('std') is not None:
        B = torch.where(std > 0, g['std'] / (d * std), zero)
    A = -B * mean_u
    if g.get('mean') is not None:
        A = A + torch.where(has, g['mean'] / d.clamp(min=1), zero)
    Gmin = zero if g.get('min') is None else torch.where(has, g['min'] / cnt_min, zero)
    Gmax = zero if g.get('max') is None else torch.where(has, g['max'] / cnt_max, zero)
    return torch.stack([A, B, Gmin, Gmax, min_u, max_u], dim=1)


def pna_backward(slots, p_src, edge_attr, wc, saved, stats, grads, dst_rows, *, want_src=True,
                 want_dst=True, want_edge_attr=True, want_wc=True):
    """``(grad_p_src, grad_p_dst [dst_rows, W], grad_edge_attr, grad_wc)``, None where not wanted
    or not given: :func:`pna_coefficients` of ``grads`` (one per statistic of ``stats``) and one
    launch by source.  ``p_dst`` takes the gradients of every statistic but std, added in the order
    of ``stats``: the caller's on the handle route, the kernel's on the operator route, as ever."""
    ptr = slots.fwd.ptr
    deg = ptr[1:] - ptr[:-1]
    g_src = g_dst = g_a = g_wc = None
    if want_src or want_edge_attr or want_wc:
        coef = pna_coefficients(saved, deg, stats, grads)
        bwd = slots.by_src()
        g_src, g_a, g_wc = _native.pna_backward(
            bwd.ptr, bwd.idx, slots.edge_id_t(), p_src, edge_attr, wc, coef, stats,
            want_grad_edge_attr=want_edge_attr, hub=bwd.hub)
    if want_dst:
        g_dst = saved.new_zeros(dst_rows, saved.size(2))
        parts = [g for s, g in zip(stats, grads) if s != 'std' and g is not None]
        if parts:  # (destinations may be a prefix of p_dst's rows: the rest takes no gradient)
            total = parts[0] if len(parts) == 1 else torch.stack(parts).sum(0)
            g_dst[:slots.fwd.n_rows] = total * (deg > 0).view(-1, 1)
    return (g_src if want_src else None, g_dst, g_a if want_edge_attr else None,
            g_wc if want_wc else None)


def gen_backward(slots, x_src, edge_attr, weight, bias, t, out, saved, grad_out, *, eps_msg=1e-7,
                 semi_grad=False, want_x_src=True, want_edge_attr=True, want_weight=True,
                 want_bias=True, want_t=False):
    """``(grad_x_src, grad_edge_attr, grad_weight, grad_bias, grad_t)``, None where not wanted or
    not given.  An elementwise pre-pass packs one row per destination — the forward's ``M``,
    ``grad_out / (L + 1e-16)`` and, unless ``semi_grad``, ``out`` — and one launch by source
    rebuilds the message and its softmax weight per out-slot.  ``grad_t = sum_i grad_out (S2 -
    out^2)`` needs no per-edge work: column sums in fp64 (the two terms nearly cancel)."""
    g_x = g_a = g_w = g_b = g_t = None
    if want_x_src or want_edge_attr or want_weight or want_bias:
        planes = [saved[0], grad_out * saved[1]] + ([] if semi_grad else [out])
        coef = torch.stack(planes, dim=1)
        bwd = slots.by_src()
        g_x, g_a, g_w, g_b = _native.gen_backward(
            bwd.ptr, bwd.idx, slots.edge_id_t(), x_src, edge_attr, weight, bias, t, coef,
            eps_msg=eps_msg, semi_grad=semi_grad,
            want_grad_edge_attr=want_edge_attr and edge_attr is not None, grad_t=want_t,
            hub=bwd.hub)
    if want_t:
        if saved.size(0) < 3:
            raise ValueError("the gradient of 't' needs the forward's third plane (want_s2)")
        cols = (grad_out * (saved[2] - out * out)).double().sum(dim=0)
        g_t = (cols.sum() if t.numel() == 1 else cols).to(t.dtype).reshape(t.shape)
    return (g_x if want_x_src else None, g_a if want_edge_attr else None,
            g_w if want_weight else None, g_b if want_bias else None, g_t)


def resgated_weight(w_gate, w_value):
    """the kernels' stacked ``[2, F, De]`` edge matrices (None without an edge term)"""
    return None if w_gate is None else torch.stack([w_gate, w_value])


def resgated_backward(slots, k, qv, edge_attr, w_gate, w_value, grad_out, *, want_k=True,
                      want_qv=True, want_edge_attr=True, want_weights=True):
    """``(grad_k, grad_qv, grad_edge_attr, grad_w_gate, grad_w_value)``, None where not wanted or
    not given: one launch by destination (``grad_k`` and everything of the edge term), then one by
    source (the packed ``grad_qv``).  Both recompute the sigmoid from the inputs."""
    fwd = slots.fwd
    weight = resgated_weight(w_gate, w_value)
    g_k = g_qv = g_a = g_w = None
    if want_k or (weight is not None and (want_edge_attr or want_weights)):
        g_k, g_a, g_w = _native.resgated_backward_dst(
            fwd.ptr, fwd.idx, slots.edge_id(), k, qv, edge_attr, weight, grad_out,
            want_grad_edge_attr=want_edge_attr and edge_attr is not None, hub=fwd.hub)
    if want_qv:
        bwd = slots.by_src()
        g_qv = _native.resgated_backward_src(
            bwd.ptr, bwd.idx, None if edge_attr is None else slots.edge_id_t(), k, qv, edge_attr,
            weight, grad_out, hub=bwd.hub)
    give_w = want_weights and g_w is not None
    return (g_k if want_k else None, g_qv, g_a if want_edge_attr else None,
            g_w[0] if give_w else None, g_w[1] if give_w else None)


def cg_weight(w_f, w_s):
    """the kernels' stacked ``[2, F, De]`` edge matrices (None without raw edge features)"""
    return None if w_f is None else torch.stack([w_f, w_s])


def cg_split(p, q):
    """``(P, Q)`` as the kernels read them: two tensors, or (``q`` None) the halves of the packed
    ``p = [P | Q] [N, 4F]`` in place"""
    if q is not None:
        return p, q
    half = p.size(1) // 2
    return p[:, :half], p[:, half:]


def cg_backward(slots, p, q, edge_attr, w_f, w_s, edge_terms, grad_out, *, mean=False,
                want_p=True, want_q=True, want_edge_attr=True, want_weights=True,
                want_edge_terms=True):
    """``(grad_p, grad_q, grad_edge_attr, grad_w_f, grad_w_s, grad_edge_terms)``, None where not
    wanted or not given: one launch by destination (``grad_P`` and everything of the edge term),
    then one by source (``grad_Q``).  Both recompute the sigmoid and the softplus.  With the
    packed ``p = [P | Q]`` (``q`` None) the two launches write the halves of ONE ``[N, 4F]``
    plane, which is ``grad_p``.  The by-destination launch is skipped when none of its outputs
    is wanted."""
    fwd = slots.fwd
    packed = q is None
    P, Q = cg_split(p, q)
    weight = cg_weight(w_f, w_s)
    linear, wide = weight is not None, edge_terms is not None
    edge = edge_terms if wide else (edge_attr if linear else None)
    want_edge = (linear and want_edge_attr) or (wide and want_edge_terms)
    out_p = out_q = g_p = g_q = g_e = g_w = None
    if packed:
        want_q = want_p
        if want_p:
            plane = torch.empty_like(p, memory_format=torch.contiguous_format)
            out_p, out_q = cg_split(plane, None)
            out_p[fwd.n_rows:].zero_()   # (sources that are no destination)
    if want_p or want_edge or (linear and want_weights):
        g_p, g_e, g_w = _native.cg_backward_dst(
            fwd.ptr, fwd.idx, slots.edge_id(), P, Q, edge, weight, grad_out, mean=mean,
            want_grad_edge=want_edge, out=out_p, hub=fwd.hub)
    if want_q:
        bwd = slots.by_src()
        g_q = _native.cg_backward_src(
            bwd.ptr, bwd.idx, None if edge is None else slots.edge_id_t(), P, Q, edge, weight,
            grad_out, dst_rowptr=fwd.ptr if mean else None, out=out_q, hub=bwd.hub)
    if packed:
        g_p, g_q = (plane if want_p else None), None
    give_w = want_weights and g_w is not None
    return (g_p if want_p else None, g_q, g_e if linear and want_edge_attr else None,
            g_w[0] if give_w else None, g_w[1] if give_w else None,
            g_e if wide and want_edge_terms else None)


class _PairForm:
    """The ``(relation, node)`` pair rows of a typed edge list (``RelationalHandle.pair_graph``):
    ``ptr`` over the non-empty pairs, ``idx`` = the other endpoint per slot, ``edge_id`` = slot ->
    edge, ``pair_rel`` / ``pair_node`` = the pair of every row, ``pair_of_slot`` = slot -> row."""

    def __init__(self, node, other, rel, n_node, n_other, R, edge_of=None):
        from .nn.conv.rgcn_conv import RelationalHandle
        handle = RelationalHandle(torch.stack([other, node]), rel, n_other, n_node, R)
        self._csr = handle.pair_graph.by_dst()
        self.ptr, self.idx = self._csr.ptr, self._csr.idx
        self.pair_rel, self.pair_node = handle.pair_rel, handle.pair_dst
        self.pair_of_slot = handle._pair_of_edge
        self.edge_id = (handle._perm if edge_of is None
                        else _native.permute_index(edge_of.to(torch.int64), handle._perm))

    @property
    def hub(self):
        return self._csr.hub


class FilmForms:
    """What the three FiLM launches walk: the by-destination form of ALL edges (``fwd``, with its
    slot -> edge map ``edge_id``, the per-edge int32 ``rel`` in ``[0, R)`` and, for mean, the
    per-edge ``scale = 1 / |N_r(i)|``) and the two pair forms of the backward, by ``(relation,
    destination)`` and by ``(relation, source)``.  The pair forms are given (a layer's cached
    ones) or, for a CSR pair of the operator route, built when the backward first asks."""

    def __init__(self, fwd, edge_id, rel, scale, R, n_src, pairs=None):
        self.fwd, self.edge_id, self.rel, self.scale = fwd, edge_id, rel, scale
        self.R, self.n_src, self._given = int(R), int(n_src), pairs

    @classmethod
    def of_edges(cls, src, dst, rel, n_src, n_dst, R, mean):
        """The forms of an edge list whose ``rel`` (int32) lies in ``[0, R)`` and is sorted: the
        stable by-destination sort then leaves every row grouped by relation."""
        from .edge_index import EdgeIndex
        fwd = EdgeIndex(torch.stack([src, dst]), (n_src, n_dst)).by_dst()
        src64, dst64 = src.to(torch.int64), dst.to(torch.int64)
        pairs = (_PairForm(dst64, src64, rel, n_dst, n_src, R),
                 _PairForm(src64, dst64, rel, n_src, n_dst, R))
        scale = film_mean_scale(pairs[0]) if mean else None
        return cls(fwd, fwd.perm, rel, scale, R, n_src, pairs)

    @classmethod
    def of_csr(cls, rowptr, col, edge_id, rel, scale, n_src, R):
        return cls(_Form(rowptr, col), edge_id, rel, scale, R, n_src)

    @functools.cached_property
    def pairs(self):
        """``(by (relation, destination), by (relation, source))``"""
        if self._given is not None:
            return self._given
        ptr, col = self.fwd.ptr, self.fwd.idx
        dst = _native.ptr2index(ptr, col.numel()).to(torch.int64)
        src = col.to(torch.int64)
        rel = self.rel if self.edge_id is None else self.rel[self.edge_id.to(torch.int64)]
        n_dst = self.fwd.n_rows
        return (_PairForm(dst, src, rel, n_dst, self.n_src, self.R),
                _PairForm(src, dst, rel, self.n_src, n_dst, self.R, edge_of=self.edge_id))


def film_mean_scale(by_dst_pairs):
    """the per-edge mean normaliser ``1 / |N_r(i)|`` (float32 ``[E]``, in edge order) from the
    lengths of the ``(relation, destination)`` pair rows"""
    ptr = by_dst_pairs.ptr
    inv = 1.0 / (ptr[1:] - ptr[:-1]).to(torch.float32)
    scale = torch.empty(by_dst_pairs.idx.numel(), dtype=torch.float32, device=ptr.device)
    scale[by_dst_pairs.edge_id] = inv[by_dst_pairs.pair_of_slot]
    return scale


def film_split(h, g):
    """``(H, G)`` as the kernels read them: two tensors, or (``g`` None) the column blocks of the
    packed ``h = [H | G] [N, 3 R F]`` in place"""
    if g is not None:
        return h, g
    third = h.size(1) // 3
    return h[:, :third], h[:, third:]


def film_forward(forms, h, g, residual, relu):
    """``out [n_dst, F]`` of :func:`_native.film_forward` on ``forms``; the rows the handle's
    indices reach are checked here, the kernels check none"""
    H, G = film_split(h, g)
    fwd = forms.fwd
    if H.size(0) < forms.n_src:
        raise ValueError(f"'h' needs {forms.n_src} rows (got {H.size(0)})")
    return _native.film_forward(fwd.ptr, fwd.idx, forms.edge_id, forms.rel, H, G, forms.R,
                                scale=forms.scale, residual=residual, relu=relu, hub=fwd.hub)


def film_backward(forms, h, g, grad_out, *, relu=True, want_h=True, want_g=True):
    """``(grad_h, grad_g)``, None where not wanted: one launch over the ``(relation, destination)``
    pair rows (``grad_G``), one over the ``(relation, source)`` pair rows (``grad_H``), both into
    zero-filled planes and both recomputing the activation's mask.  With the packed ``h = [H | G]``
    (``g`` None) they write the column blocks of ONE ``[N, 3 R F]`` plane, which is ``grad_h``."""
    H, G = film_split(h, g)
    if grad_out.size(0) != forms.fwd.n_rows or H.size(0) < forms.n_src:
        raise ValueError(f"'grad_out' needs {forms.fwd.n_rows} rows and 'h' {forms.n_src}")
    packed = g is None
    out_h = out_g = plane = None
    if packed:
        if want_h:
            plane = torch.zeros_like(h, memory_format=torch.contiguous_format)
            out_h, out_g = film_split(plane, None)
    else:
        out_h = torch.zeros_like(h, memory_format=torch.contiguous_format) if want_h else None
        out_g = torch.zeros_like(g, memory_format=torch.contiguous_format) if want_g else None
    by_dst, by_src = forms.pairs
    if out_g is not None:
        _native.film_backward_dst(by_dst.ptr, by_dst.idx, by_dst.pair_rel, by_dst.pair_node, H, G,
                                  forms.R, grad_out, out_g, mean=forms.scale is not None,
                                  relu=relu, hub=by_dst.hub)
    if out_h is not None:
        _native.film_backward_src(by_src.ptr, by_src.idx, by_src.edge_id, by_src.pair_rel,
                                  by_src.pair_node, H, G, forms.R, grad_out, out_h,
                                  scale=forms.scale, relu=relu, hub=by_src.hub)
    return (plane, None) if packed else (out_h, out_g)


class RgatForms:
    """What the RGAT launches walk: the by-destination form of ALL edges (``fwd``), the int32
    relation of every SLOT (``rel``, in ``[0, R)``), ``perm`` = slot -> the caller's edge and
    ``inv`` = the caller's edge -> slot (both int64; None: the slots are the edges), the float
    in-degree ``deg [n_dst]`` and, built when the backward first asks, the ``(relation,
    destination)`` and ``(relation, source)`` pair forms of the SLOTS: their ``edge_id`` is the map
    from a pair slot to its by-destination slot."""

    def __init__(self, fwd, rel, perm, R, n_src):
        self.fwd, self.rel, self.perm = fwd, rel, perm
        self.R, self.n_src = int(R), int(n_src)

    @classmethod
    def of_edges(cls, src, dst, et, n_src, n_dst, R):
        """The forms of an edge list with relations ``et`` (int64, in ``[0, R)``: checked by the
        caller).  The edges are sorted by relation first: the stable by-destination sort then
        leaves every row grouped by relation."""
        from .edge_index import EdgeIndex
        if src.numel() > 0:
            lo, hi = _native.index_minmax(src)
            lo_d, hi_d = _native.index_minmax(dst)
            if lo < 0 or hi >= n_src or lo_d < 0 or hi_d >= n_dst:
                raise IndexError(f"'edge_index' must point into [0, {n_src}) x [0, {n_dst}) "
                                 f"(got sources in [{lo}, {hi}], destinations in [{lo_d}, {hi_d}])")
        _, first = _native.index_sort(et, max_value=R - 1)
        fwd = EdgeIndex(torch.stack([src[first], dst[first]]), (n_src, n_dst)).by_dst()
        perm = first[fwd.perm.to(torch.int64)]
        return cls(fwd, et[perm].to(torch.int32), perm, R, n_src)

    @classmethod
    def of_csr(cls, rowptr, col, rel, n_src, R):
        return cls(_Form(rowptr, col), rel, None, R, n_src)

    @functools.cached_property
    def inv(self):
        if self.perm is None:
            return None
        inv = torch.empty_like(self.perm)
        inv[self.perm] = torch.arange(self.perm.numel(), device=self.perm.device)
        return inv

    @functools.cached_property
    def deg(self):
        ptr = self.fwd.ptr
        return (ptr[1:] - ptr[:-1]).to(torch.float32)

    @functools.cached_property
    def pairs(self):
        """``(by (relation, destination), by (relation, source))`` with their slot maps"""
        ptr, col = self.fwd.ptr, self.fwd.idx
        dst = _native.ptr2index(ptr, col.numel()).to(torch.int64)
        src = col.to(torch.int64)
        n_dst = self.fwd.n_rows
        pairs = (_PairForm(dst, src, self.rel, n_dst, self.n_src, self.R),
                 _PairForm(src, dst, self.rel, self.n_src, n_dst, self.R))
        for form in pairs:
            form.slot_map = form.edge_id.to(form.ptr.dtype).contiguous()
        return pairs


def rgat_split(p, qi, kj, R, H, C):
    """``(P, QI, KJ)`` as the kernels read them: three tensors, or (``qi`` None) the column blocks
    of the packed ``p = [P | QI | KJ] [N, R (H C + 2 H)]`` in place"""
    if qi is not None:
        return p, qi, kj
    w, h = R * H * C, R * H
    if p.dim() != 2 or p.size(1) != w + 2 * h:
        raise ValueError(f"the packed plane must be [N, {w + 2 * h}] (got {tuple(p.shape)})")
    return p[:, :w], p[:, w:w + h], p[:, w + h:]


def rgat_forward(forms, p, qi, kj, b, H, C, slope, within=False):
    """``(alpha [E, H] in SLOT order, out [n_dst, H * C])`` of :func:`_native.rgat_forward` on
    ``forms``; ``b`` is in slot order.  ``within``: one scalar launch over the ``(relation,
    destination)`` pair rows first (the pairs' normalisers).  The rows the handle's indices reach
    are checked here, the kernels check none."""
    P, QI, KJ = rgat_split(p, qi, kj, forms.R, H, C)
    fwd = forms.fwd
    if P.size(0) < forms.n_src or QI.size(0) < fwd.n_rows:
        raise ValueError(f"the planes need {forms.n_src} source and {fwd.n_rows} destination rows")
    stats = None
    if within and fwd.idx.numel() > 0:
        by_dst = forms.pairs[0]
        stats = _native.rgat_pair_stats(by_dst.ptr, by_dst.idx, by_dst.slot_map, by_dst.pair_rel,
                                        by_dst.pair_node, QI, KJ, b, fwd.n_rows, forms.R, H, slope)
    return _native.rgat_forward(fwd.ptr, fwd.idx, forms.rel, P, QI, KJ, b, forms.R, H, C, slope,
                                pair_stats=stats, hub=fwd.hub)


def rgat_backward(forms, p, qi, kj, b, alpha, out, grad_out, H, C, slope, *, within=False,
                  want_b=False):
    """``(grad_p, grad_qi, grad_kj, grad_s)``: one launch over the forward's rows (``grad_s``,
    which is the gradient of ``b`` in slot order; None unless ``want_b``), one over the ``(relation,
    destination)`` pair rows (``grad_QI``; ``within``: the scalar launch that also finishes
    ``grad_s`` with the pair's sum) and one over the ``(relation, source)`` pair rows (``grad_P``,
    ``grad_KJ``), all into zero-filled planes.  With the packed ``p`` (``qi`` None) they write the
    column blocks of ONE plane of its shape, which is ``grad_p``."""
    R = forms.R
    P, QI, KJ = rgat_split(p, qi, kj, R, H, C)
    fwd = forms.fwd
    grad_s = _native.rgat_backward_dst(fwd.ptr, fwd.idx, forms.rel, P, QI, KJ, b, alpha, grad_out,
                                       out, R, H, C, slope, within=within, hub=fwd.hub)
    if qi is None:
        plane = torch.zeros_like(p, memory_format=torch.contiguous_format)
        g_p, g_qi, g_kj = rgat_split(plane, None, None, R, H, C)
    else:
        plane = None
        g_p, g_qi, g_kj = (torch.zeros_like(t, memory_format=torch.contiguous_format)
                           for t in (p, qi, kj))
    by_dst, by_src = forms.pairs
    if within:
        _native.rgat_pair_finish(by_dst.ptr, by_dst.idx, by_dst.slot_map, by_dst.pair_rel,
                                 by_dst.pair_node, QI, KJ, b, alpha, grad_s, R, H, slope, g_qi)
    else:
        _native.rgat_backward_src(by_dst.ptr, by_dst.idx, by_dst.slot_map, by_dst.pair_rel,
                                  by_dst.pair_node, alpha, grad_s, None, R, H, C, g_qi, None,
                                  hub=by_dst.hub)
    _native.rgat_backward_src(by_src.ptr, by_src.idx, by_src.slot_map, by_src.pair_rel,
                              by_src.pair_node, alpha, grad_s, grad_out, R, H, C, g_kj, g_p,
                              hub=by_src.hub)
    grad_b = grad_s if want_b else None
    return (plane, None, None, grad_b) if qi is None else (g_p, g_qi, g_kj, grad_b)


def _transposed_product(a, b):
    """``a.T @ b`` (``a [n, p]``, ``b [n, q]``) on the package's weight-gradient GEMM from the
    row count up at which :func:`_functions.linear` takes the own kernels"""
    from ._functions import own_linear_eligible
    if own_linear_eligible(a, b):
        return _native.linear_wgrad(a, b)
    return a.t() @ b


def mixture_forward(fwd, edge_id, x_src, coef, weight):
    """``out [n_dst, M]`` of a mixture message ``m_e = sum_k coef[e, k] (x_j weight[k])`` summed
    over the slots of every destination, aggregate first: one expand launch (``Z [n_dst, K * F]``,
    one gathered row of ``F`` floats per slot) and one dense product with ``weight [K, F, M]``."""
    from ._functions import linear
    K, F, M = weight.shape
    z = _native.mixture_expand(fwd.ptr, fwd.idx, edge_id, x_src, coef, hub=fwd.hub)
    return linear(z, weight.reshape(K * F, M).t().contiguous())


def mixture_backward(slots, x_src, coef, weight, grad_out, *, want_x=True, want_coef=True,
                     want_weight=True):
    """``(grad_x_src, grad_coef, grad_weight)``, None where not wanted.  ``grad_weight = Z^T
    grad_out`` with ``Z`` recomputed by one expand; ``grad_coef`` from ``gZ = grad_out @ W^T`` held
    per destination (one launch); ``grad_x`` one expand of ``grad_out`` over the by-source form and
    one dense product with ``weight``'s axes permuted.  Each reads ``F`` or ``M`` floats per edge."""
    from ._functions import linear
    K, F, M = weight.shape
    fwd = slots.fwd
    g_x = g_c = g_w = None
    if want_weight:
        z = _native.mixture_expand(fwd.ptr, fwd.idx, slots.edge_id(), x_src, coef, hub=fwd.hub)
        g_w = _transposed_product(z, grad_out).view(K, F, M)
        del z
    if want_coef:
        g_z = linear(grad_out, weight.reshape(K * F, M))
        g_c = _native.mixture_coef_grad(fwd.ptr, fwd.idx, slots.edge_id(), g_z, x_src, hub=fwd.hub)
        del g_z
    if want_x:
        bwd = slots.by_src()
        t = _native.mixture_expand(bwd.ptr, bwd.idx, slots.edge_id_t(), grad_out, coef,
                                   hub=bwd.hub)
        g_x = linear(t, weight.permute(1, 0, 2).reshape(F, K * M))
    return g_x, g_c, g_w


def hgt_blocks(kqvs, src_pos, F):
    """``(ks, vs)`` per edge type: the key and value column blocks of its ``[N, 3 * F]`` source"""
    return [kqvs[p][:, :F] for p in src_pos], [kqvs[p][:, 2 * F:] for p in src_pos]


def hgt_backward(kqvs, wk, wv, src_pos, widx, H, grad_kv, *, want_kqvs=True, want_weights=True):
    """``(grad_kqvs | [], grad_wk, grad_wv)`` in one launch: one ``[N_t, 3 * F]`` buffer per node
    type takes the k and v gradients; its q block is cleared."""
    D = wk.size(-1)
    F = H * D
    ks, vs = hgt_blocks(kqvs, src_pos, F)
    bufs = []
    if want_kqvs:
        bufs = [torch.empty_like(x, memory_format=torch.contiguous_format) for x in kqvs]
        for b in bufs:
            b[:, F:2 * F].zero_()
    g_wk, g_wv = _native.hgt_relation_backward(
        ks, vs, widx, src_pos, wk, wv, H, D, grad_kv, [b[:, :F] for b in bufs],
        [b[:, 2 * F:] for b in bufs], weight_grads=want_weights)
    return bufs, g_wk, g_wv


def hop_forward(fwd, edge_id, w, x, a, y=None, b=0.0, z=None, c=0.0):
    """One propagation step ``a * A x (+ b y) (+ c z)`` over a by-destination form: one launch.
    ``w`` is in the caller's edge order (``edge_id``: slot -> edge, None: slot order)."""
    return _native.hop(fwd.ptr, fwd.idx, edge_id if w is not None else None, w, x, a, y=y, b=b,
                       z=z, c=c, hub=fwd.hub)


def hop_backward(slots, w, grad_out, a, b, c, *, want_x=True, want_y=False, want_z=False):
    """``(grad_x, grad_y, grad_z)`` of :func:`hop_forward`, None where not wanted: ``grad_x = a *
    A^T grad_out`` is the same launch over the by-source form; the other two are one elementwise
    pass each."""
    g_x = g_y = g_z = None
    if want_x:
        bwd = slots.by_src()
        g_x = _native.hop(bwd.ptr, bwd.idx, slots.edge_id_t() if w is not None else None, w,
                          grad_out, a, hub=bwd.hub)
    if want_y:
        g_y = grad_out * b
    if want_z:
        g_z = grad_out * c
    return g_x, g_y, g_z


def hops_forward(fwd, edge_id, w, x, h, K, a, b, d0=0.0, d=0.0, want_sum=False):
    """``(x_K, s | None)`` of the recurrence ``x_k = a * A x_{k-1} + b * h`` (``h`` None: no second
    term), ``s = d0 * x_0 + d * sum_{k >= 1} x_k``: exactly ``K >= 1`` launches, each of which adds
    its iterate to ``s`` in its epilogue; two planes alternate as the iterates."""
    edge_id = edge_id if w is not None else None
    s = x * d0 if want_sum else None
    planes = [None, None]
    cur = x
    for k in range(K):
        if planes[k & 1] is None:
            planes[k & 1] = torch.empty(fwd.n_rows, x.size(1), dtype=x.dtype, device=x.device)
        cur = _native.hop(fwd.ptr, fwd.idx, edge_id, w, cur, a, y=h, b=b, out=planes[k & 1],
                          sum=s, d=d, hub=fwd.hub)
    return cur, s


def hops_backward(slots, w, K, a, b, d0, d, grad_x, grad_s, *, has_h=False, tied=False,
                  want_x=True, want_h=False):
    """``(grad_x0, grad_h)`` of :func:`hops_forward`, None where not wanted.  With ``T = A^T`` the
    adjoints are ``G_K = grad_x + d grad_s``, ``G_{k-1} = a T G_k + d grad_s`` and ``G_0 = a T G_1
    + d0 grad_s``: ``K`` launches over the by-source form (``grad_s`` is their ``y`` term), no
    iterate of the forward is needed.  ``grad_h = b (G_1 + ... + G_K)``: the launches that write
    ``G_{K-1} .. G_1`` add ``b`` times their output to one plane in their epilogue, ``b G_K`` joins
    it in one elementwise pass.  ``tied`` (``h`` is ``x_0``, APPNP): the last launch takes that
    plane and ``G_K`` as its ``y`` / ``z`` terms and writes the whole gradient.  Besides the
    launches: one pass for ``G_K`` when both gradients arrive, one for ``grad_h``."""
    bwd = slots.by_src()
    edge_id_t = slots.edge_id_t() if w is not None else None
    if grad_x is None:
        g = grad_s * d
    elif grad_s is None:
        g = grad_x
    else:
        g = torch.add(grad_x, grad_s, alpha=d)
    g_last = g
    need_h = has_h and (want_h or (tied and want_x))
    fold = tied and need_h and grad_s is None
    n, F = bwd.n_rows, g.size(1)
    acc = (torch.empty(n, F, dtype=g.dtype, device=g.device) if need_h and K >= 2 else None)
    planes = [None, None]
    for j in range(K, 0, -1):
        last = j == 1
        if last and not (want_x or fold):
            g = None
            break
        y, by, z, cz = grad_s, (d0 if last else d), None, 0.0
        if last and fold:  # grad = G_0 + b (G_1 + ... + G_K)
            y, by, z, cz = (g_last, b, None, 0.0) if acc is None else (acc, 1.0, g_last, b)
        if planes[j & 1] is None:
            planes[j & 1] = torch.empty(n, F, dtype=g.dtype, device=g.device)
        g = _native.hop(bwd.ptr, bwd.idx, edge_id_t, w, g, a, y=y, b=by, z=z, c=cz,
                        out=planes[j & 1], sum=None if last else acc, d=b, sum_init=j == K,
                        hub=bwd.hub)
    g_h = None
    if need_h and not fold:
        g_h = g_last * b if acc is None else torch.add(acc, g_last, alpha=b)
        if tied:
            g, g_h = g + g_h, None
    return (g if want_x else None), (g_h if want_h and not tied else None)
