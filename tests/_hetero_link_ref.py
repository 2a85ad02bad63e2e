"""A plain-Python restatement of heterogeneous LINK-level neighbour sampling: the seed block and
the metadata of an edge batch of one edge type ``(S, rel, D)`` (the heterogeneous branch of the
reference's ``edge_sample``, sampler/neighbor_sampler.py:852-998) and the hop loop of
``tests/_hetero_ref.py`` started from seeds of more than one node type.  Same conventions and the
same domain as there (deterministic draws only: ``-1``, ``k = 0`` or ``deg <= k``).  The negatives
are random, so they are INPUTS here: the tests take them from the device output.

Seed dict: ``S != D`` gives ``{S: src, D: dst}`` (each its sorted unique unless ``disjoint``),
``S == D`` the one vector ``src + dst`` (its sorted unique unless ``disjoint``).  Disjoint trees are
numbered consecutively through the seed dict in its order: source seed ``j`` is tree ``j``,
destination seed ``j`` tree ``len(src) + j``; the seed time of a tree is the entry of
``src_time + dst_time`` at that number; at the end ``batch[t] %= P`` for every node type."""
import math

from tests._hetero_ref import _csc


def hetero_sample_multi(edge_index_dict, num_nodes_dict, num_neighbors, seed_dict,
                        disjoint=False):
    """``tests._hetero_ref.hetero_sample`` from a seed dict ``{node type: seeds}`` (in its order)
    instead of one input type.  Returns ``(node, row, col, edge, batch, num_sampled_nodes,
    num_sampled_edges)`` as dicts of Python lists; ``batch`` holds tree ids."""
    node_types = list(num_nodes_dict)
    edge_types = list(edge_index_dict)
    csc = {et: _csc(edge_index_dict[et], num_nodes_dict[et[2]]) for et in edge_types}
    key = {t: [] for t in node_types}        # (tree, node) or node
    where = {t: {} for t in node_types}
    span = {t: (0, 0) for t in node_types}
    tree = 0
    for t, seeds in seed_dict.items():
        for s in seeds:
            k = (tree, int(s)) if disjoint else int(s)
            where[t][k] = len(key[t])
            key[t].append(k)
            tree += 1
        span[t] = (0, len(key[t]))
    row = {et: [] for et in edge_types}
    col = {et: [] for et in edge_types}
    edge = {et: [] for et in edge_types}
    n_nodes = {t: [len(key[t])] for t in node_types}
    n_edges = {et: [] for et in edge_types}
    hops = len(next(iter(num_neighbors.values()))) if num_neighbors else 0
    for h in range(hops):
        begin = {t: len(key[t]) for t in node_types}
        for et in edge_types:
            s_t, _, d_t = et
            k = num_neighbors[et][h]
            lo, hi = span[d_t]
            m = 0
            for dl in range(lo, hi):
                dk = key[d_t][dl]
                tr, v = dk if disjoint else (None, dk)
                ins = csc[et][v] if k != 0 else []
                if k > 0 and len(ins) > k:
                    raise ValueError('the draws are random here: the restatement covers '
                                     'deg <= k, k = 0 and k = -1 only')
                for u, e in ins:
                    sk = (tr, u) if disjoint else u
                    if sk not in where[s_t]:
                        where[s_t][sk] = len(key[s_t])
                        key[s_t].append(sk)
                    row[et].append(where[s_t][sk])
                    col[et].append(dl)
                    edge[et].append(e)
                    m += 1
            n_edges[et].append(m)
        for t in node_types:
            span[t] = (begin[t], len(key[t]))
            n_nodes[t].append(len(key[t]) - begin[t])
    if disjoint:
        node = {t: [k[1] for k in key[t]] for t in node_types}
        batch = {t: [k[0] for k in key[t]] for t in node_types}
    else:
        node, batch = {t: list(key[t]) for t in node_types}, None
    return node, row, col, edge, batch, n_nodes, n_edges


def _unique_inverse(xs):
    uniq = sorted(set(xs))
    pos = {v: i for i, v in enumerate(uniq)}
    return uniq, [pos[v] for v in xs]


def link_seed_block(input_type, src, dst, mode=None, amount=1, src_neg=(), dst_neg=(),
                    disjoint=False, label=None, time=None):
    """The seed block of ``P = len(src)`` seed links of the edge type ``input_type`` given their
    negatives (``src_neg``: binary only; both ``ceil(P * amount)`` long).  Returns a dict:
    ``seed_dict`` (ordered), ``seed_time`` (one per tree, ``None`` without ``time``), ``P``, and
    the metadata after ``input_id``: ``index`` = ``[row 0, row 1]`` of ``edge_label_index`` (no
    negatives / binary) or ``(src_index, dst_pos_index, dst_neg_index)`` (triplet;
    ``dst_neg_index`` flat for ``amount == 1``, else one list of ``amount`` per positive),
    ``label`` and ``src_time``."""
    s_t, d_t = input_type[0], input_type[-1]
    src, dst = [int(v) for v in src], [int(v) for v in dst]
    P = len(src)
    num_neg = 0
    src_time = dst_time = None if time is None else [int(t) for t in time]
    if mode is not None:
        num_neg = math.ceil(P * amount)
        dst_neg = [int(v) for v in dst_neg]
        assert len(dst_neg) == num_neg
        dst = dst + dst_neg
        if mode == 'binary':
            src_neg = [int(v) for v in src_neg]
            assert len(src_neg) == num_neg
            src = src + src_neg
            label = [1.0] * P if label is None else list(label)
            label = label + [0] * num_neg
            if time is not None:
                src_time = dst_time = (src_time * (1 + math.ceil(amount)))[:P + num_neg]
        else:
            assert mode == 'triplet' and label is None and amount == int(amount)
            if time is not None:
                dst_time = dst_time * (1 + amount)
    n_src, n_dst = len(src), len(dst)
    if s_t != d_t:
        if disjoint:
            inv_src, inv_dst = list(range(n_src)), list(range(n_dst))
        else:
            src, inv_src = _unique_inverse(src)
            dst, inv_dst = _unique_inverse(dst)
        seed_dict = {s_t: src, d_t: dst}
    else:
        seed = src + dst
        if disjoint:
            inv = list(range(len(seed)))
        else:
            seed, inv = _unique_inverse(seed)
        inv_src, inv_dst = inv[:n_src], inv[n_src:]
        seed_dict = {s_t: seed}
    seed_time = None if time is None else src_time + dst_time
    if mode == 'triplet':
        neg = inv_dst[P:]
        if disjoint:   # slot P + j is negative j // P of positive j % P
            per_pos = [[neg[a * P + i] for a in range(amount)] for i in range(P)]
        else:
            per_pos = [neg[i * amount:(i + 1) * amount] for i in range(P)]
        dst_neg_index = [p[0] for p in per_pos] if amount == 1 else per_pos
        index = (inv_src, inv_dst[:P], dst_neg_index)
    else:
        index = [inv_src, inv_dst]
    return dict(seed_dict=seed_dict, seed_time=seed_time, P=P, index=index, label=label,
                src_time=src_time)


def hetero_link_sample(edge_index_dict, num_nodes_dict, num_neighbors, input_type, src, dst,
                       disjoint=False, **kw):
    """The whole edge batch: :func:`link_seed_block`, the hops from its seed dict and
    ``batch[t] %= P``.  Returns ``(hops, block)``: the 7-tuple of :func:`hetero_sample_multi` and
    the seed block's dict."""
    block = link_seed_block(input_type, src, dst, disjoint=disjoint, **kw)
    out = list(hetero_sample_multi(edge_index_dict, num_nodes_dict, num_neighbors,
                                   block['seed_dict'], disjoint=disjoint))
    if disjoint:
        out[4] = {t: [b % block['P'] for b in bs] for t, bs in out[4].items()}
    return tuple(out), block
