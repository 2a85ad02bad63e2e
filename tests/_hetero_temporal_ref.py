"""A plain-Python restatement of TEMPORAL heterogeneous neighbour sampling (rules 1-7 of
``HeteroNeighborSampler``'s docstring) for the draws that are deterministic: ``'last'`` without
replacement for any ``k``, and ``'uniform'`` with ``-1`` or with every window ``<= k``.  It is the
edge-type loop of ``tests/_hetero_ref.hetero_sample`` (always disjoint: nodes are (tree, node)
pairs) with, per timed edge type, the time-sorted column, the eligible prefix (time <= the seed
time of the destination's TREE) and its last ``k`` slots.  An untimed edge type keeps ``edge_index``
order and its whole column, whatever the strategy.  It raises on a random draw."""


def _timed_csc(edge_index, num_dst, key):
    """Per destination the (source, edge position) pairs: ascending in (time, edge position) when
    ``key`` (one time per edge) is given, in ``edge_index`` order otherwise."""
    ins = [[] for _ in range(num_dst)]
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    for e, (u, v) in enumerate(zip(src, dst)):
        ins[v].append((u, e))
    if key is not None:
        for v in range(num_dst):
            ins[v].sort(key=lambda ue: (key[ue[1]], ue[1]))
    return ins


def hetero_temporal_sample(edge_index_dict, num_nodes_dict, num_neighbors, input_type, seeds,
                           node_time=None, edge_time=None, seed_time=None, strategy='uniform',
                           replace=False):
    """Returns ``(node, row, col, edge, batch, num_sampled_nodes, num_sampled_edges)`` as dicts of
    Python lists.  ``num_neighbors``: a dict of lists keyed by edge type; ``node_time`` /
    ``edge_time``: dicts of integer sequences (types may be missing); ``seed_time``: one integer
    per seed (default ``node_time[input_type][seed]``)."""
    if (node_time is None) == (edge_time is None):
        raise ValueError("exactly one of 'node_time' and 'edge_time'")
    node_types = list(num_nodes_dict)
    edge_types = list(edge_index_dict)
    as_list = (lambda t: t.tolist() if hasattr(t, 'tolist') else list(t))
    key = {}                                  # timed edge types: one time per edge
    for et in edge_types:
        if node_time is not None and et[0] in node_time:
            nt = as_list(node_time[et[0]])
            key[et] = [nt[u] for u in edge_index_dict[et][0].tolist()]
        elif edge_time is not None and et in edge_time:
            key[et] = as_list(edge_time[et])
    csc = {et: _timed_csc(edge_index_dict[et], num_nodes_dict[et[2]], key.get(et))
           for et in edge_types}
    seeds = [int(s) for s in seeds]
    B = len(seeds)
    if seed_time is None:
        if node_time is None or input_type not in node_time:
            raise ValueError('needs the seed times')
        nt = as_list(node_time[input_type])
        seed_time = [nt[s] for s in seeds]
    seed_time = [int(t) for t in as_list(seed_time)]
    keys = {t: [] for t in node_types}        # (tree, node)
    where = {t: {} for t in node_types}
    for i, s in enumerate(seeds):
        where[input_type][(i, s)] = len(keys[input_type])
        keys[input_type].append((i, s))
    span = {t: (0, 0) for t in node_types}
    span[input_type] = (0, B)
    row = {et: [] for et in edge_types}
    col = {et: [] for et in edge_types}
    edge = {et: [] for et in edge_types}
    n_nodes = {t: [B if t == input_type else 0] for t in node_types}
    n_edges = {et: [] for et in edge_types}
    hops = len(next(iter(num_neighbors.values()))) if num_neighbors else 0
    for h in range(hops):
        begin = {t: len(keys[t]) for t in node_types}
        for et in edge_types:
            s_t, _, d_t = et
            k = num_neighbors[et][h]
            lo, hi = span[d_t]
            m = 0
            for dl in range(lo, hi):
                tree, v = keys[d_t][dl]
                ins = csc[et][v]
                if et in key:
                    ins = [ue for ue in ins if key[et][ue[1]] <= seed_time[tree]]
                    if strategy == 'last' and k >= 0:
                        ins = ins[max(0, len(ins) - k):]
                if k == 0:
                    ins = []
                if k > 0 and (len(ins) > k or (replace and len(ins) > 0)):
                    raise ValueError('the draws are random here: the restatement covers '
                                     "'last' without replacement, k = 0, k = -1 and windows <= k")
                for u, e in ins:
                    sk = (tree, u)
                    if sk not in where[s_t]:
                        where[s_t][sk] = len(keys[s_t])
                        keys[s_t].append(sk)
                    row[et].append(where[s_t][sk])
                    col[et].append(dl)
                    edge[et].append(e)
                    m += 1
            n_edges[et].append(m)
        for t in node_types:
            span[t] = (begin[t], len(keys[t]))
            n_nodes[t].append(len(keys[t]) - begin[t])
    node = {t: [k[1] for k in keys[t]] for t in node_types}
    batch = {t: [k[0] for k in keys[t]] for t in node_types}
    return node, row, col, edge, batch, n_nodes, n_edges


def edge_level_loader_graph():
    """The graph of the reference's ``test_edge_level_temporal_hetero_neighbor_loader``
    (test/loader/test_neighbor_loader.py:913-937): a path 0 - 1 - 2 - 3 - 4 of one node type with
    both directions of every edge, edge times 0..7."""
    import torch
    ei = torch.tensor([[0, 1, 1, 2, 2, 3, 3, 4], [1, 0, 2, 1, 3, 2, 4, 3]])
    et = ('A', 'to', 'A')
    return {et: ei}, {'A': 5}, {et: torch.arange(8)}
