"""A plain-Python restatement of heterogeneous neighbour sampling, ``pyg-lib``'s sequential hetero
loop as the reference calls it with ``csc=True`` (sampler/neighbor_sampler.py:438-548), for the
draws that are deterministic: ``-1`` fan-outs, and bounded ones where no destination has more
in-neighbours than ``k`` (without replacement).  Hop ``h`` goes through the edge types in order;
an edge type ``(src, rel, dst)`` takes the in-edges, in ``edge_index`` order, of every ``dst`` node
added in hop ``h - 1`` (the seeds count as hop -1); a new ``src`` node is appended to its type's
list on first sight.  ``disjoint``: nodes are (tree, node) pairs."""


def _csc(edge_index, num_dst):
    ins = [[] for _ in range(num_dst)]
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    for e, (u, v) in enumerate(zip(src, dst)):
        ins[v].append((u, e))
    return ins


def hetero_sample(edge_index_dict, num_nodes_dict, num_neighbors, input_type, seeds,
                  disjoint=False):
    """Returns ``(node, row, col, edge, batch, num_sampled_nodes, num_sampled_edges)`` as dicts of
    Python lists (``batch`` is ``None`` unless ``disjoint``).  ``num_neighbors``: a dict of lists
    keyed by edge type."""
    node_types = list(num_nodes_dict)
    edge_types = list(edge_index_dict)
    csc = {et: _csc(edge_index_dict[et], num_nodes_dict[et[2]]) for et in edge_types}
    seeds = [int(s) for s in seeds]
    B = len(seeds)
    key = {t: [] for t in node_types}        # (tree, node) or node
    where = {t: {} for t in node_types}
    for i, s in enumerate(seeds):
        k = (i, s) if disjoint else s
        where[input_type][k] = len(key[input_type])
        key[input_type].append(k)
    span = {t: (0, 0) for t in node_types}
    span[input_type] = (0, B)
    row = {et: [] for et in edge_types}
    col = {et: [] for et in edge_types}
    edge = {et: [] for et in edge_types}
    n_nodes = {t: [B if t == input_type else 0] for t in node_types}
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
                tree, v = dk if disjoint else (None, dk)
                ins = csc[et][v] if k != 0 else []
                if k > 0 and len(ins) > k:
                    raise ValueError('the draws are random here: the restatement covers '
                                     'deg <= k, k = 0 and k = -1 only')
                for u, e in ins:
                    sk = (tree, u) if disjoint else u
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


def sampled_info_graph():
    """The graph of the reference's ``test_hetero_neighbor_loader_sampled_info``
    (test/loader/test_neighbor_loader.py:756-793): one edge_index for three edge types."""
    import torch
    ei = torch.tensor([[2, 3, 4, 5, 7, 7, 10, 11, 12, 13],
                       [0, 1, 2, 3, 2, 3, 7, 7, 7, 7]])
    num_nodes = {'paper': 14, 'author': 14}
    eid = {('paper', 'to', 'paper'): ei, ('paper', 'to', 'author'): ei,
           ('author', 'to', 'paper'): ei}
    return eid, num_nodes


SAMPLED_INFO_NODES = {'paper': [2, 2, 3, 4], 'author': [0, 2, 3, 4]}
SAMPLED_INFO_EDGES = {('paper', 'to', 'paper'): [2, 4, 4], ('paper', 'to', 'author'): [0, 4, 4],
                      ('author', 'to', 'paper'): [2, 4, 4]}
