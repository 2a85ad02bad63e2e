"""Generates tests/golden/golden_attn_nonfinite_v1.pt by running the REAL reference (PyG) on CPU:
``TransformerConv`` (with and without ``edge_dim``), ``GATv2Conv`` and a two-edge-type ``HGTConv``
on small graphs where head 1's score of every 7th source node overflows to -inf THROUGH THE
WEIGHTS, the attention-layer counterpart of ``test_gat_conv_with_masked_sources``.  Build
container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_attn_nonfinite.py

How the mask is made (C = 5 channels per head, ``r`` = the row of (head 1, channel 0)):
  * input column 0 is 0, and 1e10 on the masked nodes; no projection reads it except row ``r`` of
    the key-side one (``lin_key`` / ``lin_l`` / the k block of the source type's ``kqv_lin``), which
    copies it: key[j, 1, 0] = x[j, 0];
  * the other factor of that channel's product is a constant -1e30 (``lin_query.bias[r]``;
    ``att[1, 0]``) — for HGTConv -2e28 in the query and 4 in ``p_rel``: <q, K> = -2e38 is finite
    and overflows at the prior, so that the prior's gradient is not 0 * inf;
  * whatever else enters channel 0 of head 1 is zeroed (``lin_edge`` row r, ``lin_r`` row r, the
    relation matrices' column 0), so an unmasked source contributes an exact 0 there and the rest
    of the row is an ordinary softmax.
A masked edge gets coefficient exactly 0; every output and every gradient is finite.  Node 0 is
unmasked and reaches every destination.

Gradients that are multiplied by the 1e30 weight are ~1e29 and, where the softmax's
``sum_k d s = 0`` cancels them, pure rounding noise: ``group`` marks those entries (per input /
parameter) with 2, so that a test can judge them on their own, relative to their joint scale, and
with 1 the weights' column 0, whose gradients carry x[:, 0] = 1e10 (3: see ``finish``).  Everything else is of order 1
(asserted below).  Tensors only: inputs, state dicts, outputs,
attention weights, gradients and those masks.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ.get('PYG_REFERENCE', '/root/reference'))
import torch_geometric  # noqa: E402
import torch_geometric.typing as pyg_typing  # noqa: E402
from torch_geometric.nn import GATv2Conv, HGTConv, TransformerConv  # noqa: E402

assert not pyg_typing.WITH_TORCH_SCATTER and not pyg_typing.WITH_PYG_LIB \
    and not pyg_typing.WITH_SOFTMAX, "goldens must come from the plain CPU scatter path"

HERE = os.path.dirname(os.path.abspath(__file__))
N, E, FIN, HEADS, C = 60, 400, 6, 4, 5
R = 1 * C          # row of (head 1, channel 0) in a [HEADS * C] projection
BIG = 1e30


def gen(seed):
    return torch.Generator().manual_seed(seed)


def homogeneous(seed, edge_dim=None):
    g = gen(seed)
    x = torch.randn(N, FIN, generator=g)
    masked = torch.arange(N) % 7 == 3
    x[:, 0] = 0.
    x[masked, 0] = 1e10
    ei = torch.randint(1, N, (2, E), generator=g)
    ei = torch.cat([ei, torch.stack([torch.zeros(N - 1, dtype=torch.long),
                                     torch.arange(1, N)])], 1)  # node 0 (unmasked) reaches all
    ea = None if edge_dim is None else torch.randn(ei.size(1), edge_dim, generator=g)
    return x, masked, ei, ea


def zero_col0_except(weight, row):
    weight[:, 0] = 0.
    weight[row] = 0.
    weight[row, 0] = 1.


def run(conv, inputs, call):
    """forward + autograd on leaves cloned from ``inputs`` (a dict of float tensors)"""
    conv.eval()
    leaves = {k: v.clone().requires_grad_(True) for k, v in inputs.items()}
    res = call(conv, leaves)
    out = res['out']
    outs = list(out.values()) if isinstance(out, dict) else [out]
    g = gen(99)
    grad_out = [torch.randn(o.shape, generator=g) for o in outs]
    params = list(conv.named_parameters())
    grads = torch.autograd.grad(outs, list(leaves.values()) + [p for _, p in params], grad_out,
                                allow_unused=True)
    rec = {'state': {k: v.detach().clone() for k, v in conv.state_dict().items()},
           'out': {k: v.detach() for k, v in out.items()} if isinstance(out, dict)
           else out.detach(),
           'grad_out': dict(zip(out, grad_out)) if isinstance(out, dict) else grad_out[0],
           'grad_inputs': {k: g_.detach() for k, g_ in zip(leaves, grads) if g_ is not None},
           'grad_params': {n: g_.detach() for (n, _), g_ in zip(params, grads[len(leaves):])
                           if g_ is not None}}
    if 'attention' in res:
        rec['attention'] = (res['attention'][0].clone(), res['attention'][1].detach())
    return rec


def finish(rec, through, col0, noise=None):
    """``through``: name -> index of the entries behind the 1e30 weight; ``col0``: the weights
    whose column 0 multiplies x[:, 0] = 1e10 (gradients ~1e10, well conditioned).  Stored as
    ``group`` per tensor: 0 ordinary (of order 1), 1 column 0, 2 behind the 1e30 weight, 3
    (``noise``) the entries that are BOTH a sum that cancels behind the 1e30 weight and multiplied
    by 1e10: rounding noise of ~1e32 in any float32 evaluation, of which only finiteness can be
    asked."""
    groups = {}
    grads = {**rec['grad_inputs'], **rec['grad_params']}
    for name, g in grads.items():
        assert bool(g.isfinite().all()), name
        m = torch.zeros_like(g, dtype=torch.uint8)
        if name in col0:
            m[:, 0] = 1
        if name in through:
            m[through[name]] = 2
        if noise and name in noise:
            m[noise[name]] = 3
        assert float(g[m == 0].abs().max()) < 1e3, (name, float(g[m == 0].abs().max()))
        assert not bool((m == 1).any()) or float(g[m == 1].abs().max()) < 1e14, name
        groups[name] = m
    assert set(through) | set(col0) <= set(grads), (set(through) | set(col0)) - set(grads)
    assert max(float(grads[n][groups[n] == 2].abs().max()) for n in through) > 1e20
    assert max(float(grads[n][groups[n] == 2].abs().max()) for n in through) < 1e31
    rec['group'] = groups
    return rec


def transformer_case(seed, edge_dim=None):
    x, masked, ei, ea = homogeneous(seed, edge_dim)
    torch.manual_seed(seed)
    kw = dict(in_channels=FIN, out_channels=C, heads=HEADS)
    if edge_dim is not None:
        kw['edge_dim'] = edge_dim
    conv = TransformerConv(**kw)
    with torch.no_grad():
        for lin in (conv.lin_query, conv.lin_value, conv.lin_skip):
            lin.weight[:, 0] = 0.
        zero_col0_except(conv.lin_key.weight, R)     # key[:, head 1, 0] = x[:, 0]
        conv.lin_key.bias[R] = 0.
        conv.lin_query.weight[R] = 0.
        conv.lin_query.bias[R] = -BIG                # 1e10 * -1e30 overflows: the score is -inf
        if edge_dim is not None:
            conv.lin_edge.weight[R] = 0.
    inputs = {'x': x} if ea is None else {'x': x, 'edge_attr': ea}

    def call(conv, t):
        out, att = conv(t['x'], ei, t.get('edge_attr'), return_attention_weights=True)
        return {'out': out, 'attention': att}

    rec = run(conv, inputs, call)
    through = {'x': (slice(None), 0), 'lin_key.weight': R, 'lin_key.bias': R}
    if edge_dim is not None:
        through['lin_edge.weight'] = R
    rec.update(cls='TransformerConv', kwargs=kw, x=x, edge_index=ei, edge_attr=ea, masked=masked,
               seed=seed)
    return finish(rec, through, ['lin_key.weight', 'lin_query.weight', 'lin_value.weight',
                                 'lin_skip.weight'])


def gatv2_case(seed):
    x, masked, ei, _ = homogeneous(seed)
    torch.manual_seed(seed)
    kw = dict(in_channels=FIN, out_channels=C, heads=HEADS)
    conv = GATv2Conv(**kw)
    with torch.no_grad():
        zero_col0_except(conv.lin_l.weight, R)       # x_l[:, head 1, 0] = x[:, 0]
        conv.lin_l.bias[R] = 0.
        conv.lin_r.weight[:, 0] = 0.
        conv.lin_r.weight[R] = 0.                    # x_r[:, head 1, 0] = 0
        conv.lin_r.bias[R] = 0.
        conv.att[0, 1, 0] = -BIG                     # -1e30 * leaky_relu(1e10) overflows
    def call(conv, t):
        out, att = conv(t['x'], ei, return_attention_weights=True)
        return {'out': out, 'attention': att}

    rec = run(conv, {'x': x}, call)
    through = {'x': (slice(None), 0), 'lin_l.weight': R, 'lin_l.bias': R, 'lin_r.weight': R,
               'lin_r.bias': R}
    rec.update(cls='GATv2Conv', kwargs=kw, x=x, edge_index=ei, edge_attr=None, masked=masked,
               seed=seed)
    # grad lin_r.weight[R, 0] = sum_i grad_x_r[i, 1, 0] * x[i, 0]: grad_x_r[i, 1, 0] is -1e30 * slope
    # times sum_k d s[k] = 0 (every unmasked edge has the same slope), i.e. noise of ~1e22, and
    # x[i, 0] = 1e10 on the masked destinations
    return finish(rec, through, ['lin_l.weight', 'lin_r.weight'], {'lin_r.weight': (R, 0)})


AWP, PCP = ('author', 'writes', 'paper'), ('paper', 'cites', 'paper')


def hgt_case(seed):
    """Two edge types into 'paper'; the masked sources are authors, so only 'writes' has masked
    edges.  The overflow happens at the prior: <q, K> = -2e28 * 1e10, times p_rel = 4."""
    g = gen(seed)
    n_a, n_p, W = N, 30, HEADS * C
    x = {'author': torch.randn(n_a, FIN, generator=g), 'paper': torch.randn(n_p, W, generator=g)}
    masked = torch.arange(n_a) % 7 == 3
    x['author'][:, 0] = 0.
    x['author'][masked, 0] = 1e10
    awp = torch.stack([torch.randint(1, n_a, (300, ), generator=g),
                       torch.randint(0, n_p, (300, ), generator=g)])
    awp = torch.cat([awp, torch.stack([torch.zeros(n_p, dtype=torch.long),
                                       torch.arange(n_p)])], 1)   # author 0 reaches every paper
    pcp = torch.randint(0, n_p, (2, 100), generator=g)
    eis = {AWP: awp, PCP: pcp}
    torch.manual_seed(seed)
    kw = dict(in_channels={'author': FIN, 'paper': W}, out_channels=W,
              metadata=(['author', 'paper'], [AWP, PCP]), heads=HEADS)
    conv = HGTConv(**kw)
    T = 2
    with torch.no_grad():
        for p in list(conv.skip.values()) + list(conv.p_rel.values()):
            p.copy_(torch.randn(p.shape, generator=g))
        wa, ba = conv.kqv_lin.lins['author'].weight, conv.kqv_lin.lins['author'].bias
        wp, bp = conv.kqv_lin.lins['paper'].weight, conv.kqv_lin.lins['paper'].bias
        zero_col0_except(wa, R)                      # k block: k_author[:, head 1, 0] = x[:, 0]
        ba[R] = 0.
        wp[R] = 0.                                   # k_paper[:, head 1, 0] = 0
        bp[R] = 0.
        wp[W + R] = 0.                               # q block: q_paper[:, head 1, 0] = -2e28
        bp[W + R] = -2e28
        k_rel = conv.k_rel.weight.view(HEADS, T, C, C)
        k_rel[1, :, :, 0] = 0.                       # nothing else enters channel 0 of head 1 ...
        k_rel[1, 0, 0, :] = 0.                       # ... and 1e10 enters no other channel
        k_rel[1, 0, 0, 0] = 1.                       # K_writes[:, head 1, 0] = k_author[:, 1, 0]
        conv.p_rel['__'.join(AWP)][0, 1] = 4.

    def call(conv, t):
        return {'out': conv(t, eis)}

    rec = run(conv, x, call)
    assert list(rec['out']) == ['paper']
    through = {'author': (slice(None), 0), 'kqv_lin.lins.author.weight': R,
               'kqv_lin.lins.author.bias': R,
               'k_rel.weight': (torch.tensor([1 * T + 0, 1 * T + 1]), slice(None), 0)}
    rec.update(cls='HGTConv', kwargs=kw, x_dict=x, edge_index_dict=eis, masked=masked, seed=seed)
    return finish(rec, through, ['kqv_lin.lins.author.weight'])


def main():
    cases = {'transformer': transformer_case(7301), 'transformer_edge': transformer_case(7302, 3),
             'gatv2': gatv2_case(7303), 'hgt': hgt_case(7304)}
    for name in ('transformer', 'transformer_edge', 'gatv2'):
        c = cases[name]
        ei, alpha = c['attention']
        m = c['masked'][ei[0]]
        assert bool(m.any()) and bool((alpha[m, 1] == 0).all()), name
        assert bool((alpha[m][:, [0, 2, 3]] > 0).all()) and bool(c['out'].isfinite().all()), name
    assert bool(cases['hgt']['out']['paper'].isfinite().all())
    path = os.path.join(HERE, 'golden_attn_nonfinite_v1.pt')
    torch.save({'cases': cases, 'torch': torch.__version__,
                'reference': torch_geometric.__version__}, path)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
