"""ResGatedGraphConv: what the host and the GPU tests share.  The recorded reference cases of
tests/golden/golden_resgated_v1.pt (tests/golden/make_golden_resgated.py) and the torch restatement
of the aggregate in the dtype of its inputs, in the reference's UNSPLIT form (``cat`` then
``Linear`` per edge, res_gated_graph_conv.py:143-148), so that the split of every ``Linear`` into
node and edge columns the kernels of csrc/resgated.hip rest on is itself under test:

    out[i] = sum_{k: dst_k = i} act(key_k + query_k) * value_k
    key_k = lin_key(cat[k[dst_k], a_k]),  query_k = lin_query(cat[q[src_k], a_k]),  value_k alike
"""
import os

import torch

CASES = ['defaults', 'no_root', 'no_bias', 'wider_out', 'edge_dim', 'pair', 'pair_edge_dim',
         'tanh', 'mean']
FUSED_CASES = [c for c in CASES if c not in ('tanh', 'mean')]

_GOLDEN = []


def load_golden():
    """tests/golden/golden_resgated_v1.pt, loaded once and never modified."""
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_resgated_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


def _lin(x, wb):
    w, b = wb
    out = x @ w.t()
    return out if b is None else out + b


def resgated_aggregate(k, q, v, edge_attr, lins, edge_index, n_dst, act=torch.sigmoid,
                       mean=False, flow='source_to_target'):
    """The aggregate in the dtype of its inputs.  ``edge_attr=None``: ``k``, ``q``, ``v`` are the
    node-level key, query and value; otherwise they are what the three ``Linear`` of ``lins =
    ((Wk, bk), (Wq, bq), (Wv, bv))`` read next to ``edge_attr``, with ``W [F, width + De]``."""
    j, i = (0, 1) if flow == 'source_to_target' else (1, 0)
    src, dst = edge_index[j].long(), edge_index[i].long()
    k_i, q_j, v_j = k[dst], q[src], v[src]
    if edge_attr is not None:
        k_i = _lin(torch.cat([k_i, edge_attr], dim=-1), lins[0])
        q_j = _lin(torch.cat([q_j, edge_attr], dim=-1), lins[1])
        v_j = _lin(torch.cat([v_j, edge_attr], dim=-1), lins[2])
    msg = act(k_i + q_j) * v_j
    out = msg.new_zeros(n_dst, msg.size(1)).index_add(0, dst, msg)
    if mean:
        out = out / torch.bincount(dst, minlength=n_dst).clamp(min=1).to(out.dtype).view(-1, 1)
    return out


def resgated_layer(state, x_src, x_dst, edge_attr, edge_index, act=torch.sigmoid, mean=False,
                   flow='source_to_target'):
    """The whole layer from a state dict (the reference's keys), in the dtype of its tensors"""
    lins = [(state[f'lin_{n}.weight'], state.get(f'lin_{n}.bias'))
            for n in ('key', 'query', 'value')]
    if edge_attr is None:
        k, q, v = _lin(x_dst, lins[0]), _lin(x_src, lins[1]), _lin(x_src, lins[2])
    else:
        k, q, v = x_dst, x_src, x_src
    n_dst = x_dst.size(0)
    out = resgated_aggregate(k, q, v, edge_attr, lins, edge_index, n_dst, act, mean, flow)
    if 'lin_skip.weight' in state:
        out = out + x_dst @ state['lin_skip.weight'].t()
    if 'bias' in state:
        out = out + state['bias']
    return out


def _act(case):
    return None if case['act'] is None else getattr(torch.nn, case['act'])()


def make_layer(case):
    from pytorch_geometric_amd.nn import ResGatedGraphConv
    extra = {} if case['act'] is None else {'act': _act(case)}
    layer = ResGatedGraphConv(case['in_channels'], case['out_channels'], **case['kwargs'], **extra)
    assert list(layer.state_dict()) == list(case['state'])
    layer.load_state_dict(case['state'], strict=True)
    return layer


def case_inputs(G, case, device, index_dtype=torch.int64, dtype=torch.float32):
    """``(xs, edge_index, edge_attr | None)`` of a recorded case as fresh leaves on ``device``"""
    pair = case['mode'] == 'pair'
    xs = [G['x'].detach().clone().to(device, dtype).requires_grad_(True)]
    if pair:
        width = case['in_channels'][1]
        xs.append(G['x_dst'][:, :width].detach().clone().to(device, dtype).requires_grad_(True))
    ei = (G['edge_index_pair'] if pair else G['edge_index']).to(device).to(index_dtype)
    ea = None
    if 'edge_attr' in case:
        ea = case['edge_attr'].detach().clone().to(device, dtype).requires_grad_(True)
    return xs, ei, ea


def check_restatement_case(G, name):
    """The restatement in float32 against one recorded case, at ``check_class_case``'s bounds"""
    case = G['cases'][name]
    xs, ei, ea = case_inputs(G, case, 'cpu')
    state = {k: v.detach().clone().requires_grad_(True) for k, v in case['state'].items()}
    act = torch.sigmoid if case['act'] is None else _act(case)
    out = resgated_layer(state, xs[0], xs[-1], ea, ei, act=act,
                         mean=case['kwargs'].get('aggr') == 'mean')
    leaves = xs + ([] if ea is None else [ea])
    names = list(case['grad_params'])
    grads = torch.autograd.grad(out, leaves + [state[n] for n in names], case['grad_out'])
    _compare(name, case, out, grads, len(xs), ea is not None, names)


def _compare(name, case, out, grads, n_x, has_ea, names):
    from _util import assert_close
    assert_close(out, case['out'], what=f'{name} out')
    for g, ref in zip(grads[:n_x], case['grad_x']):
        assert_close(g, ref, what=f'{name} grad_x')
    if has_ea:
        assert_close(grads[n_x], case['grad_edge_attr'], what=f'{name} grad_edge_attr')
    for n, g in zip(names, grads[n_x + int(has_ea):]):
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'{name} grad {n}')


def check_class_case(G, name, device, index_dtype=torch.int64):
    """This package's class with the reference's state dict against one recorded case: ``out``,
    ``grad_x`` and ``grad_edge_attr`` at 1e-5, parameter gradients at 5e-5 (the tolerances of
    ``_gen_ref.check_class_case``)."""
    case = G['cases'][name]
    layer = make_layer(case).to(device)
    xs, ei, ea = case_inputs(G, case, device, index_dtype)
    out = layer(xs[0] if len(xs) == 1 else (xs[0], xs[1]), ei, edge_attr=ea)
    params = [(n, p) for n, p in layer.named_parameters() if p.requires_grad]
    assert [n for n, _ in params] == list(case['grad_params']), name
    leaves = xs + ([] if ea is None else [ea])
    grads = torch.autograd.grad(out, leaves + [p for _, p in params], case['grad_out'].to(device))
    _compare(name, case, out, grads, len(xs), ea is not None, [n for n, _ in params])
    return layer


def make_stack():
    from pytorch_geometric_amd.nn import ResGatedGraphConv
    return torch.nn.ModuleList([ResGatedGraphConv(16, 24, edge_dim=3), ResGatedGraphConv(24, 16)])


def check_stack(G, device, index_dtype=torch.int64):
    from _util import assert_close
    case = G['stack']
    layers = make_stack()
    assert list(layers.state_dict()) == list(case['state'])
    layers.load_state_dict(case['state'], strict=True)
    layers = layers.to(device)
    x = G['x'].detach().clone().to(device).requires_grad_(True)
    ea = case['edge_attr'].detach().clone().to(device).requires_grad_(True)
    ei = G['edge_index'].to(device).to(index_dtype)
    h = layers[1](layers[0](x, ei, edge_attr=ea).relu(), ei)
    params = [(n, p) for n, p in layers.named_parameters() if p.requires_grad]
    assert [n for n, _ in params] == list(case['grad_params'])
    grads = torch.autograd.grad(h, [x, ea] + [p for _, p in params], case['grad_out'].to(device))
    assert_close(h, case['out'], what='stack out')
    assert_close(grads[0], case['grad_x'][0], atol=5e-5, rtol=5e-5, what='stack grad_x')
    assert_close(grads[1], case['grad_edge_attr'], atol=5e-5, rtol=5e-5,
                 what='stack grad_edge_attr')
    for (n, _), g in zip(params, grads[2:]):
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'stack grad {n}')
    return layers
