"""A restatement of RGATConv in plain tensor code, written from the formulas of the layer (the
reference: torch_geometric/nn/conv/rgat_conv.py:373-529) and differentiable by autograd, in the
dtype of its inputs (the tests run it in float64):

* :func:`rgat_attend`: the node-level form the kernels compute — ``s = leaky_relu(QI[i, r] +
  KJ[j, r] + B[e])``, the softmax over the edges into ``i`` (across-relation) or, by a loop of one
  mask per relation, over those of relation ``r`` (within-relation), ``out[i, h] = sum alpha *
  P[j, r, h]``;
* :func:`rgat_layer`: the whole layer from a state dict, per edge and unsplit: ``outi = x_i W_r``
  and ``outj = x_j W_r`` with the weight of every edge's relation, both attention modes, both
  mechanisms, all four ``mod``.

Also the helpers that run this package's class against the recorded cases of
tests/golden/golden_rgat_v1.pt."""
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_rgat_v1.pt')

CASES = ('default', 'heads2', 'heads3_mean', 'within', 'no_bias', 'bases2', 'blocks2', 'edge5',
         'mod_additive', 'mod_scaled', 'mod_f_additive', 'mod_f_scaled', 'mult_dim2',
         'mult_dim2_edge')
# the cases whose conditions the fused route serves (the routing tests pin this list)
FUSED_CASES = ('default', 'heads2', 'heads3_mean', 'within', 'no_bias', 'bases2', 'blocks2', 'edge5',
               'mod_scaled', 'mod_f_scaled')


def group_softmax(s, key, n):
    """softmax of ``s [E, ...]`` over the rows with equal ``key`` (``< n``): the maximum (detached)
    subtracted, ``1e-16`` on the denominator, as torch_geometric/utils/_softmax.py:82-88"""
    key = key.long()
    where = key.view(-1, *[1] * (s.dim() - 1)).expand_as(s)
    top = s.new_full((n, ) + s.shape[1:], float('-inf')).scatter_reduce(
        0, where, s.detach(), 'amax', include_self=True)
    num = (s - top.index_select(0, key)).exp()
    den = s.new_zeros((n, ) + s.shape[1:]).index_add(0, key, num) + 1e-16
    return num / den.index_select(0, key)


def mechanism_softmax(s, dst, rel, n_dst, R, within):
    if not within:
        return group_softmax(s, dst, n_dst)
    alpha = torch.zeros_like(s)
    for r in range(R):   # one mask per relation
        mask = rel == r
        if bool(mask.any()):
            alpha = alpha.index_put((mask.nonzero().view(-1), ),
                                    group_softmax(s[mask], dst[mask], n_dst))
    return alpha


def rgat_scores(QI, KJ, B, src, dst, rel):
    """the pre-activations ``[E, H]``; ``QI`` / ``KJ`` are ``[N, R, H]``"""
    t = QI[dst.long(), rel.long()] + KJ[src.long(), rel.long()]
    return t if B is None else t + B


def rgat_attend(P, QI, KJ, B, src, dst, rel, n_dst, H, C, slope=0.2, within=False):
    """``(out [n_dst, H * C], alpha [E, H])`` from ``P [N, R * H * C]``, ``QI`` / ``KJ [N, R * H]``
    and the optional ``B [E, H]``, everything in edge order"""
    R = P.size(1) // (H * C)
    src, dst, rel = src.long(), dst.long(), rel.long()
    t = rgat_scores(QI.view(-1, R, H), KJ.view(-1, R, H), B, src, dst, rel)
    s = torch.where(t > 0, t, t * slope)
    alpha = mechanism_softmax(s, dst, rel, n_dst, R, within)
    rows = P.view(-1, R, H, C)[src, rel]
    out = P.new_zeros(n_dst, H, C).index_add(0, dst, alpha.unsqueeze(-1) * rows)
    return out.view(n_dst, H * C), alpha


def dense_weight(state, cfg):
    """``[R, in, H C]`` from the state dict's ``weight`` or ``att`` / ``basis``"""
    R, W = cfg['num_relations'], cfg.get('heads', 1) * cfg['out_channels']
    if cfg.get('num_bases') is not None:
        return torch.einsum('rb,biw->riw', state['att'], state['basis'])
    w = state['weight']
    if cfg.get('num_blocks') is not None:
        nb, bi, bo = w.shape[1:]
        full = w.new_zeros(R, nb * bi, nb * bo)
        for b in range(nb):
            full[:, b * bi:(b + 1) * bi, b * bo:(b + 1) * bo] = w[:, b]
        return full
    assert w.shape[2] == W
    return w


def rgat_layer(state, cfg, x, edge_index, edge_type, edge_attr=None, n_dst=None):
    """``(out, alpha, margin)`` of the layer with the reference's parameter names, per edge and
    unsplit.  ``margin``: the least distance of a kinked pre-activation from its kink (the leaky
    ReLU's argument, the ReLU of ``mod='scaled'``)."""
    H, C, R = cfg.get('heads', 1), cfg['out_channels'], cfg['num_relations']
    D = cfg.get('dim', 1)
    additive = cfg.get('attention_mode', 'additive-self-attention') == 'additive-self-attention'
    within = cfg.get('attention_mechanism', 'across-relation') == 'within-relation'
    mod, concat = cfg.get('mod'), cfg.get('concat', True)
    src, dst, rel = edge_index[0].long(), edge_index[1].long(), edge_type.long()
    n = x.size(0) if n_dst is None else n_dst
    w = dense_weight(state, cfg)[rel]                                   # [E, in, H C]
    outi = torch.bmm(x[dst].unsqueeze(1), w).squeeze(1)
    outj = torch.bmm(x[src].unsqueeze(1), w).squeeze(1)
    qi, kj = outi @ state['q'], outj @ state['k']
    margin = float('inf')
    if edge_attr is not None:
        ea = edge_attr.view(-1, 1) if edge_attr.dim() == 1 else edge_attr
        edge = (ea @ state['lin_edge.weight'].t()) @ state['e']
        t = qi + kj + edge if additive else (qi * kj) * edge
    else:
        t = qi + kj if additive else qi * kj
    if additive:
        if t.numel():
            margin = min(margin, float(t.detach().abs().min()))
        t = torch.where(t > 0, t, t * cfg.get('negative_slope', 0.2))
    alpha = mechanism_softmax(t, dst, rel, n, R, within)
    deg = torch.bincount(dst, minlength=n).to(x.dtype)
    heads = outj.view(-1, H, C) if additive else outj.view(-1, H, 1, C)
    score = alpha.view(-1, H, 1) if additive else alpha.view(-1, H, D, 1)
    if mod == 'additive':
        msg = heads * score + state['w'] * (heads * torch.ones_like(score))
    elif mod == 'scaled':
        pre = deg[dst].view(-1, 1) @ state['l1'] + state['b1']
        if pre.numel():
            margin = min(margin, float(pre.detach().abs().min()))
        psi = torch.relu(pre) @ state['l2'] + state['b2']
        msg = (heads * score) * (psi.view(-1, 1, C) if additive else psi.view(-1, 1, 1, C))
    elif mod == 'f-additive':
        a = torch.where(alpha > 0, alpha + 1, alpha)
        msg = heads * (a.view(-1, H, 1) if additive else a.view(-1, H, D, 1))
    elif mod == 'f-scaled':
        a = alpha * deg[dst].view(-1, 1)
        msg = heads * (a.view(-1, H, 1) if additive else a.view(-1, H, D, 1))
    else:
        msg = heads * score
    out = msg.new_zeros((n, ) + msg.shape[1:]).index_add(0, dst, msg)
    if concat:
        out = out.reshape(n, -1)
    else:
        out = out.mean(dim=1).reshape(n, -1)
    if state.get('bias') is not None:
        out = out + state['bias']
    return out, alpha, margin


# ---- the recorded cases ---------------------------------------------------------------------------
def load_golden():
    return torch.load(GOLDEN, map_location='cpu', weights_only=True)


def make_layer(case):
    from pytorch_geometric_amd.nn import RGATConv
    layer = RGATConv(**case['cfg'])
    assert list(layer.state_dict()) == list(case['state'])
    layer.load_state_dict(case['state'], strict=True)
    layer.fuse = True    # the fused route wherever its conditions hold, whatever the switch says
    return layer.train()


def case_inputs(G, case, device, index_dtype=torch.int64, dtype=torch.float32):
    """``(x, edge_index, edge_type, edge_attr | None)`` of a recorded case as fresh leaves"""
    x = G['x'].detach().clone().to(device, dtype).requires_grad_(True)
    ei = G['edge_index'].to(device).to(index_dtype)
    et = G['edge_type'].to(device).to(index_dtype)
    ea = None
    if case['cfg'].get('edge_dim') is not None:
        ea = G['edge_attr'].detach().clone().to(device, dtype).requires_grad_(True)
    return x, ei, et, ea


def _compare(name, case, out, alpha, grads, n_in, names):
    """every recorded tensor at the project's 2e-5 relative to the tensor's scale
    (``assert_close_scaled``): the records are float32 results themselves, two of the cases
    multiply by in-degrees up to 30, and gradient entries cancel"""
    from _util import assert_close_scaled
    assert_close_scaled(out, case['out'], what=f'{name} out')
    assert_close_scaled(alpha, case['alpha'], what=f'{name} alpha')
    for g, ref, what in zip(grads[:n_in], case['grad_in'], ('grad_x', 'grad_edge_attr')):
        assert_close_scaled(g, ref, what=f'{name} {what}')
    for n, g in zip(names, grads[n_in:]):
        assert_close_scaled(g, case['grad_params'][n], what=f'{name} grad {n}')


def check_restatement_case(G, name):
    """The restatement in float32 against one recorded case, at ``check_class_case``'s bound"""
    case = G['cases'][name]
    x, ei, et, ea = case_inputs(G, case, 'cpu')
    state = {k: v.detach().clone().requires_grad_(True) for k, v in case['state'].items()}
    out, alpha, _ = rgat_layer(state, case['cfg'], x, ei, et, ea)
    names = list(case['grad_params'])
    ins = [x] + ([] if ea is None else [ea])
    grads = torch.autograd.grad(out, ins + [state[n] for n in names], case['grad_out'])
    _compare(name, case, out, alpha, grads, len(ins), names)


def check_class_case(G, name, device, index_dtype=torch.int64):
    """This package's class with the reference's state dict against one recorded case: ``out``,
    ``alpha`` (in the caller's edge order), the input gradients and the gradient of every
    parameter the case reaches at 2e-5 of the tensor's scale (``_compare``)."""
    case = G['cases'][name]
    layer = make_layer(case).to(device)
    x, ei, et, ea = case_inputs(G, case, device, index_dtype)
    out, (ei_back, alpha) = layer(x, ei, et, ea, return_attention_weights=True)
    assert ei_back is ei
    names = list(case['grad_params'])
    params = dict(layer.named_parameters())
    ins = [x] + ([] if ea is None else [ea])
    grads = torch.autograd.grad(out, ins + [params[n] for n in names],
                                case['grad_out'].to(device), allow_unused=True)
    assert all(g is not None for g in grads), name
    _compare(name, case, out, alpha, grads, len(ins), names)
    return layer


def make_stack(G):
    from pytorch_geometric_amd.nn import RGATConv
    layers = torch.nn.ModuleList([RGATConv(**cfg) for cfg in G['stack']['cfgs']])
    for layer in layers:   # (as make_layer)
        layer.fuse = True
    return layers


def check_stack(G, device, index_dtype=torch.int64):
    """The two-layer stack against its record, relative to each tensor's scale at the project's
    2e-5 (``assert_close_scaled``, the bound of deep-model gradients)."""
    from _util import assert_close_scaled
    case = G['stack']
    layers = make_stack(G)
    assert list(layers.state_dict()) == list(case['state'])
    layers.load_state_dict(case['state'], strict=True)
    layers = layers.to(device)
    x = G['x'].detach().clone().to(device).requires_grad_(True)
    ei = G['edge_index'].to(device).to(index_dtype)
    et = G['edge_type'].to(device).to(index_dtype)
    out = layers[1](torch.relu(layers[0](x, ei, et)), ei, et)
    names = list(case['grad_params'])
    params = dict(layers.named_parameters())
    grads = torch.autograd.grad(out, [x] + [params[n] for n in names],
                                case['grad_out'].to(device))
    assert_close_scaled(out, case['out'], what='stack out')
    assert_close_scaled(grads[0], case['grad_in'][0], what='stack grad_x')
    for n, g in zip(names, grads[1:]):
        assert_close_scaled(g, case['grad_params'][n], what=f'stack grad {n}')
    return layers
