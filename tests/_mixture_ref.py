"""GMMConv and NNConv: what the host and the GPU tests share.  The recorded reference cases of
tests/golden/golden_mixture_v1.pt (tests/golden/make_golden_mixture.py) and torch restatements in
the dtype of their inputs, all in the reference's own MESSAGE-FIRST order (transform every edge's
row, weight it, then sum per destination: gmm_conv.py:154-165, nn_conv.py:119-122), so that they
are independent of the aggregate-first reordering that csrc/mixture.hip and
``MixtureConvFunction`` rest on:

    expand:       Z[i, k, :] = sum_{e: dst_e = i} coef[e, k] * x[src_e, :]
    coef_grad:    grad_coef[e, k] = <wide[dst_e, k, :], x[src_e, :]>
    mixture_conv: out[i] = sum_{e: dst_e = i} sum_k coef[e, k] * (x[src_e] @ weight[k])
"""
import os

import torch

GMM_CASES = ['gmm_defaults', 'gmm_add', 'gmm_no_root', 'gmm_no_bias', 'gmm_wider_out', 'gmm_pair',
             'gmm_separate', 'gmm_max']
NN_CASES = ['nn_linear', 'nn_mlp', 'nn_last_no_bias', 'nn_mean', 'nn_pair', 'nn_max',
            'nn_ends_relu']
CASES = GMM_CASES + NN_CASES
GENERIC_CASES = ['gmm_separate', 'gmm_max', 'nn_max', 'nn_ends_relu']
FUSED_CASES = [c for c in CASES if c not in GENERIC_CASES]

_GOLDEN = []


def load_golden():
    """tests/golden/golden_mixture_v1.pt, loaded once and never modified."""
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'golden_mixture_v1.pt')
        _GOLDEN.append(torch.load(path, map_location='cpu', weights_only=False))
    return _GOLDEN[0]


# ---- the kernels' contracts ------------------------------------------------------------------------
def expand(x, coef, src, dst, n_rows):
    """``Z [n_rows, K * F]``; ``coef [E, K]`` in the order of ``src`` / ``dst``"""
    msg = coef.unsqueeze(2) * x[src.long()].unsqueeze(1)                     # [E, K, F]
    z = msg.new_zeros(n_rows, coef.size(1), x.size(1)).index_add(0, dst.long(), msg)
    return z.reshape(n_rows, -1)


def coef_grad(wide, x, src, dst):
    """``grad_coef [E, K]`` for ``wide [n_rows, K * F]``"""
    F = x.size(1)
    return (wide[dst.long()].view(dst.numel(), -1, F) * x[src.long()].unsqueeze(1)).sum(-1)


def mixture_conv(x, coef, weight, src, dst, n_dst):
    """``out [n_dst, M]``, message first: every edge's row through all ``K`` maps ``weight [K, F,
    M]``, mixed with its coefficients, then the sum per destination"""
    per_map = torch.einsum('ef,kfm->ekm', x[src.long()], weight)             # [E, K, M]
    msg = (per_map * coef.unsqueeze(2)).sum(1)
    return msg.new_zeros(n_dst, weight.size(2)).index_add(0, dst.long(), msg)


# ---- the layers ------------------------------------------------------------------------------------
def _aggregate(msg, dst, n_dst, aggr):
    dst = dst.long()
    if aggr == 'max':
        index = dst.view(-1, 1).expand_as(msg)
        return msg.new_zeros(n_dst, msg.size(1)).scatter_reduce(0, index, msg, 'amax',
                                                                include_self=False)
    out = msg.new_zeros(n_dst, msg.size(1)).index_add(0, dst, msg)
    if aggr == 'mean':
        out = out / torch.bincount(dst, minlength=n_dst).clamp(min=1).to(out.dtype).view(-1, 1)
    return out


def gmm_layer(state, x_src, x_dst, edge_attr, edge_index, kernel_size, aggr='mean',
              separate=False):
    """``GMMConv.forward`` from a state dict (the reference's keys), in the dtype of its tensors"""
    EPS = 1e-15
    src, dst = edge_index[0].long(), edge_index[1].long()
    g, mu, sigma = state['g'], state['mu'], state['sigma']
    F, K = g.size(0), kernel_size
    M = g.size(1) // K
    (E, D) = edge_attr.shape
    if not separate:
        w = -0.5 * (edge_attr.view(E, 1, D) - mu.view(1, K, D)).pow(2)
        w = torch.exp((w / (EPS + sigma.view(1, K, D).pow(2))).sum(-1))      # [E, K]
        msg = ((x_src @ g)[src].view(E, K, M) * w.view(E, K, 1)).sum(-2)
    else:
        w = -0.5 * (edge_attr.view(E, 1, 1, 1, D) - mu.view(1, F, M, K, D)).pow(2)
        w = torch.exp((w / (EPS + sigma.view(1, F, M, K, D).pow(2))).sum(-1))
        w = (w * g.view(1, F, M, K)).sum(-1)                                  # [E, F, M]
        msg = (x_src[src].view(E, F, 1) * w).sum(-2)
    out = _aggregate(msg, dst, x_dst.size(0), aggr)
    if 'root.weight' in state:
        out = out + x_dst @ state['root.weight'].t()
    if 'bias' in state:
        out = out + state['bias']
    return out


def edge_network(state, spec, edge_attr):
    """the edge network of an NNConv state dict; ``spec``: ``('Linear', in, out, bias)`` /
    ``('ReLU', )`` entries"""
    h = edge_attr
    for i, entry in enumerate(spec):
        key = 'nn' if len(spec) == 1 else f'nn.{i}'
        if entry[0] == 'Linear':
            h = h @ state[f'{key}.weight'].t()
            if entry[3]:
                h = h + state[f'{key}.bias']
        else:
            h = torch.relu(h)
    return h


def nn_layer(state, spec, x_src, x_dst, edge_attr, edge_index, out_channels, aggr='add'):
    """``NNConv.forward`` from a state dict, in the dtype of its tensors"""
    src, dst = edge_index[0].long(), edge_index[1].long()
    F = x_src.size(1)
    weight = edge_network(state, spec, edge_attr).view(-1, F, out_channels)
    msg = torch.matmul(x_src[src].unsqueeze(1), weight).squeeze(1)
    out = _aggregate(msg, dst, x_dst.size(0), aggr)
    if 'lin.weight' in state:
        out = out + x_dst @ state['lin.weight'].t()
    if 'bias' in state:
        out = out + state['bias']
    return out


def layer_from_state(case, state, x_src, x_dst, edge_attr, edge_index):
    aggr = case['kwargs'].get('aggr', 'mean' if case['kind'] == 'gmm' else 'add')
    if case['kind'] == 'gmm':
        meta = load_golden()['meta']
        return gmm_layer(state, x_src, x_dst, edge_attr, edge_index, meta['kernel_size'], aggr,
                         case['kwargs'].get('separate_gaussians', False))
    return nn_layer(state, case['nn'], x_src, x_dst, edge_attr, edge_index, case['out_channels'],
                    aggr)


# ---- this package's classes against the recorded cases -----------------------------------------------
def make_edge_network(spec):
    layers = []
    for entry in spec:
        if entry[0] == 'Linear':
            layers.append(torch.nn.Linear(entry[1], entry[2], bias=entry[3]))
        else:
            layers.append(getattr(torch.nn, entry[0])())
    return layers[0] if len(layers) == 1 else torch.nn.Sequential(*layers)


def make_layer(case, fuse=True):
    """this package's layer with the case's state; ``fuse`` sets the per-layer switch, whatever
    the environment says"""
    from pytorch_geometric_amd.nn import GMMConv, NNConv
    if case['kind'] == 'gmm':
        meta = load_golden()['meta']
        layer = GMMConv(case['in_channels'], case['out_channels'], dim=meta['dim'],
                        kernel_size=meta['kernel_size'], **case['kwargs'])
    else:
        layer = NNConv(case['in_channels'], case['out_channels'], make_edge_network(case['nn']),
                       **case['kwargs'])
    assert list(layer.state_dict()) == list(case['state'])
    layer.load_state_dict(case['state'], strict=True)
    layer.fuse = fuse
    return layer


def case_inputs(G, case, device, index_dtype=torch.int64, dtype=torch.float32):
    """``(xs, edge_index, edge_attr)`` of a recorded case as fresh leaves on ``device``"""
    pair = case['mode'] == 'pair'
    xs = [G['x'].detach().clone().to(device, dtype).requires_grad_(True)]
    if pair:
        width = case['in_channels'][1]
        xs.append(G['x_dst'][:, :width].detach().clone().to(device, dtype).requires_grad_(True))
    ei = (G['edge_index_pair'] if pair else G['edge_index']).to(device).to(index_dtype)
    ea = case['edge_attr'].detach().clone().to(device, dtype).requires_grad_(True)
    return xs, ei, ea


def _compare(name, case, out, grads, n_x, names):
    from _util import assert_close
    assert_close(out, case['out'], what=f'{name} out')
    for g, ref in zip(grads[:n_x], case['grad_x']):
        assert_close(g, ref, what=f'{name} grad_x')
    assert_close(grads[n_x], case['grad_edge_attr'], atol=5e-5, rtol=5e-5,
                 what=f'{name} grad_edge_attr')
    for n, g in zip(names, grads[n_x + 1:]):
        assert_close(g, case['grad_params'][n], atol=5e-5, rtol=5e-5, what=f'{name} grad {n}')


def check_restatement_case(G, name):
    """The restatement in float32 against one recorded case, at ``check_class_case``'s bounds"""
    case = G['cases'][name]
    xs, ei, ea = case_inputs(G, case, 'cpu')
    state = {k: v.detach().clone().requires_grad_(True) for k, v in case['state'].items()}
    out = layer_from_state(case, state, xs[0], xs[-1], ea, ei)
    names = list(case['grad_params'])
    grads = torch.autograd.grad(out, xs + [ea] + [state[n] for n in names], case['grad_out'])
    _compare(name, case, out, grads, len(xs), names)


def check_class_case(G, name, device, index_dtype=torch.int64, fuse=True, prepare=None):
    """This package's class with the reference's state dict against one recorded case: ``out`` and
    ``grad_x`` at 1e-5, ``grad_edge_attr`` and the parameter gradients at 5e-5 (sums over all 400
    edges; the tolerances of ``_resgated_ref.check_class_case``).  ``prepare(layer)`` runs before
    the forward."""
    case = G['cases'][name]
    layer = make_layer(case, fuse).to(device)
    if prepare is not None:
        prepare(layer)
    xs, ei, ea = case_inputs(G, case, device, index_dtype)
    out = layer(xs[0] if len(xs) == 1 else (xs[0], xs[1]), ei, edge_attr=ea)
    params = [(n, p) for n, p in layer.named_parameters() if p.requires_grad]
    assert [n for n, _ in params] == list(case['grad_params']), name
    grads = torch.autograd.grad(out, xs + [ea] + [p for _, p in params],
                                case['grad_out'].to(device))
    _compare(name, case, out, grads, len(xs), [n for n, _ in params])
    return layer
