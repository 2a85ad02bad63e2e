"""The restatement of the propagation step, of the recurrence and of the six layers built on them
(APPNP, SGConv, SSGConv, TAGConv, LGConv, GCN2Conv) in a chosen dtype, and the checks of
tests/golden/golden_hops_v1.pt that test_hops_host.py and test_gpu_hops.py share.  Plain torch on
the edge list in the order it is given: ``index_add_`` over the destinations."""
import math
import os

import torch

from _util import assert_close_scaled

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_hops_v1.pt')

# every case of the golden file, and per case the hops its LAST call makes on the fused route with
# edge weights that take no gradient (None: the case takes the generic route whatever the weights)
CASES = {
    'appnp': 10, 'appnp_k1': 1, 'appnp_given': 3, 'appnp_given_norm': 3, 'appnp_no_loops': 10,
    'appnp_cached': 10, 'appnp_mean': None,
    'sg_k1': 1, 'sg_k3': 3, 'sg_k3_wide': 3, 'sg_cached': 0, 'sg_no_bias': 3, 'sg_mean': None,
    'ssg_k1': 1, 'ssg_k3': 3, 'ssg_k3_wide': 3, 'ssg_cached': 0, 'ssg_no_bias': 3,
    'ssg_mean': None,
    'tag_k0': 0, 'tag_k3': 3, 'tag_k3_wide': 3, 'tag_given': 3, 'tag_no_bias': 2, 'tag_mean': None,
    'lg': 1, 'lg_given': 1, 'lg_given_raw': 1,
    'gcn2_shared': 1, 'gcn2_separate': 1, 'gcn2_theta': 1, 'gcn2_theta_separate': 1,
    'gcn2_x0_rows': 1, 'gcn2_cached': 1,
}
FUSED_CASES = {k: v for k, v in CASES.items() if v is not None}
STACK_HOPS = 2 + 2 + 3          # TAGConv K = 2, SGConv K = 2, APPNP K = 3

_G = None


def load_golden():
    global _G
    if _G is None:
        _G = torch.load(GOLDEN, weights_only=False)
    return _G


# ---- the step and the recurrence -------------------------------------------------------------------
def step(ei, w, x, n_dst, a=1.0, y=None, b=0.0, z=None, c=0.0, reduce='sum'):
    """``a * sum_{(j -> i)} w_e x[j] (+ b y) (+ c z)`` in the dtype of ``x``"""
    src, dst = ei[0].long(), ei[1].long()
    msg = x[src] if w is None else w.to(x.dtype).view(-1, 1) * x[src]
    t = torch.zeros(n_dst, x.size(1), dtype=x.dtype, device=x.device).index_add_(0, dst, msg)
    if reduce == 'mean':
        t = t / torch.bincount(dst, minlength=n_dst).clamp(min=1).to(x.dtype).view(-1, 1)
    out = a * t
    if y is not None:
        out = out + b * y
    if z is not None:
        out = out + c * z
    return out


def recurrence(ei, w, x, h, K, a, b, d0=0.0, d=0.0, reduce='sum'):
    """``(x_K, s)`` of ``x_k = a A x_{k-1} + b h``, ``s = d0 x_0 + d (x_1 + ... + x_K)``"""
    s = d0 * x
    for _ in range(K):
        x = step(ei, w, x, x.size(0), a, y=h, b=b, reduce=reduce)
        s = s + d * x
    return x, s


def gcn_norm(ei, w, n, add_self_loops, dtype):
    """``D^-1/2 (A + I) D^-1/2`` with the remaining self-loops of weight 1 appended
    (torch_geometric/nn/conv/gcn_conv.py:45-113), flow source_to_target"""
    src, dst = ei[0].long(), ei[1].long()
    w = torch.ones(src.numel(), dtype=dtype, device=ei.device) if w is None else w.to(dtype)
    if add_self_loops:
        keep = src != dst
        loop_w = torch.ones(n, dtype=dtype, device=ei.device)
        loop_w[src[~keep]] = w[~keep]
        loops = torch.arange(n, device=ei.device)
        src, dst = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
        w = torch.cat([w[keep], loop_w])
    deg = torch.zeros(n, dtype=dtype, device=ei.device).index_add_(0, dst, w)
    inv = deg.pow(-0.5)
    inv = torch.where(torch.isinf(inv), torch.zeros_like(inv), inv)
    return torch.stack([src, dst]), inv[src] * w * inv[dst]


# ---- the layers ------------------------------------------------------------------------------------
class Restated:
    """One layer object of the restatement: the constructor arguments, the parameters in a dtype
    (leaves that take gradients) and what ``cached`` keeps between calls."""

    def __init__(self, cls, kwargs, state, dtype):
        self.cls, self.kw, self.dtype = cls, dict(kwargs), dtype
        self.p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in state.items()}
        self.reduce = {'add': 'sum'}.get(self.kw.get('aggr', 'add'), self.kw.get('aggr', 'add'))
        self.cache = None

    def _norm(self, x, ei, w, add_self_loops):
        return gcn_norm(ei, w, x.size(0), add_self_loops, self.dtype)

    def _lin(self, x, prefix='lin'):
        out = x @ self.p[f'{prefix}.weight'].t()
        bias = self.p.get(f'{prefix}.bias')
        return out if bias is None else out + bias

    def __call__(self, x, ei, w=None, x_0=None):
        kw, n = self.kw, x.size(0)
        loops = kw.get('add_self_loops', True)
        if self.cls in ('APPNP', 'GCN2Conv'):
            if kw.get('normalize', True):
                if self.cache is None:
                    ei, w = self._norm(x, ei, w, loops)
                    if kw.get('cached'):
                        self.cache = (ei, w)
                else:
                    ei, w = self.cache
            if self.cls == 'APPNP':
                alpha = kw['alpha']
                return recurrence(ei, w, x, x, kw['K'], 1 - alpha, alpha, reduce=self.reduce)[0]
            alpha, beta = kw['alpha'], 1.0
            if kw.get('theta') is not None:
                beta = math.log(kw['theta'] / kw['layer'] + 1)
            h = step(ei, w, x, n, reduce=self.reduce) * (1 - alpha)
            h0 = alpha * x_0[:n]
            if 'weight2' not in self.p:
                h = h + h0
                return (1 - beta) * h + beta * (h @ self.p['weight1'])
            return ((1 - beta) * h + beta * (h @ self.p['weight1'])
                    + (1 - beta) * h0 + beta * (h0 @ self.p['weight2']))
        if self.cls in ('SGConv', 'SSGConv'):
            if self.cache is not None:
                return self._lin(self.cache.detach())
            ei, w = self._norm(x, ei, w, loops)
            K = kw.get('K', 1)
            if self.cls == 'SGConv':
                h = recurrence(ei, w, x, None, K, 1.0, 0.0, reduce=self.reduce)[0]
            else:
                alpha = kw['alpha']
                h = recurrence(ei, w, x, None, K, 1.0, 0.0, alpha, (1 - alpha) / K,
                               reduce=self.reduce)[1]
            if kw.get('cached') and (K > 0 or self.cls == 'SSGConv'):
                self.cache = h
            return self._lin(h)
        if self.cls == 'TAGConv':
            if kw.get('normalize', True):
                ei, w = self._norm(x, ei, w, False)
            out = x @ self.p['lins.0.weight'].t()
            for k in range(1, kw.get('K', 3) + 1):
                x = step(ei, w, x, n, reduce=self.reduce)
                out = out + x @ self.p[f'lins.{k}.weight'].t()
            return out if 'bias' not in self.p else out + self.p['bias']
        assert self.cls == 'LGConv'
        if kw.get('normalize', True):
            ei, w = self._norm(x, ei, w, False)
        return step(ei, w, x, n, reduce=self.reduce)


def _inputs(G, case, call, dtype, device, weight_grad=True):
    """The leaves of one call: ``{'x', 'x_0'?, 'edge_weight'?}`` and the edge list"""
    opt = case['options']
    width = opt.get('width', G['meta']['K'])
    x = G['x' if call == 0 else 'x2'][:, :width].to(device=device, dtype=dtype)
    leaves = {'x': x.clone().requires_grad_(True)}
    if case['cls'] == 'GCN2Conv':
        x_0 = G['x_0'][:opt.get('x0_rows', G['meta']['N'])].to(device=device, dtype=dtype)
        leaves['x_0'] = x_0.clone().requires_grad_(True)
    if opt.get('weights'):
        leaves['edge_weight'] = (G['edge_weight'].to(device=device, dtype=dtype).clone()
                                 .requires_grad_(weight_grad))
    ei = G['edge_index'] if call == 0 else G['edge_index'].flip(0)
    return leaves, ei.to(device)


def _compare(rec, out, grads, names, tol, what, skip=()):
    assert_close_scaled(out, rec['out'], tol=tol, what=f'{what} out')
    for name, g in zip(names, grads):
        want = rec[f'grad {name}']
        if name in skip:
            continue
        if want is None:
            assert g is None or not bool(g.any()), f'{what}: grad {name} should be absent'
        else:
            assert g is not None, f'{what}: grad {name} is missing'
            assert_close_scaled(g, want, tol=tol, what=f'{what} grad {name}')


def check_restatement_case(G, name, dtype=torch.float64, tol=1e-5):
    """The restatement in ``dtype`` reproduces the golden case: outputs and every gradient"""
    case = G['cases'][name]
    layer = Restated(case['cls'], case['kwargs'], case['state'], dtype)
    for call, rec in enumerate(case['calls']):
        leaves, ei = _inputs(G, case, call, dtype, 'cpu')
        out = layer(leaves['x'], ei, leaves.get('edge_weight'), leaves.get('x_0'))
        params = {f'param {k}': v for k, v in layer.p.items()}
        grads = torch.autograd.grad(out, list(leaves.values()) + list(params.values()),
                                    rec['grad_out'].to(dtype), allow_unused=True)
        _compare(rec, out, grads, list(leaves) + list(params), tol, f'{name} call {call}')


def make_layer(case):
    """This package's class of a golden case with the reference's state dict loaded, strict"""
    from pytorch_geometric_amd import nn
    layer = getattr(nn, case['cls'])(**case['kwargs'])
    assert sorted(layer.state_dict()) == sorted(case['state'])
    layer.load_state_dict(case['state'], strict=True)
    return layer


def check_class_case(G, name, device, index_dtype=torch.int64, tol=1e-5, weight_grad=True,
                     fuse=None, routes=None):
    """This package's class reproduces the golden case on ``device``: ``repr``, outputs and every
    gradient of every call.  ``weight_grad=False``: the given edge weights take no gradient (the
    fused route's condition) and theirs is not compared.  ``routes``: a list that takes the route
    of every call."""
    case = G['cases'][name]
    layer = make_layer(case)
    assert repr(layer) == case['repr']
    layer = layer.to(device)
    if fuse is not None:
        layer.fuse = fuse
    for call, rec in enumerate(case['calls']):
        leaves, ei = _inputs(G, case, call, torch.float32, device, weight_grad)
        ei = ei.to(index_dtype)
        args = [leaves['x']] + ([leaves['x_0']] if 'x_0' in leaves else []) + [ei]
        if 'edge_weight' in leaves:
            args.append(leaves['edge_weight'])
        if routes is not None:
            routes.append(layer.hop_route(leaves['x'], ei, leaves.get('edge_weight')))
        out = layer(*args)
        params = {f'param {k}': v for k, v in layer.named_parameters()}
        wanted = [v for v in leaves.values() if v.requires_grad] + list(params.values())
        names = [k for k, v in leaves.items() if v.requires_grad] + list(params)
        grads = torch.autograd.grad(out, wanted, rec['grad_out'].to(device), allow_unused=True)
        _compare(rec, out, grads, names, tol, f'{name} call {call} on {device}')
    return layer


def check_stack(G, device, index_dtype=torch.int64, tol=1e-5, fuse=None):
    """The 3-layer stack with ReLU between the layers"""
    from pytorch_geometric_amd import nn
    S = G['stack']
    layers = []
    for (cls, kw), state in zip(S['layers'], S['state']):
        layer = getattr(nn, cls)(**kw)
        layer.load_state_dict(state, strict=True)
        layer = layer.to(device)
        if fuse is not None:
            layer.fuse = fuse
        layers.append(layer)
    x = G['x'].to(device).clone().requires_grad_(True)
    ei = G['edge_index'].to(device).to(index_dtype)
    h = x
    for i, layer in enumerate(layers):
        h = layer(h, ei)
        if i + 1 < len(layers):
            h = h.relu()
    params = {f'{i}.{n}': p for i, layer in enumerate(layers) for n, p in layer.named_parameters()}
    grads = torch.autograd.grad(h, [x] + list(params.values()), S['grad_out'].to(device))
    assert_close_scaled(h, S['out'], tol=tol, what='stack out')
    assert_close_scaled(grads[0], S['grad x'], tol=tol, what='stack grad x')
    for (n, _), g in zip(params.items(), grads[1:]):
        assert_close_scaled(g, S['grad_params'][n], tol=tol, what=f'stack grad {n}')
    return layers
