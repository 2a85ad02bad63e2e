"""What the norm tests share (tests/test_norm_host.py, tests/test_gpu_norm.py): the golden
(tests/golden/golden_norm_v1.pt), a float64 restatement of GraphNorm and of LayerNorm over whole
graphs in plain torch (a loop over the graphs: nothing of the code under test), and the runners
of the golden cases on a device.

Tolerance of a tensor compared against float64: ``max(2e-5, 2 x the float32 error of the
reference arithmetic on that tensor)``.  2e-5 is the project's constant.  The second term exists
because the reference in float32 is itself off by up to 1e-5 .. 3e-5 on ``grad_mean_scale`` at the
input offset by 30 (a sum of products of the mean with cancelling gradient sums); the factor 2
covers a different order of summation.  For the golden cases the reference's error is the
recorded ``ref_err``; for restatement cases it is measured by running the restatement in
float32."""
import os

import torch

from tests._util import assert_close_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_G = None


def load_golden():
    global _G
    if _G is None:
        _G = torch.load(os.path.join(ROOT, 'tests', 'golden', 'golden_norm_v1.pt'),
                        map_location='cpu', weights_only=False)
    return _G


def tol_of(ref_err: float) -> float:
    return max(2e-5, 2.0 * ref_err)


def scaled_err(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / max(float(b.abs().max()), 1.0))


# ---- the restatement ---------------------------------------------------------------------------
def ptr_of(sizes, device='cpu', dtype=torch.int64):
    return torch.tensor([0] + list(torch.tensor(sizes).cumsum(0).tolist()), dtype=dtype,
                        device=device)


def batch_of(sizes, device='cpu', dtype=torch.int64):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(
        device=device, dtype=dtype)


def restate(kind, x, sizes, weight=None, bias=None, mean_scale=None, eps=1e-5, no_batch=False):
    """``kind``: 'graph_norm' | 'layer_norm' (graph mode), at the dtype of ``x``; graph by graph.
    ``no_batch``: the formulas the reference uses without a batch vector (one graph)."""
    outs, start = [], 0
    for n in sizes:
        xs = x[start:start + n]
        start += n
        if n == 0:
            continue
        if kind == 'graph_norm':
            u = xs - xs.mean(0, keepdim=True) * (1.0 if mean_scale is None else mean_scale)
            y = u / (u.pow(2).mean(0, keepdim=True) + eps).sqrt()
        else:
            u = xs - xs.mean()
            var = u.pow(2).mean()
            y = u / (var.sqrt() + eps) if no_batch else u / (var + eps).sqrt()
        outs.append(y)
    out = torch.cat(outs) if outs else x[:0]
    if weight is not None:
        out = out * weight
    if bias is not None:
        out = out + bias
    return out


def restate_with_grads(kind, x, sizes, grad_out, params, dtype, **kw):
    """``(out, grad_x, {name: grad})`` of the restatement at ``dtype``; ``params``: name -> tensor"""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    pp = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()
          if v is not None}
    out = restate(kind, xx, sizes, **pp, **kw)
    grads = torch.autograd.grad(out, [xx] + list(pp.values()), grad_out.to(dtype))
    return out.detach(), grads[0], dict(zip(pp, grads[1:]))


def check_against_restatement(layer, kind, x, sizes, batch, grad_out, what, no_batch=False,
                              batch_size=None):
    """``layer`` on ``(x, batch)`` against the float64 restatement on the same device; every
    tensor's tolerance from the float32 restatement's own error.  Returns the figures."""
    params = {n: p for n, p in layer.named_parameters()}
    eps = layer.eps
    r64 = restate_with_grads(kind, x, sizes, grad_out, params, torch.float64, eps=eps,
                             no_batch=no_batch)
    r32 = restate_with_grads(kind, x, sizes, grad_out, params, torch.float32, eps=eps,
                             no_batch=no_batch)
    xx = x.detach().clone().requires_grad_(True)
    layer.zero_grad()
    out = layer(xx) if batch is None else layer(xx, batch, batch_size)
    out.backward(grad_out)
    got = {'out': out, 'grad_x': xx.grad}
    got.update({f'grad_{n}': p.grad for n, p in layer.named_parameters()})
    ref = {'out': (r64[0], r32[0]), 'grad_x': (r64[1], r32[1])}
    ref.update({f'grad_{n}': (r64[2][n], r32[2][n]) for n in r64[2]})
    figures = {}
    for name, (w64, w32) in ref.items():
        tol = tol_of(scaled_err(w32, w64))
        figures[name] = (scaled_err(got[name], w64), tol)
        print(f'{what} {name}: err {figures[name][0]:.2e} tol {tol:.2e}')
    for name, (w64, _) in ref.items():
        assert_close_scaled(got[name].double(), w64, tol=figures[name][1], what=f'{what} {name}')
    return figures


# ---- the golden cases --------------------------------------------------------------------------
def make_layer(case, nn):
    G = load_golden()
    cls = nn.GraphNorm if case['kind'] == 'graph_norm' else nn.LayerNorm
    layer = cls(G['meta']['F'], **case['kwargs'])
    layer.load_state_dict(case['state'])
    return layer


def check_golden_case(name, device, index_dtype=torch.int64, fuse=None):
    """golden case ``name`` through this package's layer on ``device``"""
    import pytorch_geometric_amd.nn as nn
    G = load_golden()
    case = G['cases'][name]
    layer = make_layer(case, nn).to(device)
    if fuse is not None:
        layer.fuse = fuse
    assert repr(layer) == case['repr']
    x = G['inputs'][case['x']].to(device).clone().requires_grad_(True)
    batch = G['batch'].to(device=device, dtype=index_dtype) if case['batch'] else None
    out = layer(x, batch, case['batch_size']) if case['batch'] else layer(x)
    out.backward(G['grad_out'].to(device))
    err = case['ref_err']
    got = {'out': out, 'grad_x': x.grad}
    got.update({f'grad_params.{n}': p.grad for n, p in layer.named_parameters()})
    want = {'out': case['out'], 'grad_x': case['grad_x']}
    want.update({f'grad_params.{n}': g for n, g in case['grad_params'].items()})
    assert set(got) == set(want)
    for key in want:
        print(f'{name} {key}: err {scaled_err(got[key], want[key]):.2e} '
              f'tol {tol_of(err[key]):.2e}')
    for key in want:
        assert_close_scaled(got[key].double(), want[key].double(), tol=tol_of(err[key]),
                            what=f'{name} {key}')
    return layer


def check_golden_model(norm, device, index_dtype=torch.int64):
    import pytorch_geometric_amd.nn as nn
    G = load_golden()
    M = G['models']
    case = M['cases'][norm]
    model = nn.GCN(G['meta']['F'], M['hidden'], 2, M['out'], norm=norm)
    model.load_state_dict(case['state'])
    model = model.to(device)
    assert model.supports_norm_batch == case['supports_norm_batch']
    x = G['inputs']['centred'].to(device).clone().requires_grad_(True)
    out = model(x, G['edge_index'].to(device),
                batch=G['batch'].to(device=device, dtype=index_dtype))
    out.backward(M['grad_out'].to(device))
    err = case['ref_err']
    got = {'out': out, 'grad_x': x.grad}
    got.update({f'grad_params.{n}': p.grad for n, p in model.named_parameters()})
    want = {'out': case['out'], 'grad_x': case['grad_x']}
    want.update({f'grad_params.{n}': g for n, g in case['grad_params'].items()})
    assert set(got) == set(want)
    for key in want:
        print(f'GCN({norm}) {key}: err {scaled_err(got[key], want[key]):.2e} '
              f'tol {tol_of(err[key]):.2e}')
    for key in want:
        assert_close_scaled(got[key].double(), want[key].double(), tol=tol_of(err[key]),
                            what=f'GCN({norm}) {key}')
    return model


def check_pools(device):
    import pytorch_geometric_amd.nn as nn
    G = load_golden()
    P = G['pools']
    fns = {'add': nn.global_add_pool, 'mean': nn.global_mean_pool, 'max': nn.global_max_pool}
    x0 = G['inputs'][P['x']]
    batch = G['batch'].to(device)
    for name, case in P['cases'].items():
        x = x0.to(device).clone().requires_grad_(True)
        out = fns[name](x, batch, P['size'])
        out.backward(case['grad_out'].float().to(device))
        assert_close_scaled(out.double(), case['out'], what=f'pool {name}')
        assert_close_scaled(x.grad.double(), case['grad_x'].double(), what=f'pool {name} grad_x')
        assert_close_scaled(fns[name](x0.to(device), None).double(), case['out_no_batch'],
                            what=f'pool {name} without batch')
        assert_close_scaled(fns[name](x0[:, 0].contiguous().to(device), batch).double(),
                            case['out_1d'], what=f'pool {name} 1-d')
