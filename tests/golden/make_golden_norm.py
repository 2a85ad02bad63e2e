"""Generates tests/golden/golden_norm_v1.pt by running the REAL reference (PyG) on CPU: ``GraphNorm``
(nn/norm/graph_norm.py), ``LayerNorm`` (nn/norm/layer_norm.py) in graph and node mode, two
two-layer ``GCN(norm=...)`` models (nn/models/basic_gnn.py) and the three global pools
(nn/pool/glob.py).  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_norm.py

One batch of nine graphs of ``[1, 2, 3, 63, 64, 65, 0, 70, 5]`` nodes (one of them empty) with
``F = 20`` features; ``x`` is drawn centred and, as a second input, offset by 30 with a per-column
ramp (the input on which a one-pass variance in float32 can go wrong).  The parameters are set to
ramps: ``weight`` 0.5 .. 1.5, ``bias`` -1 .. 1, ``mean_scale`` 0.2 .. 1.3.  One case passes
``batch_size = 11``, i.e. two trailing empty graphs.

Every case is evaluated twice by the reference: in float64 — the stored ``out``, ``grad_x`` and
``grad_params`` (the two ``[N, F]`` results rounded once to float32 to keep the file small, the
parameter gradients kept in float64) — and in float32, whose scaled error against float64, ``max
|f32 - f64| / max(max |f64|, 1)``, is stored per tensor as a plain float under ``ref_err``: the
reference's own float32 error is what a float32 kernel is measured against.  For the models the
seed is advanced until no input of a ReLU sits within 1e-4 of zero (a float32 evaluation may take
the other branch there).  Tensors, floats and constructor arguments only."""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import (GCN, GraphNorm, LayerNorm, global_add_pool,  # noqa: E402
                                global_max_pool, global_mean_pool)

HERE = os.path.dirname(os.path.abspath(__file__))
F = 20
SIZES = [1, 2, 3, 63, 64, 65, 0, 70, 5]
MARGIN = 1e-4


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ramp(lo, hi, n=F):
    return torch.linspace(lo, hi, n)


batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
N = batch.numel()
x_centred = torch.randn(N, F, generator=gen(11))
x_offset = torch.randn(N, F, generator=gen(12)) + 30.0 + ramp(-3.0, 3.0)
grad_out = torch.randn(N, F, generator=gen(13))
INPUTS = {'centred': x_centred, 'offset': x_offset}


def scaled_err(a32, a64):
    if a64.numel() == 0:
        return 0.0
    return float((a32.double() - a64).abs().max() / max(float(a64.abs().max()), 1.0))


def evaluate(module, x, dtype, call):
    module = module.to(dtype)
    xx = x.to(dtype).clone().requires_grad_(True)
    out = call(module, xx)
    params = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(out, [xx] + [p for _, p in params], grad_out.to(dtype),
                                allow_unused=True)
    return (out.detach(), grads[0].detach(),
            {n: g.detach() for (n, _), g in zip(params, grads[1:]) if g is not None})


def record(make, x_name, call, **meta):
    x = INPUTS[x_name]
    o64, gx64, gp64 = evaluate(make(), x, torch.float64, call)
    o32, gx32, gp32 = evaluate(make(), x, torch.float32, call)
    module = make()
    err = {'out': scaled_err(o32, o64), 'grad_x': scaled_err(gx32, gx64)}
    err.update({f'grad_params.{n}': scaled_err(gp32[n], g) for n, g in gp64.items()})
    return {'x': x_name, 'state': {k: v.detach().clone() for k, v in module.state_dict().items()},
            'repr': repr(module), 'out': o64.float(), 'grad_x': gx64.float(), 'grad_params': gp64,
            'ref_err': err, **meta}


def make_graph_norm():
    m = GraphNorm(F)
    with torch.no_grad():
        m.weight.copy_(ramp(0.5, 1.5))
        m.bias.copy_(ramp(-1.0, 1.0))
        m.mean_scale.copy_(ramp(0.2, 1.3))
    return m


def make_layer_norm(**kw):
    def make():
        m = LayerNorm(F, **kw)
        if m.weight is not None:
            with torch.no_grad():
                m.weight.copy_(ramp(0.5, 1.5))
                m.bias.copy_(ramp(-1.0, 1.0))
        return m
    return make


def with_batch(size=None):
    return lambda m, x: m(x, batch, size)


def no_batch(m, x):
    return m(x)


G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'F': F,
              'sizes': SIZES, 'margin': MARGIN},
     'batch': batch, 'inputs': INPUTS, 'grad_out': grad_out, 'cases': {}}
C = G['cases']
for name in INPUTS:
    C[f'graph_norm_{name}'] = record(make_graph_norm, name, with_batch(), kind='graph_norm',
                                     kwargs={}, batch=True, batch_size=None)
    C[f'layer_norm_{name}'] = record(make_layer_norm(), name, with_batch(), kind='layer_norm',
                                     kwargs={}, batch=True, batch_size=None)
C['graph_norm_size11'] = record(make_graph_norm, 'offset', with_batch(11), kind='graph_norm',
                                kwargs={}, batch=True, batch_size=11)
C['graph_norm_no_batch'] = record(make_graph_norm, 'offset', no_batch, kind='graph_norm',
                                  kwargs={}, batch=False, batch_size=None)
C['layer_norm_no_batch'] = record(make_layer_norm(), 'offset', no_batch, kind='layer_norm',
                                  kwargs={}, batch=False, batch_size=None)
C['layer_norm_no_affine'] = record(make_layer_norm(affine=False), 'centred', with_batch(),
                                   kind='layer_norm', kwargs={'affine': False}, batch=True,
                                   batch_size=None)
C['layer_norm_node'] = record(make_layer_norm(mode='node'), 'offset', no_batch, kind='layer_norm',
                              kwargs={'mode': 'node'}, batch=False, batch_size=None)

# ---- two-layer GCN models with a norm between the layers -----------------------------------------
E = 1200
g = gen(21)
edge_index = torch.stack([torch.randint(0, N, (E, ), generator=g),
                          torch.randint(0, N, (E, ), generator=g)])
G['edge_index'] = edge_index
HIDDEN, OUT = 16, 7
grad_model = torch.randn(N, OUT, generator=gen(22))


def run_model(norm, seed):
    def make():
        torch.manual_seed(seed)
        m = GCN(F, HIDDEN, 2, OUT, norm=norm)
        with torch.no_grad():
            for p in m.norms[0].parameters():
                p.add_(0.3 * torch.randn(p.shape, generator=gen(seed + 1)))
        return m

    seen = []
    probe = make().double()
    probe.norms[0].register_forward_hook(
        lambda m, a, o: seen.append(float(o.detach().abs().min())))
    probe(x_centred.double(), edge_index, batch=batch)
    if min(seen) < MARGIN:
        return None

    def evaluate_model(dtype):
        m = make().to(dtype)
        xx = x_centred.to(dtype).clone().requires_grad_(True)
        out = m(xx, edge_index, batch=batch)
        params = list(m.named_parameters())
        grads = torch.autograd.grad(out, [xx] + [p for _, p in params], grad_model.to(dtype))
        return out.detach(), grads[0].detach(), {n: g.detach() for (n, _), g
                                                 in zip(params, grads[1:])}

    o64, gx64, gp64 = evaluate_model(torch.float64)
    o32, gx32, gp32 = evaluate_model(torch.float32)
    m = make()
    err = {'out': scaled_err(o32, o64), 'grad_x': scaled_err(gx32, gx64)}
    err.update({f'grad_params.{n}': scaled_err(gp32[n], v) for n, v in gp64.items()})
    return {'norm': norm, 'seed': seed, 'margin': min(seen), 'repr': repr(m),
            'norms_repr': repr(m.norms), 'supports_norm_batch': m.supports_norm_batch,
            'state': {k: v.detach().clone() for k, v in m.state_dict().items()},
            'out': o64.float(), 'grad_x': gx64.float(), 'grad_params': gp64, 'ref_err': err}


G['models'] = {'hidden': HIDDEN, 'out': OUT, 'grad_out': grad_model, 'cases': {}}
for i, norm in enumerate(('graph_norm', 'layer_norm')):
    seed = 500 + 100 * i
    case = run_model(norm, seed)
    while case is None:
        seed += 1
        case = run_model(norm, seed)
    G['models']['cases'][norm] = case
    print(f"GCN(norm={norm}): seed {case['seed']}  margin {case['margin']:.2e}  keys "
          f"{list(case['state'])}")

# ---- the three pools -----------------------------------------------------------------------------
pools = {}
for name, fn in (('add', global_add_pool), ('mean', global_mean_pool), ('max', global_max_pool)):
    x64 = x_offset.double().requires_grad_(True)
    out = fn(x64, batch, 11)
    go = torch.randn(out.shape, generator=gen(31), dtype=torch.float64)
    (gx, ) = torch.autograd.grad(out, x64, go)
    pools[name] = {'out': out.detach(), 'grad_out': go, 'grad_x': gx.float(),
                   'out_no_batch': fn(x_offset.double(), None).detach(),
                   'out_1d': fn(x_offset[:, 0].double(), batch).detach()}
G['pools'] = {'x': 'offset', 'size': 11, 'cases': pools}

G['reprs'] = {'graph_norm': repr(GraphNorm(F)), 'layer_norm': repr(LayerNorm(F)),
              'layer_norm_node': repr(LayerNorm(F, affine=False, mode='node'))}
G['keys'] = {'graph_norm': {k: tuple(v.shape) for k, v in GraphNorm(F).state_dict().items()},
             'layer_norm': {k: tuple(v.shape) for k, v in LayerNorm(F).state_dict().items()},
             'layer_norm_no_affine': {k: tuple(v.shape) for k, v
                                      in LayerNorm(F, affine=False).state_dict().items()}}

for name, case in C.items():
    print(f"{name}: |out| max {float(case['out'].abs().max()):.3f}  ref_err "
          + '  '.join(f'{k} {v:.1e}' for k, v in case['ref_err'].items()))
out_path = os.path.join(HERE, 'golden_norm_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
