"""Generates tests/golden/golden_rgat_v1.pt by running the REAL reference (PyG) on CPU: ``RGATConv``
(nn/conv/rgat_conv.py:16-534) in fourteen settings and one two-layer stack.  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_rgat.py

One multigraph for every case: 40 nodes, 12 input features, 250 edges of 3 relations with skewed
destinations (so that a relation is absent at some destinations), node 39 without an incoming
edge, self loops, and duplicate edges (the same source, destination and relation twice, and once
more under another relation), plus 5 edge features.

EVERY parameter of a case is set explicitly from the case's seeded generator and stored — ``l2``
too, which the reference's ``reset_parameters`` leaves uninitialised (rgat_conv.py:310).  Tensors
only (and each case's constructor arguments as plain values): inputs, state dict, ``out``,
``alpha`` in edge order, the cotangent, the gradients of ``x`` and ``edge_attr`` and of every
parameter the case's forward reaches.

Kinks: a float32 kernel may round a pre-activation across zero, which flips the leaky ReLU's slope
(or the ReLU of ``mod='scaled'``, or the ReLU between the stack's layers) and changes a gradient by
a whole entry.  The generator computes the least ``|pre|`` with the restatement of
tests/_rgat_ref.py, advances the case's seed until it is at least 1e-4, and records the seed taken
and the minimum (``margin``).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ['PYG_REFERENCE'])
sys.path.insert(0, os.path.dirname(HERE))
from torch_geometric.nn import RGATConv  # noqa: E402

from _rgat_ref import rgat_layer  # noqa: E402

N, K, E, R, DE = 40, 12, 250, 3, 5
MARGIN = 1e-4
MULT = 'multiplicative-self-attention'

CASES = {
    'default': dict(out_channels=8),
    'heads2': dict(out_channels=8, heads=2),
    'heads3_mean': dict(out_channels=6, heads=3, concat=False),
    'within': dict(out_channels=8, heads=2, attention_mechanism='within-relation'),
    'no_bias': dict(out_channels=8, heads=2, bias=False),
    'bases2': dict(out_channels=8, heads=2, num_bases=2),
    'blocks2': dict(out_channels=8, heads=2, num_blocks=2),
    'edge5': dict(out_channels=8, heads=2, edge_dim=DE),
    'mod_additive': dict(out_channels=8, heads=2, mod='additive'),
    'mod_scaled': dict(out_channels=8, heads=2, mod='scaled'),
    'mod_f_additive': dict(out_channels=8, heads=2, mod='f-additive'),
    'mod_f_scaled': dict(out_channels=8, heads=2, mod='f-scaled'),
    'mult_dim2': dict(out_channels=8, heads=2, attention_mode=MULT, dim=2),
    'mult_dim2_edge': dict(out_channels=8, heads=2, attention_mode=MULT, dim=2, edge_dim=DE),
}
STACK = [dict(in_channels=K, out_channels=8, num_relations=R, heads=2),
         dict(in_channels=16, out_channels=6, num_relations=R, heads=3, concat=False,
              attention_mechanism='within-relation')]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_graph(seed):
    g = gen(seed)
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(2) * (N - 1)).long().clamp(max=N - 2)   # never node 39
    et = torch.randint(0, R, (E, ), generator=g)
    src[:6] = dst[:6]                                      # self loops
    src[10], dst[10], et[10] = src[9], dst[9], et[9]       # a duplicate edge
    src[11], dst[11], et[11] = src[9], dst[9], (et[9] + 1) % R   # and once more, another relation
    x = torch.randn(N, K, generator=g)
    ea = torch.randn(E, DE, generator=g)
    return x, torch.stack([src, dst]), et, ea


def set_params(module, seed):
    g = gen(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            scale = 0.5 if p.dim() > 1 else 0.3
            p.copy_(torch.randn(p.shape, generator=g) * scale)


def run(cfg, seed, x, ei, et, ea):
    layer = RGATConv(**cfg)
    set_params(layer, seed)
    x = x.clone().requires_grad_(True)
    ea = ea.clone().requires_grad_(True) if cfg.get('edge_dim') is not None else None
    out, (_, alpha) = layer(x, ei, et, ea, return_attention_weights=True)
    grad_out = torch.randn(out.shape, generator=gen(seed + 1))
    params = list(layer.named_parameters())
    ins = [x] + ([] if ea is None else [ea])
    grads = torch.autograd.grad(out, ins + [p for _, p in params], grad_out, allow_unused=True)
    state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    with torch.no_grad():
        margin = rgat_layer({k: v.double() for k, v in state.items()}, cfg, x.double(), ei, et,
                            None if ea is None else ea.double())[2]
    return dict(cfg=cfg, seed=seed, margin=margin, state=state, out=out.detach(),
                alpha=alpha.detach(), grad_out=grad_out,
                grad_in=[g.detach() for g in grads[:len(ins)]],
                grad_params={n: g.detach() for (n, _), g in zip(params, grads[len(ins):])
                             if g is not None})


def main():
    x, ei, et, ea = make_graph(7)
    indeg = torch.bincount(ei[1], minlength=N)
    assert int(indeg[N - 1]) == 0 and int((ei[0] == ei[1]).sum()) >= 6
    per = torch.zeros(N, R).index_put((ei[1], et), torch.ones(E), accumulate=True)
    assert bool(((per == 0).any(1) & (indeg > 0)).any()), 'no destination lacks a relation'
    G = dict(x=x, edge_index=ei, edge_type=et, edge_attr=ea, cases={})
    for i, (name, extra) in enumerate(CASES.items()):
        cfg = dict(in_channels=K, num_relations=R, **extra)
        seed = 100 * (i + 1)
        while True:
            case = run(cfg, seed, x, ei, et, ea)
            if case['margin'] >= MARGIN:
                break
            seed += 1
        G['cases'][name] = case
        print(f"{name}: seed {seed}, margin {case['margin']:.2e}, "
              f"grads of {list(case['grad_params'])}")
    seed = 5000
    while True:
        layers = torch.nn.ModuleList([RGATConv(**cfg) for cfg in STACK])
        set_params(layers, seed)
        xs = x.clone().requires_grad_(True)
        hidden = layers[0](xs, ei, et)
        out = layers[1](torch.relu(hidden), ei, et)
        state = {k: v.detach().clone() for k, v in layers.state_dict().items()}
        with torch.no_grad():
            margins = [float(hidden.abs().min())]
            for i, (cfg, inp) in enumerate(zip(STACK, (x, torch.relu(hidden)))):
                sub = {k[2:]: v.double() for k, v in state.items() if k.startswith(f'{i}.')}
                margins.append(rgat_layer(sub, cfg, inp.double(), ei, et)[2])
        if min(margins) >= MARGIN:
            break
        seed += 1
    grad_out = torch.randn(out.shape, generator=gen(seed + 1))
    params = list(layers.named_parameters())
    grads = torch.autograd.grad(out, [xs] + [p for _, p in params], grad_out, allow_unused=True)
    G['stack'] = dict(cfgs=STACK, seed=seed, margin=min(margins), state=state, out=out.detach(),
                      grad_out=grad_out, grad_in=[grads[0].detach()],
                      grad_params={n: g.detach() for (n, _), g in zip(params, grads[1:])
                                   if g is not None})
    print(f"stack: seed {seed}, margin {min(margins):.2e}")
    path = os.path.join(HERE, 'golden_rgat_v1.pt')
    torch.save(G, path)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
