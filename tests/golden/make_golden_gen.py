"""Generates tests/golden/golden_gen_v1.pt by running the REAL reference (PyG) on CPU: ``GENConv``
(nn/conv/gen_conv.py:44-243) in thirteen settings, one two-layer ``DeepGCNLayer('res+')`` stack
(nn/models/deepgcn.py), ``DeepGCNLayer`` in its other three blocks and ``MessageNorm``
(nn/norm/msg_norm.py).  Build container only:

    PYG_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_gen.py

The graph is the one of make_golden_gin.py (48 nodes, 16 features, 400 edges with skewed
destinations, empty destinations and some self-loops, a 20-node destination set for the pair
cases).  A case with edge features draws its own ``edge_attr [400, 16]`` from its seed (a case with
``edge_dim = D`` reads the first ``D`` columns).  An fp32 kernel may round the ReLU's argument
``x_j + e`` across zero, which flips a mask and changes a gradient by a whole entry: the argument is
formed in float64 and a case's seed is advanced until ``min |pre| >= 1e-4``; the seed that was taken
is recorded.  In the stack the convolutions read ``relu(norm(x))``, whose zeros are exact; there
the margin is taken on the outputs of the two outer norms.  Tensors only (and each case's
constructor arguments): inputs, state dicts, outputs and the gradients of every ``x``, of
``edge_attr`` and of every parameter.
"""
import os
import sys

import torch

sys.path.insert(0, os.environ['PYG_REFERENCE'])
import torch_geometric  # noqa: E402
from torch_geometric.nn import DeepGCNLayer, GENConv, MessageNorm  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, E, N_PAIR_DST = 48, 16, 400, 20
MARGIN = 1e-4

# (in_channels, out_channels), constructor arguments, x: 'one' | 'pair' | 'pair_none',
# width of edge_attr (0: none)
CASES = {
    'defaults': ((K, K), dict(), 'one', 0),
    'learn_t': ((K, K), dict(t=0.7, learn_t=True), 'one', 0),
    't_half': ((K, K), dict(t=0.5), 'one', 0),
    'softmax_sg': ((K, K), dict(aggr='softmax_sg', t=1.5), 'one', 0),
    'wide_edge': ((K, K), dict(), 'one', K),
    'edge_dim': ((K, K), dict(edge_dim=3), 'one', 3),
    'edge_dim_bias': ((K, K), dict(edge_dim=3, bias=True, learn_t=True), 'one', 3),
    'lin_src_dst': ((K, 8), dict(), 'one', 0),
    'pair': ((K, K), dict(edge_dim=3), 'pair', 3),
    'pair_none': ((K, K), dict(), 'pair_none', 0),
    'msg_norm': ((K, K), dict(msg_norm=True, learn_msg_scale=True, norm='layer'), 'one', 0),
    'powermean': ((K, K), dict(aggr='powermean', p=1.5, learn_p=True), 'one', 0),
    'mean': ((K, K), dict(aggr='mean'), 'one', K),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_graph(seed):  # (make_golden_gin.py's)
    g = gen(seed)
    src = torch.randint(0, N, (E, ), generator=g)
    dst = (torch.rand(E, generator=g).pow(3) * N).long().clamp(max=N - 1)
    src[:12] = dst[:12]                                   # some self-loops
    pair_dst = (torch.rand(E, generator=g).pow(3) * N_PAIR_DST).long().clamp(max=N_PAIR_DST - 1)
    return {'x': torch.randn(N, K, generator=g), 'x_dst': torch.randn(N_PAIR_DST, K, generator=g),
            'edge_index': torch.stack([src, dst]), 'edge_index_pair': torch.stack([src, pair_dst])}


def record(case, module, out, leaves, n_x, seed):
    go = torch.randn(out.shape, generator=gen(seed + 1))
    params = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(out, leaves + [p for _, p in params], go)
    case.update({'state': {k: v.detach().clone() for k, v in module.state_dict().items()},
                 'out': out.detach(), 'grad_out': go,
                 'grad_x': [g.detach() for g in grads[:n_x]],
                 'grad_params': {n: g.detach() for (n, _), g in zip(params, grads[len(leaves):])}})
    if len(leaves) > n_x:
        case['grad_edge_attr'] = grads[n_x].detach()
    return case


def run_conv(channels, kw, mode, width, graph, seed):
    torch.manual_seed(seed)
    conv = GENConv(channels[0], channels[1], **kw)
    xs = [graph['x'].clone().requires_grad_(True)]
    if mode == 'pair':
        xs.append(graph['x_dst'].clone().requires_grad_(True))
    ei = graph['edge_index'] if mode == 'one' else graph['edge_index_pair']
    size = None if mode == 'one' else (N, N_PAIR_DST)
    x_in = xs[0] if mode == 'one' else (xs[0], xs[1] if mode == 'pair' else None)
    case = {'channels': channels, 'kwargs': dict(kw), 'mode': mode, 'seed': seed,
            'repr': repr(conv)}
    leaves = list(xs)
    ea = None
    # the margin of the ReLU's argument, in float64
    pre = graph['x'].double()
    if hasattr(conv, 'lin_src'):
        pre = pre @ conv.lin_src.weight.detach().double().t()
    pre = pre[ei[0]]
    if width:
        ea = torch.randn(E, K, generator=gen(seed + 100))[:, :width].clone().requires_grad_(True)
        e64 = ea.detach().double()
        if hasattr(conv, 'lin_edge'):
            e64 = e64 @ conv.lin_edge.weight.detach().double().t()
            if conv.lin_edge.bias is not None:
                e64 = e64 + conv.lin_edge.bias.detach().double()
        pre = pre + e64
        case['edge_attr'] = ea.detach().clone()
        leaves.append(ea)
    case['margin'] = float(pre.abs().min())
    if case['margin'] < MARGIN:
        return None
    out = conv(x_in, ei, edge_attr=ea, size=size)
    return record(case, conv, out, leaves, len(xs), seed)


def make_stack(block='res+'):
    return torch.nn.ModuleList([
        DeepGCNLayer(GENConv(K, K, learn_t=True, norm='layer'), torch.nn.LayerNorm(K),
                     torch.nn.ReLU(), block=block, dropout=0.0) for _ in range(2)])


def run_stack(graph, seed):
    torch.manual_seed(seed)
    layers = make_stack()
    seen = []
    for layer in layers:
        layer.norm.register_forward_hook(lambda m, a, o: seen.append(float(o.detach().abs().min())))
    x = graph['x'].clone().requires_grad_(True)
    h = x
    for layer in layers:
        h = layer(h, graph['edge_index'])
    case = {'seed': seed, 'margin': min(seen)}
    if case['margin'] < MARGIN:
        return None
    return record(case, layers, h, [x], 1, seed)


def run_blocks(graph, seed):
    """one layer's state in the three other blocks (the parameters do not depend on the block)"""
    torch.manual_seed(seed)
    state = make_stack()[0].state_dict()
    outs = {}
    for block in ('res', 'dense', 'plain'):
        layer = make_stack(block)[0]
        layer.load_state_dict(state)
        outs[block] = layer(graph['x'], graph['edge_index']).detach()
    return {'state': {k: v.clone() for k, v in state.items()}, 'out': outs}


def run_msg_norm(seed):
    g = gen(seed)
    mod = MessageNorm(learn_scale=True)
    mod.scale.data.fill_(1.3)
    x = torch.randn(N, K, generator=g, requires_grad=True)
    msg = torch.randn(N, K, generator=g, requires_grad=True)
    out = mod(x, msg)
    case = record({'x': x.detach().clone(), 'msg': msg.detach().clone()}, mod, out, [x, msg], 2,
                  seed)
    case['out_p1'] = mod(x, msg, p=1.0).detach()
    return case


graph = make_graph(2)
deg = torch.bincount(graph['edge_index'][1], minlength=N)
assert int((deg == 0).sum()) > 0 and int(deg.max()) > 40

G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__, 'N': N, 'K': K,
              'margin': MARGIN}, **graph, 'cases': {}}
for i, (name, (channels, kw, mode, width)) in enumerate(CASES.items()):
    seed = 7000 + 200 * i
    case = run_conv(channels, kw, mode, width, graph, seed)
    while case is None:
        seed += 1
        case = run_conv(channels, kw, mode, width, graph, seed)
    G['cases'][name] = case
    assert case['margin'] >= MARGIN
    print(f"{name}: seed {case['seed']}  out {tuple(case['out'].shape)}  |out| max "
          f"{float(case['out'].abs().max()):.3f}  margin {case['margin']:.2e}  "
          f"params {list(case['grad_params'])}")

seed = 9900
stack = run_stack(graph, seed)
while stack is None:
    seed += 1
    stack = run_stack(graph, seed)
G['stack'] = stack
print(f"stack: seed {stack['seed']}  margin {stack['margin']:.2e}  keys {len(stack['state'])}")
G['blocks'] = run_blocks(graph, 9950)
G['msg_norm'] = run_msg_norm(9960)
multi = GENConv((K, 12), 8, aggr=['softmax', 'mean', 'max'], edge_dim=5, bias=True, msg_norm=True,
                num_layers=3, norm='batch')
G['multi'] = {'repr': repr(multi), 'keys': list(multi.state_dict())}
G['reprs'] = {'deep': repr(make_stack('dense')[0]), 'msg_norm': repr(MessageNorm(True)),
              'msg_norm_fixed': repr(MessageNorm())}

out_path = os.path.join(HERE, 'golden_gen_v1.pt')
torch.save(G, out_path)
print('wrote', out_path, os.path.getsize(out_path), 'bytes')
