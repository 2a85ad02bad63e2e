"""The layers that reach ``propagate`` on host tensors, on one small bipartite graph, shared by the
CPU test of ``forward`` leaving ``fuse`` alone and the GPU test of the generic device route against
the host route.  Each case: constructor, whether ``x`` is a ``(x_src, x_dst)`` pair, whether the
layer takes ``edge_attr``."""
import torch

from pytorch_geometric_amd.nn import (GATConv, GATv2Conv, GENConv, GINConv, GINEConv, HGTConv,
                                      PNAConv, TransformerConv)

N_SRC, N_DST, E, F, DE = 37, 29, 200, 12, 5
DEG = torch.tensor([1, 2, 4, 6, 8, 7, 5, 3, 2, 1])      # an in-degree histogram for PNAConv


def _mlp(n_in, n_out):
    return torch.nn.Sequential(torch.nn.Linear(n_in, n_out), torch.nn.ReLU(),
                               torch.nn.Linear(n_out, n_out))


LAYERS = {
    'gat': (lambda: GATConv((F, F), 8, heads=3, add_self_loops=False), True, False),
    'gatv2': (lambda: GATv2Conv((F, F), 8, heads=3, add_self_loops=False), True, False),
    'transformer': (lambda: TransformerConv((F, F), 8, heads=3, beta=True), True, False),
    'gin': (lambda: GINConv(_mlp(F, 7), train_eps=True), True, False),
    'gine': (lambda: GINEConv(_mlp(F, 7), edge_dim=DE, train_eps=True), True, True),
    'pna': (lambda: PNAConv(F, 8, ['mean', 'min', 'max', 'std'],
                            ['identity', 'amplification', 'attenuation'], DEG, edge_dim=DE,
                            towers=2), False, True),
    'gen': (lambda: GENConv((F, F), 8, learn_t=True, norm='layer', edge_dim=DE), True, True),
}
HGT_META = (['a', 'p'], [('a', 'w', 'p'), ('p', 'c', 'p')])
NAMES = list(LAYERS) + ['hgt']


def recording(layer):
    """Every value assigned to ``layer.fuse`` from now on, through a throwaway subclass with a
    recording ``__setattr__``."""
    writes = []

    class Recording(type(layer)):
        def __setattr__(self, name, value):
            if name == 'fuse':
                writes.append(value)
            super().__setattr__(name, value)

    layer.__class__ = Recording
    return writes


def make(name):
    """``(layer, inputs)``: ``layer(*call(inputs, edge_index))`` runs it; ``inputs`` are float
    leaves on the host, in a dict"""
    g = torch.Generator().manual_seed(23)
    torch.manual_seed(29)
    if name == 'hgt':
        layer = HGTConv({'a': F, 'p': 16}, 16, HGT_META, heads=2)
        return layer, {'a': torch.randn(N_SRC, F, generator=g),
                       'p': torch.randn(N_DST, 16, generator=g)}
    ctor, pair, edge = LAYERS[name]
    inputs = {'x': torch.randn(N_SRC, F, generator=g)}
    if pair:
        inputs['x_dst'] = torch.randn(N_DST, F, generator=g)
    if edge:
        inputs['edge_attr'] = torch.randn(E, DE, generator=g)
    return ctor(), inputs


def edges(n_src, n_dst, seed, dtype):
    """``[2, E]``: the last destination has no edge"""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n_src, (E, ), generator=g),
                        torch.randint(0, n_dst - 1, (E, ), generator=g)]).to(dtype)


def run(name, layer, inputs, dtype, device='cpu'):
    """The outputs of ``layer`` on ``inputs`` (moved to ``device``) as a list of tensors"""
    t = {k: v.to(device) for k, v in inputs.items()}
    if name == 'hgt':
        eis = {('a', 'w', 'p'): edges(N_SRC, N_DST, 31, dtype).to(device),
               ('p', 'c', 'p'): edges(N_DST, N_DST, 37, dtype).to(device)}
        return list(layer(t, eis).values())
    pair = 'x_dst' in t
    ei = edges(N_SRC, N_DST if pair else N_SRC, 31, dtype).to(device)
    x = (t['x'], t['x_dst']) if pair else t['x']
    kw = {'edge_attr': t['edge_attr']} if 'edge_attr' in t else {}
    return [layer(x, ei, **kw)]
