"""nn.HeteroConv / nn.HeteroDictLinear: everything that needs no device.  The plain-torch
restatement (tests/_hetero_conv_ref.py) is pinned to the reference's recorded results
(tests/golden/golden_hetero_conv_v1.pt); state dicts interchange with the reference; argument
routing, the planner of the fast path and the argument checks of the two new entry points."""
import ctypes
import os
import warnings

import pytest
import torch

import _hetero_conv_ref as R
from pytorch_geometric_amd.nn import HeteroConv, HeteroDictLinear, SAGEConv, group
from _util import assert_close, assert_close_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_golden():
    path = os.path.join(ROOT, 'tests', 'golden', 'golden_hetero_conv_v1.pt')
    G = torch.load(path, map_location='cpu', weights_only=False)
    ets = [tuple(et) for et in G['meta']['edge_types']]
    G['edge_types'] = ets
    G['edge_index'] = {et: G['edge_index_dict']['__'.join(et)] for et in ets}
    return G


def build_layer(G, case, device='cpu'):
    """This package's layer for a golden case, the reference's state dict loaded."""
    K, N = G['meta']['K'], G['meta']['N_out']
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        layer = HeteroConv({et: SAGEConv((K, K), N, aggr=case['conv_aggr'],
                                         **G['meta']['conv_kwargs'].get('__'.join(et), {}))
                            for et in G['edge_types']}, aggr=case['group_aggr'])
    layer.load_state_dict(case['state'])
    return layer.to(device)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_restatement_reproduces_every_golden_case(dtype):
    G = load_golden()
    assert len(G['cases']) == 12
    for name, case in G['cases'].items():
        xs = {t: v.to(dtype).requires_grad_(True) for t, v in G['x_dict'].items()}
        params = {k: v.to(dtype).requires_grad_(True) for k, v in case['state'].items()}
        out = R.hetero_conv(G['edge_types'], xs, G['edge_index'], params, case['conv_aggr'],
                            case['group_aggr'])
        assert list(out) == case['out_order'] == ['b', 'a']
        for t in out:
            assert_close(out[t].float(), case['out'][t], what=f'{name} out[{t}]')
        leaves = list(xs.values()) + list(params.values())
        grads = torch.autograd.grad([out[t] for t in out], leaves,
                                    [case['grad_out'][t].to(dtype) for t in out])
        for t, g in zip(xs, grads):
            assert_close_scaled(g.float(), case['grad_x'][t], what=f'{name} grad_x[{t}]')
        for k, g in zip(params, grads[len(xs):]):
            assert_close_scaled(g.float(), case['grad_params'][k], what=f'{name} grad {k}')


def test_state_dict_interchanges_with_the_reference():
    G = load_golden()
    case = G['cases']['sum-mean']
    layer = build_layer(G, case)
    assert list(layer.state_dict()) == list(case['state'])
    assert 'convs.<a___to___b>.lin_l.weight' in case['state']
    assert 'convs.<a___also___b>.lin_r.weight' not in case['state']   # root_weight=False
    assert 'convs.<b___self___b>.lin_l.bias' not in case['state']     # bias=False
    for k, v in layer.state_dict().items():
        assert torch.equal(v, case['state'][k])
    assert list(layer.convs.keys()) == G['edge_types']
    assert ('a', 'to', 'b') in layer.convs and layer.convs[('a', 'to', 'b')].aggr == 'mean'
    assert repr(layer) == 'HeteroConv(num_relations=5)'
    # dots in a key are stored as '#'
    from pytorch_geometric_amd.nn.module_dict import ModuleDict
    assert ModuleDict.name_of(('a.x', 'r', 'b')) == '<a#x___r___b>'
    assert ModuleDict.name_of('keys') == '<keys>' and ModuleDict.name_of('v1.0') == 'v1#0'
    d = ModuleDict({('a.x', 'r', 'b'): torch.nn.Identity(), 'type': torch.nn.Identity()})
    assert list(d.keys()) == list(d) == [('a.x', 'r', 'b'), 'type'] and len(d) == 2
    assert list(d.state_dict()) == [] and [n for n, _ in d.named_children()] == \
        ['<a#x___r___b>', '<type>']
    assert ('a.x', 'r', 'b') in d and 'keys' not in d
    del d['type']
    assert [k for k, _ in d.items()] == [('a.x', 'r', 'b')]


class Recorder(torch.nn.Module):
    """A stand-in conv: returns a constant and remembers how it was called."""

    def __init__(self, value):
        super().__init__()
        self.value, self.calls = value, []

    def reset_parameters(self):
        self.calls.append('reset')

    def forward(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return torch.full((2, 3), float(self.value))


def test_argument_routing_and_grouping():
    ab, bb, ca, cb = ('a', 'r', 'b'), ('b', 's', 'b'), ('c', 't', 'a'), ('c', 'u', 'b')
    convs = {ab: Recorder(1), bb: Recorder(2), ca: Recorder(4), cb: Recorder(8)}
    with pytest.warns(UserWarning, match=r"There exist node types \(\{'c'\}\) whose "
                                         r"representations do not get updated during message "
                                         r"passing as they do not occur as destination type in "
                                         r"any edge type. This may lead to unexpected behavior."):
        layer = HeteroConv(convs, aggr='sum')
    x = {'a': torch.zeros(1), 'b': torch.ones(1)}
    ei = {ab: 'E_ab', bb: 'E_bb', ca: 'E_ca'}                 # no edge-level entry for `cb`
    out = layer(x, ei, edge_attr_dict={ab: 'A_ab'}, size_dict={'b': 7})
    assert list(out) == ['b', 'a']                            # order of first appearance
    assert float(out['b'][0, 0]) == 3 and float(out['a'][0, 0]) == 4
    (args, kwargs), = convs[ab].calls
    assert args[0][0] is x['a'] and args[0][1] is x['b'] and args[1] == 'E_ab'   # the (src, dst) pair
    assert kwargs == {'edge_attr': 'A_ab', 'size': (None, 7)}
    (args, kwargs), = convs[bb].calls
    assert args[0] is x['b'] and args[1] == 'E_bb' and kwargs == {'size': 7}     # src == dst
    (args, kwargs), = convs[ca].calls
    assert args[0][0] is None and args[0][1] is x['a'] and kwargs == {}          # 'c' has no features
    assert convs[cb].calls == []                              # skipped: no edge-level argument
    with pytest.raises(ValueError, match=r"Keyword arguments in 'HeteroConv' need to end with "
                                         r"'_dict' \(got 'edge_attr'\)"):
        layer(x, ei, edge_attr={ab: 'A_ab'})
    layer.reset_parameters()
    assert all(c.calls[-1] == 'reset' for c in convs.values())
    # the group modes
    xs = [torch.tensor([[1., 5.]]), torch.tensor([[3., 2.]])]
    assert group([], 'sum') is None
    assert group(xs[:1], 'max') is xs[0]
    assert group(xs, None).shape == (1, 2, 2) and group(xs[:1], None).shape == (1, 1, 2)
    assert group(xs, 'cat').tolist() == [[1., 5., 3., 2.]]
    assert group(xs, 'sum').tolist() == [[4., 7.]] and group(xs, 'mean').tolist() == [[2., 3.5]]
    assert group(xs, 'min').tolist() == [[1., 2.]] and group(xs, 'max').tolist() == [[3., 5.]]
    # a bipartite edge type refuses a conv that adds self loops
    from pytorch_geometric_amd.nn import GCNConv
    with pytest.raises(ValueError, match="'add_self_loops' attribute set to 'True'"):
        HeteroConv({ab: GCNConv(4, 4)})


def test_planner_picks_the_fast_path_edge_types():
    from pytorch_geometric_amd import _hetero
    from pytorch_geometric_amd.nn import GraphConv
    ab, ab2, bb, ca = ('a', 'r', 'b'), ('a', 'r2', 'b'), ('b', 's', 'b'), ('c', 't', 'a')
    x = {'a': torch.randn(5, 8), 'b': torch.randn(4, 8), 'c': torch.randn(3, 16)}
    ei = {et: torch.zeros(2, 0, dtype=torch.int64) for et in (ab, ab2, bb, ca)}

    def make(over=None):
        convs = {ab: SAGEConv((8, 8), 6), ab2: SAGEConv((8, 8), 6, aggr='sum', root_weight=False),
                 bb: SAGEConv(8, 6, bias=False), ca: SAGEConv((16, 8), 6)}
        convs.update(over or {})
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return HeteroConv(convs)

    def plan(layer, xd=x, eid=ei, aggr='sum', fuse=True):
        return _hetero.plan(layer.convs.items(), xd, eid, aggr, fuse, require_device=False)

    p = plan(make())
    assert p is not None
    assert p.groups == [(8, [ab, ab2, bb]), (16, [ca])]       # grouped by source width
    assert p.dst == {'b': ([ab, ab2, bb], True), 'a': ([ca], True)}
    assert plan(make(), aggr='mean') is not None
    for aggr in ('min', 'max', 'cat', None):
        assert plan(make(), aggr=aggr) is None
    assert plan(make(), fuse=False) is None
    # an edge type without an edge_index is skipped, not refused
    p = plan(make(), eid={k: v for k, v in ei.items() if k != ca})
    assert p.groups == [(8, [ab, ab2, bb])] and list(p.dst) == ['b']
    # a layer is planned as a whole: one edge type that does not qualify makes it generic
    assert plan(make({ab: GraphConv((8, 8), 6)})) is None
    assert plan(make({ab: SAGEConv((8, 8), 6, aggr='max')})) is None
    assert plan(make({ab: SAGEConv((8, 8), 6, project=True)})) is None
    assert plan(make({ab: SAGEConv((8, 8), 6, normalize=True)})) is None
    hooked = make()
    hooked.convs[ab].register_propagate_forward_pre_hook(lambda *a: None)
    assert plan(hooked) is None
    off = make()
    off.convs[bb].fuse = False
    assert plan(off) is None
    assert plan(make(), xd={**x, 'a': x['a'].double()}) is None
    # features the kernels cannot read in place (the generic loop accepts them): a transposed
    # view, an expanded row, overlapping rows; a row-strided block is fine
    assert plan(make(), xd={**x, 'a': torch.randn(8, 5).t()}) is None
    assert plan(make(), xd={**x, 'b': torch.randn(1, 8).expand(4, 8)}) is None
    assert plan(make(), xd={**x, 'b': torch.randn(40).as_strided((4, 8), (4, 1))}) is None
    assert plan(make(), xd={**x, 'a': torch.randn(5, 24)[:, 8:16]}) is not None
    assert plan(make(), eid={**ei, ab: ei[ab].to(torch.int32)}) is None      # mixed index dtypes
    assert plan(make(), eid={k: v.to(torch.int32) for k, v in ei.items()}) is not None
    assert plan(make(), eid={**ei, ab: ei[ab].to(torch.float32)}) is None
    # device tensors are required on the real path
    assert _hetero.plan(make().convs.items(), x, ei, 'sum') is None
    # HeteroConv only plans the plain (x_dict, edge_index_dict) call
    layer = make()
    assert layer._fast_plan((x, ei), {'size_dict': {}}) is None
    assert layer._fast_plan((x, ei, {}), {}) is None


def test_planner_refuses_more_than_64_edge_types():
    from pytorch_geometric_amd import _hetero
    x = {'a': torch.randn(5, 8)}
    for n, ok in ((64, True), (65, False)):
        ets = [('a', f'r{i}', 'a') for i in range(n)]
        layer = HeteroConv({et: SAGEConv(8, 4) for et in ets})
        ei = {et: torch.zeros(2, 0, dtype=torch.int64) for et in ets}
        p = _hetero.plan(layer.convs.items(), x, ei, 'sum', require_device=False)
        assert (p is not None) == ok
        if ok:
            assert len(p.groups) == 1 and len(p.groups[0][1]) == 64


def test_hetero_dict_linear():
    lin = HeteroDictLinear({'a': 3, 'b': 5}, 4)
    assert list(lin.state_dict()) == ['lins.a.weight', 'lins.a.bias', 'lins.b.weight',
                                      'lins.b.bias']
    x = {'b': torch.randn(6, 5), 'c': torch.randn(2, 9)}
    out = lin(x)
    assert list(out) == ['b']
    assert_close(out['b'], x['b'] @ lin.lins['b'].weight.t() + lin.lins['b'].bias)
    lin2 = HeteroDictLinear(3, 4, types=['u', 'v.w'], bias=False)
    assert list(lin2.state_dict()) == ['lins.u.weight', 'lins.v#w.weight']   # dots as '#'
    assert list(lin2({'v.w': torch.randn(2, 3)})) == ['v.w'] and lin2.types == ['u', 'v.w']
    assert repr(lin2) == ("HeteroDictLinear(in_channels={'u': 3, 'v.w': 3}, out_channels=4, "
                          "bias=False)")
    with pytest.raises(ValueError, match="needs the list of 'types'"):
        HeteroDictLinear(3, 4)
    with pytest.raises(ValueError, match="are not the keys of 'in_channels'"):
        HeteroDictLinear({'a': 3}, 4, types=['b'])
    with pytest.raises(ValueError, match='lazy'):
        HeteroDictLinear(-1, 4, types=['a'])
    with pytest.raises(ValueError, match='lazy'):
        HeteroDictLinear({'a': -1}, 4)


def test_entry_points_validate_without_gpu():
    """pygamd_hetero_spmm / pygamd_hetero_spmm_backward reject bad arguments before any launch."""
    from pytorch_geometric_amd import _build, _lib
    if _build.is_stale() and _build.find_hipcc() is None:
        pytest.skip('library not built and no hipcc here')
    lib = _lib.load()
    P = ctypes.c_void_p
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)  # noqa: E731
    dev = P(16)  # (never dereferenced: every call below is rejected or launches nothing)
    rb, tab = i64(0, 4), i64(8, 10, 1, 8)

    def fwd(row_begin=rb, table=tab, n_et=1, F=8, idx=1, x=ptrs(16), out=ptrs(16), rowptr=dev):
        return lib.pygamd_hetero_spmm(rowptr, dev, idx, row_begin, x, out, table, n_et, F, None,
                                      None)

    assert fwd(n_et=65, row_begin=i64(*range(66))) == 2       # above 64: unsupported
    assert fwd(n_et=0) == 1
    assert fwd(row_begin=None) == 1
    assert fwd(row_begin=i64(1, 4)) == 1                      # must start at 0
    assert fwd(row_begin=i64(0, -1)) == 1                     # decreasing
    assert fwd(idx=7) == 1
    assert fwd(F=-1) == 1
    assert fwd(table=i64(4, 10, 1, 8)) == 1                   # ldx < F
    assert fwd(table=i64(8, 10, 1, 4)) == 1                   # ldo < F
    assert fwd(table=i64(8, 10, 1, 1 << 31)) == 1             # a pitch that does not fit 32 bits
    assert fwd(table=i64(8, -1, 1, 8)) == 1                   # n_src < 0
    assert fwd(table=i64(8, 10, 2, 8)) == 1                   # mean flag
    assert fwd(x=ptrs(None)) == 1 and fwd(out=ptrs(None)) == 1
    assert fwd(x=None) == 1 and fwd(table=None) == 1
    assert fwd(rowptr=None) == 1
    assert fwd(row_begin=i64(0, 0)) == 0                      # no rows: nothing to launch
    assert fwd(F=0, table=i64(0, 10, 1, 0)) == 0

    sb = i64(0, 10)

    def bwd(row_begin=rb, table=i64(8, 1), n_et=1, src_begin=sb, n_nt=1, ld=i64(8), F=8, idx=1,
            grad=ptrs(16), gx=ptrs(16), rowptr_t=dev):
        return lib.pygamd_hetero_spmm_backward(rowptr_t, dev, dev, idx, row_begin, grad, table,
                                               n_et, src_begin, gx, ld, n_nt, F, None)

    assert bwd(n_et=65, row_begin=i64(*range(66))) == 2
    assert bwd(n_nt=65, src_begin=i64(*range(66))) == 2
    assert bwd(n_et=0) == 1 and bwd(n_nt=0) == 1
    assert bwd(src_begin=i64(2, 10)) == 1 and bwd(src_begin=i64(0, -3)) == 1
    assert bwd(idx=3) == 1 and bwd(F=-2) == 1
    assert bwd(table=i64(4, 1)) == 1 and bwd(table=i64(8, 5)) == 1
    assert bwd(ld=i64(4)) == 1
    assert bwd(grad=ptrs(None)) == 1 and bwd(gx=ptrs(None)) == 1
    assert bwd(grad=None) == 1 and bwd(ld=None) == 1
    assert bwd(rowptr_t=None) == 1
    assert bwd(src_begin=i64(0, 0)) == 0
