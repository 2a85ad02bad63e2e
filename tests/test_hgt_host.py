"""nn.HGTConv without a GPU: the class on CPU tensors and the fp64 restatement (tests/_hgt_ref.py)
against the reference's recorded cases (tests/golden/golden_hgt_v1.pt, written by
tests/golden/make_golden_hgt.py), the state-dict interchange, the output-key rules, the
eligibility rules of the fused route on CPU stand-ins and the stacking plan of the handle."""
import pytest
import torch

import _hgt_ref
from _util import assert_close
from pytorch_geometric_amd import _hgt
from pytorch_geometric_amd.nn import HGTConv

G = _hgt_ref.load_golden()
CASES = list(G['cases'])
AWP, PRA, PCP = ('author', 'writes', 'paper'), ('paper', 'rev_writes', 'author'), \
    ('paper', 'cites', 'paper')


def test_the_file_holds_the_cases_the_layer_is_judged_on():
    assert set(CASES) >= {'three_types', 'skip', 'shared', 'empty_missing', 'source_only',
                          'heads1', 'd5'}
    c = G['cases']
    assert len(set(c['three_types']['kwargs']['in_channels'].values())) == 3
    assert c['skip']['kwargs']['in_channels'] == c['skip']['kwargs']['out_channels']
    assert any(ei.size(1) == 0 for ei in c['empty_missing']['edge_index_dict'].values())
    assert len(c['empty_missing']['edge_index_dict']) < len(c['empty_missing']['kwargs']
                                                            ['metadata'][1])
    assert 'venue' in c['source_only']['x_dict'] and 'venue' not in c['source_only']['out']
    assert c['heads1']['kwargs']['heads'] == 1
    assert c['d5']['kwargs']['out_channels'] // c['d5']['kwargs']['heads'] == 5


@pytest.mark.parametrize('name', CASES)
def test_class_on_cpu_reproduces_the_reference(name):
    _hgt_ref.check_class_case(G, name, 'cpu')


@pytest.mark.parametrize('name', CASES)
def test_restatement_in_fp64_reproduces_the_reference(name):
    case = G['cases'][name]
    p = {k: v.double().requires_grad_(True) for k, v in case['state'].items()}
    xs = {t: v.double().requires_grad_(True) for t, v in case['x_dict'].items()}
    out = _hgt_ref.conv(xs, case['edge_index_dict'], p, **case['kwargs'])
    assert list(out) == list(case['out'])
    grads = torch.autograd.grad([out[t] for t in out], list(xs.values()) + list(p.values()),
                                [case['grad_out'][t].double() for t in out], allow_unused=True)
    for t in out:
        assert_close(out[t].float(), case['out'][t], what=f'{name} out[{t}]')
    for t, g in zip(xs, grads):
        assert_close(g.float(), case['grad_x'][t], what=f'{name} grad_x[{t}]')
    got = [None if g is None else g.float() for g in grads[len(xs):]]
    _hgt_ref.check_gradients(name, [(n, None) for n in p], got, case['grad_params'],
                             assert_close, atol=5e-5, rtol=5e-5)


def test_state_dict_interchanges_strictly_and_inits_follow_the_reference():
    case = G['cases']['three_types']
    layer = HGTConv(**case['kwargs'])
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in case['state'].items()}
    assert all(bool((p == 1).all()) for p in layer.skip.values())
    assert all(bool((p == 1).all()) for p in layer.p_rel.values())
    assert layer.k_rel.weight.shape == (2 * 4, 8, 8) and layer.p_rel['paper__in__venue'].shape \
        == (1, 2)
    missing = layer.load_state_dict(case['state'], strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys


def test_constructor_refusals():
    meta = (['author', 'paper'], [AWP, PRA])
    with pytest.raises(ValueError, match=r"'out_channels' \(got 10\) must be divisible by the "
                                         r"number of heads \(got 4\)"):
        HGTConv(8, 10, meta, heads=4)
    with pytest.raises(ValueError, match='lazy'):
        HGTConv(-1, 8, meta)
    with pytest.raises(ValueError, match='lazy'):
        HGTConv({'author': 8, 'paper': -1}, 8, meta)


def test_output_keys_are_the_metadata_destinations_present_in_x_dict():
    meta = (['author', 'paper', 'venue'], [AWP, PRA, ('paper', 'in', 'venue')])
    layer = HGTConv(8, 8, meta, heads=2).eval()
    g = torch.Generator().manual_seed(5)
    x = {'author': torch.randn(4, 8, generator=g), 'paper': torch.randn(6, 8, generator=g),
         'venue': torch.randn(3, 8, generator=g)}
    ei = {AWP: torch.tensor([[0, 1, 3], [5, 5, 0]])}
    out = layer(x, ei)
    # venue and author are destinations in the metadata: present although no edge reaches them,
    # with no message their rows are out_lin(gelu(0)) = the bias, mixed with the input
    assert list(out) == ['author', 'paper', 'venue']
    a = layer.skip['venue'].sigmoid()
    want = a * layer.out_lin.lins['venue'].bias + (1 - a) * x['venue']
    assert_close(out['venue'], want.expand(3, -1))
    # a node type that is absent from x_dict is absent from the result
    out = layer({t: x[t] for t in ('author', 'paper')}, ei)
    assert list(out) == ['author', 'paper']
    # no edge type at all
    out = layer(x, {})
    assert list(out) == ['author', 'paper', 'venue'] and out['paper'].shape == (6, 8)
    with pytest.raises(KeyError):
        layer(x, {('paper', 'likes', 'paper'): torch.zeros(2, 0, dtype=torch.long)})


def test_edge_type_order_of_the_call_does_not_matter():
    case = G['cases']['three_types']
    layer = HGTConv(**case['kwargs']).eval()
    layer.load_state_dict(case['state'])
    out = layer(case['x_dict'], dict(reversed(list(case['edge_index_dict'].items()))))
    for t in case['out']:
        assert_close(out[t], case['out'][t], what=t)


def _stand_in(**kw):
    case = G['cases']['skip']
    layer = HGTConv(**dict(case['kwargs'], **kw))
    ets = list(case['edge_index_dict'])
    return layer, case['x_dict'], ets, case['edge_index_dict']


def test_fused_route_eligibility_on_cpu_stand_ins():
    def ok(layer, x, ets, eis):
        return _hgt.eligible(layer, x, ets, eis, require_device=False)

    layer, x, ets, eis = _stand_in()
    assert ok(layer, x, ets, eis)
    assert not _hgt.eligible(layer, x, ets, eis)               # CPU tensors, device required
    layer.fuse = False
    assert not ok(layer, x, ets, eis)
    assert not ok(_stand_in(flow='target_to_source')[0], x, ets, eis)
    for register in ('register_propagate_forward_pre_hook', 'register_propagate_forward_hook',
                     'register_message_forward_pre_hook', 'register_message_forward_hook'):
        hooked = _stand_in()[0]
        handle = getattr(hooked, register)(lambda *a: None)
        assert not ok(hooked, x, ets, eis), register
        handle.remove()
        assert ok(hooked, x, ets, eis), register
    hooked = _stand_in()[0]
    hooked.register_forward_hook(lambda *a: None)
    assert not ok(hooked, x, ets, eis)
    assert not ok(layer.half(), x, ets, eis)                   # parameters not float32
    layer = _stand_in()[0]
    assert not ok(layer, {t: v.half() for t, v in x.items()}, ets, eis)
    assert not ok(layer, {t: v.double() for t, v in x.items()}, ets, eis)
    mixed = dict(eis)
    mixed[ets[0]] = mixed[ets[0]].int()
    assert not ok(layer, x, ets, mixed)                        # two index dtypes
    assert ok(layer, x, ets, {et: ei.int() for et, ei in eis.items()})
    # head layouts: D <= 128, H <= 64, H * D <= 512
    meta = (['author', 'paper'], [AWP, PRA, PCP])
    for width, heads, want in ((128, 1, True), (256, 1, False), (512, 4, True), (1024, 8, False),
                               (130, 65, False), (64, 64, True)):
        big = HGTConv(4, width, meta, heads=heads)
        xs = {t: torch.zeros(2, 4) for t in meta[0]}
        assert ok(big, xs, ets, eis) is want, (width, heads)


def test_message_hooks_are_honoured_by_propagate():
    layer, x, ets, eis = _stand_in()
    layer = layer.eval()
    seen = []
    want = layer(x, eis)
    layer.register_message_forward_hook(lambda mod, args, out: seen.append(out.shape))
    # (host tensors do not go through propagate: the hook is a device-route matter; here the
    # registration only has to leave the result alone)
    got = layer(x, eis)
    for t in want:
        assert torch.equal(got[t], want[t])


def test_stacking_offsets():
    st = _hgt.Stacking({'author': 20, 'paper': 30, 'venue': 0}, [AWP, PRA, PCP])
    assert st.dst_off == {'author': 0, 'paper': 20, 'venue': 50} and st.num_dst == 50
    # paper is stacked twice on the source side, once per relation that reads it
    assert st.src_off == [0, 20, 50] and st.num_src == 80
    assert _hgt.Stacking({'a': 3}, []).num_src == 0


def test_stacked_edge_list_on_the_host():
    """The builder's arithmetic on CPU tensors (the handle's sorted forms are device work)."""
    st = _hgt.Stacking({'author': 4, 'paper': 6}, [AWP, PRA, PCP])
    eis = [torch.tensor([[0, 3], [5, 0]]), torch.zeros(2, 0, dtype=torch.long),
           torch.tensor([[1], [2]])]
    h = _hgt.build_stacked(st, eis)
    assert h.sparse_size == (4 + 6 + 6, 10)
    assert h.edge_index.tolist() == [[0, 3, 10 + 1], [4 + 5, 4 + 0, 4 + 2]]
    bad = [eis[0], eis[1], torch.tensor([[6], [2]])]
    with pytest.raises(IndexError, match=r"edge type \('paper', 'cites', 'paper'\) outside the "
                                         r"valid range \[0, 5\] of its source node type"):
        _hgt.build_stacked(st, bad)
