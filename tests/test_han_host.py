"""nn.HANConv without a GPU: the class on CPU tensors (the generic route) and the fp64 restatement
(tests/_han_ref.py) against the reference's recorded cases (tests/golden/golden_han_v1.pt, written
by tests/golden/make_golden_han.py), the state-dict interchange, the ``None`` / zero-row / order
rules, the eligibility rules of the fused route on CPU stand-ins and the stacking plan."""
import pytest
import torch

import _han_ref
from _util import assert_close
from pytorch_geometric_amd import _build, _han, _lib
from pytorch_geometric_amd.nn import HANConv
from pytorch_geometric_amd.nn.conv import HANConv as HANConv2

G = _han_ref.load_golden()
CASES = list(G['cases'])
AWP, ARP, PRA, PCP = ('author', 'writes', 'paper'), ('author', 'reviews', 'paper'), \
    ('paper', 'rev_writes', 'author'), ('paper', 'cites', 'paper')


def test_the_file_holds_the_cases_the_layer_is_judged_on():
    assert HANConv is HANConv2
    assert CASES == ['three_types', 'shared', 'empty_missing', 'source_only', 'heads1', 'd5',
                     'no_venue_rows']
    c = G['cases']
    assert c['three_types']['beta']['paper'].shape == (2, )
    assert [et[0::2] for et in c['shared']['edge_index_dict']][:2] == [('author', 'paper')] * 2
    assert any(ei.size(1) == 0 for ei in c['empty_missing']['edge_index_dict'].values())
    assert len(c['empty_missing']['edge_index_dict']) < len(c['empty_missing']['kwargs']
                                                            ['metadata'][1])
    assert 'lin_src.paper__cites__paper' not in c['empty_missing']['grad_params']
    assert c['source_only']['none'] == ['venue']
    assert c['heads1']['kwargs']['heads'] == 1
    assert c['d5']['kwargs']['out_channels'] // c['d5']['kwargs']['heads'] == 5
    assert c['no_venue_rows']['out']['venue'].shape == (0, 16)
    assert 'venue' not in c['no_venue_rows']['beta']
    for case in c.values():   # no value near a kink (make_golden_han.py refuses such seeds)
        assert float(case['margin_leaky']) >= 1e-4 and float(case['margin_relu']) >= 1e-4


@pytest.mark.parametrize('name', CASES)
def test_class_on_cpu_reproduces_the_reference(name):
    _han_ref.check_class_case(G, name, 'cpu', assert_close)


@pytest.mark.parametrize('name', CASES)
def test_restatement_in_fp64_reproduces_the_reference(name):
    case = G['cases'][name]
    p = {k: v.double().requires_grad_(True) for k, v in case['state'].items()}
    xs = {t: v.double().requires_grad_(True) for t, v in case['x_dict'].items()}
    out, beta = _han_ref.layer(p, xs, case['edge_index_dict'], case['kwargs']['heads'])
    assert [t for t in out if out[t] is None] == case['none']
    for t, want in case['out'].items():
        assert_close(out[t].float(), want, what=f'{name} out[{t}]')
        if t in case['beta']:
            assert_close(beta[t].float(), case['beta'][t], what=f'{name} beta[{t}]')
        else:
            assert beta[t] is None
    diff = [t for t in case['out'] if out[t].requires_grad]
    grads = torch.autograd.grad([out[t] for t in diff], list(xs.values()) + list(p.values()),
                                [case['grad_out'][t].double() for t in diff], allow_unused=True)
    for t, g in zip(xs, grads):
        if t in case['grad_x']:
            assert_close(g.float(), case['grad_x'][t], what=f'{name} grad_x[{t}]')
    for n, g in zip(p, grads[len(xs):]):
        if n in case['grad_params']:
            assert_close(g.float(), case['grad_params'][n], what=f'{name} grad {n}')
        else:
            assert g is None or not bool(g.any()), n


def test_state_dict_interchanges_strictly():
    case = G['cases']['three_types']
    layer = HANConv(**case['kwargs'])
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in case['state'].items()}
    assert list(layer.state_dict()) == list(case['state'])
    assert {'q', 'k_lin.weight', 'k_lin.bias', 'proj.venue.weight', 'proj.venue.bias',
            'lin_src.paper__in__venue', 'lin_dst.paper__in__venue'} <= set(layer.state_dict())
    missing = layer.load_state_dict(case['state'], strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    assert repr(layer) == 'HANConv(16, heads=2)'


def test_constructor_refusals():
    meta = (['author', 'paper'], [AWP, PRA])
    with pytest.raises(ValueError, match=r"'out_channels' \(got 10\) must be divisible by the "
                                         r"number of heads \(got 4\)"):
        HANConv(8, 10, meta, heads=4)
    with pytest.raises(ValueError, match='lazy'):
        HANConv(-1, 8, meta)


def test_none_zero_row_and_key_rules():
    case = G['cases']['source_only']
    layer = HANConv(**case['kwargs']).eval()
    layer.load_state_dict(case['state'])
    out, beta = layer(case['x_dict'], case['edge_index_dict'],
                      return_semantic_attention_weights=True)
    assert out['venue'] is None and beta['venue'] is None
    plain = layer(case['x_dict'], case['edge_index_dict'])
    assert isinstance(plain, dict) and plain['venue'] is None
    case = G['cases']['no_venue_rows']
    layer = HANConv(**case['kwargs']).eval()
    out, beta = layer(case['x_dict'], case['edge_index_dict'],
                      return_semantic_attention_weights=True)
    assert out['venue'].shape == (0, 16) and beta['venue'] is None
    with pytest.raises(KeyError):   # an edge type that is not in the metadata
        layer(case['x_dict'], {('paper', 'likes', 'paper'): torch.zeros(2, 0, dtype=torch.long)})
    with pytest.raises(KeyError):   # an edge type whose endpoint features are missing
        layer({'author': case['x_dict']['author']}, {AWP: case['edge_index_dict'][AWP]})


def test_beta_follows_the_order_of_edge_index_dict():
    case = G['cases']['three_types']
    layer = HANConv(**case['kwargs']).eval()
    layer.load_state_dict(case['state'])
    eis = case['edge_index_dict']
    assert [et for et in eis if et[-1] == 'paper'] == [AWP, PCP]
    out, beta = layer(case['x_dict'], dict(reversed(list(eis.items()))),
                      return_semantic_attention_weights=True)
    assert_close(beta['paper'], case['beta']['paper'].flip(0))
    assert float((case['beta']['paper'][0] - case['beta']['paper'][1]).abs()) > 1e-3
    for t, want in case['out'].items():
        assert_close(out[t], want, what=t)


def _stand_in(case='shared', **kw):
    case = G['cases'][case]
    layer = HANConv(**dict(case['kwargs'], **kw))
    return layer, case['x_dict'], list(case['edge_index_dict']), case['edge_index_dict']


def test_fused_route_eligibility_on_cpu_stand_ins():
    def ok(layer, x, ets, eis):
        return _han.eligible(layer, x, ets, eis, require_device=False)

    layer, x, ets, eis = _stand_in()
    assert layer.fuse is _han.FUSE_DEFAULT
    layer.fuse = True
    assert ok(layer, x, ets, eis)
    assert not _han.eligible(layer, x, ets, eis)               # CPU tensors, device required
    layer.fuse = False
    assert not ok(layer, x, ets, eis)
    # dropout on the coefficients: generic while training, eligible in eval
    drop = _stand_in(dropout=0.5)[0]
    drop.fuse = True
    assert drop.training and not ok(drop, x, ets, eis)
    assert ok(drop.eval(), x, ets, eis)
    t2s = _stand_in(flow='target_to_source')[0]
    t2s.fuse = True
    assert not ok(t2s, x, ets, eis)
    for register in ('register_propagate_forward_pre_hook', 'register_propagate_forward_hook',
                     'register_message_forward_pre_hook', 'register_message_forward_hook'):
        hooked = _stand_in()[0]
        hooked.fuse = True
        handle = getattr(hooked, register)(lambda *a: None)
        assert not ok(hooked, x, ets, eis), register
        handle.remove()
        assert ok(hooked, x, ets, eis), register

    class Own(HANConv):
        def message(self, x_j, alpha_i, alpha_j, index, ptr, size_i):
            return super().message(x_j, alpha_i, alpha_j, index, ptr, size_i)

    own = Own(**G['cases']['shared']['kwargs'])
    own.fuse = True
    assert not ok(own, x, ets, eis)
    layer = _stand_in()[0]
    layer.fuse = True
    assert not ok(layer.half(), x, ets, eis)                   # parameters not float32
    layer = _stand_in()[0]
    layer.fuse = True
    assert not ok(layer, {t: v.half() for t, v in x.items()}, ets, eis)
    mixed = dict(eis)
    mixed[ets[0]] = mixed[ets[0]].int()
    assert not ok(layer, x, ets, mixed)                        # two index dtypes
    assert ok(layer, x, ets, {et: ei.int() for et, ei in eis.items()})
    # head layouts: H <= 64, H * D <= 512 (D alone is not bounded)
    meta = (['author', 'paper'], [AWP, ARP, PRA])
    for width, heads, want in ((256, 1, True), (512, 4, True), (1024, 8, False),
                               (130, 65, False), (64, 64, True)):
        big = HANConv(4, width, meta, heads=heads)
        big.fuse = True
        xs = {t: torch.zeros(2, width) for t in meta[0]}
        assert ok(big, xs, ets, eis) is want, (width, heads)
    # at most 64 edge types in the call
    many = [('author', f'r{i}', 'paper') for i in range(65)]
    wide = HANConv(4, 8, (['author', 'paper'], many), heads=2)
    wide.fuse = True
    xs = {t: torch.zeros(3, 8) for t in ('author', 'paper')}
    ei = torch.tensor([[0, 1], [2, 0]])
    assert ok(wide, xs, many[:64], {et: ei for et in many[:64]})
    assert not ok(wide, xs, many, {et: ei for et in many})


def test_stacking_plan_of_a_node_type_that_feeds_three_edge_types():
    PIV = ('paper', 'in', 'venue')
    st = _han.Stacking({'author': 20, 'paper': 30, 'venue': 6}, [PCP, AWP, PRA, PIV])
    assert st.node_off == {'author': 0, 'paper': 20, 'venue': 50} and st.num_nodes == 56
    # rows: (edge type, destination) blocks; columns: sources stacked by edge type
    assert st.row_begin == [0, 30, 60, 80, 86] and st.num_rows == 86
    assert st.src_begin == [0, 30, 50, 80, 110] and st.num_cols == 110
    # paper feeds three edge types and is stacked ONCE: every block of columns shifts back onto
    # the same 30 feature rows
    assert st.val_shift == [20 - 0, 0 - 30, 20 - 50, 20 - 80]
    for e, et in enumerate(st.edge_types):
        assert st.src_begin[e] + st.val_shift[e] == st.node_off[et[0]]
    assert st.types == (tuple(st.row_begin), tuple(st.src_begin), tuple(st.val_shift))


def test_stacked_edge_list_on_the_host():
    """The builder's arithmetic on CPU tensors (the handle's sorted forms are device work)."""
    st = _han.Stacking({'author': 4, 'paper': 6}, [AWP, PRA, PCP])
    eis = [torch.tensor([[0, 3], [5, 0]]), torch.zeros(2, 0, dtype=torch.long),
           torch.tensor([[1], [2]])]
    h = _han.build_stacked(st, eis)
    assert h.sparse_size == (4 + 6 + 6, 6 + 4 + 6)
    assert h.edge_index.tolist() == [[0, 3, 10 + 1], [5, 0, 10 + 2]]
    bad = [eis[0], eis[1], torch.tensor([[6], [2]])]
    with pytest.raises(IndexError, match=r"edge type \('paper', 'cites', 'paper'\) outside the "
                                         r"valid range \[0, 5\] of its source node type"):
        _han.build_stacked(st, bad)


def test_the_c_abi_lists_the_five_entry_points():
    for sym in ('pygamd_han_supported', 'pygamd_han_workspace_bytes', 'pygamd_han_forward',
                'pygamd_han_backward_dst', 'pygamd_han_backward_src'):
        assert sym in _lib.SIGNATURES, sym
    assert 'han.hip' in _build.SOURCES
    assert _lib.ABI_VERSION == 11
    import pytorch_geometric_amd.ops as ops
    assert 'han_attend' in ops.OPS and 'han_attend_backward' in ops.OPS


def test_fuse_follows_the_environment_read_at_import():
    import os
    import subprocess
    import sys
    here = os.environ.get('PYGAMD_FUSE_HAN', '1') not in ('', '0')
    assert _han.FUSE_DEFAULT is here
    assert HANConv(**G['cases']['heads1']['kwargs']).fuse is here
    code = ("from pytorch_geometric_amd.nn import HANConv; "
            "print(HANConv(4, 8, (['a'], [('a', 'r', 'a')]), heads=2).fuse)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (('1', 'True'), ('0', 'False')):
        env = dict(os.environ, PYGAMD_FUSE_HAN=value,
                   PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
        res = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True,
                             text=True, cwd=root)
        assert res.returncode == 0, res.stderr
        assert res.stdout.split()[-1] == want, (value, res.stdout)
