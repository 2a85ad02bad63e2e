"""The two autograd routes of every one-pass family — the ``torch.autograd.Function`` on an
``EdgeIndex`` handle and the ``torch.ops.pyg_amd.*`` operator on ``(rowptr, col)`` — on the same
inputs: every output both return and every gradient bit for bit, and the same sequence of the
family's C calls in the backward.  The inputs are the smallest that reach every branch of the
bodies the routes share (pytorch_geometric_amd/_onepass.py): destinations a prefix of a longer
tensor, a chunked row in each sorted form, destinations and sources without slots.  The edge list
is sorted by destination, so that a stable sort by source is the same permutation on both routes
(for any other order the routes order the slots of a source differently and may differ in the last
bit)."""
import pytest
import torch

from _util import _counted, gen

pytestmark = pytest.mark.gpu

N_SRC, N_DST, ROWS = 1300, 1100, 1300  # the destination-side tensors have ROWS >= N_DST rows
H, C, W, DE = 2, 12, 24, 3
INDEX = pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32], ids=['int64', 'int32'])


@pytest.fixture(scope='module')
def coo():
    """``[2, E]`` sorted by destination (stable): destination 3 fed by HUB_THRESHOLD + 1 distinct
    sources, source 7 feeding HUB_THRESHOLD + 1 distinct destinations, 2,000 random edges;
    destinations >= 1050 and sources >= 1250 stay without a slot."""
    from pytorch_geometric_amd import _native
    long, g = _native.HUB_THRESHOLD + 1, gen(5)
    src = torch.cat([torch.randperm(1250, generator=g)[:long], torch.full((long, ), 7),
                     torch.randint(0, 1250, (2000, ), generator=g)])
    dst = torch.cat([torch.full((long, ), 3), torch.randperm(1050, generator=g)[:long],
                     torch.randint(0, 1050, (2000, ), generator=g)])
    order = torch.sort(dst, stable=True).indices
    return torch.stack([src[order], dst[order]])


def _handle(coo, dev, index_dtype):
    from pytorch_geometric_amd import as_edge_index
    graph = as_edge_index(coo.to(dev).to(index_dtype), N_SRC, N_DST)
    fwd = graph.by_dst()
    return graph, fwd.ptr, fwd.idx


def _randn(seed, *shape):
    return torch.randn(*shape, generator=gen(seed))


def _agree(monkeypatch, dev, prefix, inputs, handle_route, operator_route):
    """Runs both routes on fresh leaves of ``inputs`` (None: an input that is not given); each
    returns the tuple of outputs the two have in common."""
    import pytorch_geometric_amd.ops  # noqa: F401 (registers torch.ops.pyg_amd)
    runs = []
    for route in (handle_route, operator_route):
        leaves = [None if t is None else t.to(dev).requires_grad_(True) for t in inputs]
        outs = route(*leaves)
        grad_outs = [_randn(70 + i, *o.shape).to(dev) for i, o in enumerate(outs)]
        given = [t for t in leaves if t is not None]
        state = {}
        c = _counted(monkeypatch,
                     lambda: state.update(grads=torch.autograd.grad(outs, given, grad_outs)))
        runs.append(([o.detach() for o in outs], state['grads'],
                     [name for name in c.order if name.startswith(prefix)]))
    (outs_h, grads_h, calls_h), (outs_o, grads_o, calls_o) = runs
    for i, (a, b) in enumerate(zip(outs_h, outs_o, strict=True)):
        assert torch.equal(a, b), f'output {i} differs between the routes'
    for i, (a, b) in enumerate(zip(grads_h, grads_o, strict=True)):
        assert a.shape == b.shape and torch.equal(a, b), \
            f'the gradient of given input {i} differs between the routes'
    assert calls_h == calls_o and any('backward' in name for name in calls_h), (calls_h, calls_o)


@INDEX
def test_gatv2(dev, monkeypatch, coo, index_dtype):
    from pytorch_geometric_amd._functions import Gatv2AttendFunction
    graph, rowptr, col = _handle(coo, dev, index_dtype)
    inputs = [_randn(1, N_SRC, H, C), _randn(2, ROWS, H, C), _randn(3, 1, H, C)]
    _agree(monkeypatch, dev, 'pygamd_gatv2_', inputs,
           lambda x_l, x_r, att: (Gatv2AttendFunction.apply(x_l, x_r, att, graph, 0.2, N_DST), ),
           lambda x_l, x_r, att: torch.ops.pyg_amd.gatv2_attend(x_l, x_r, att, rowptr, col,
                                                                0.2)[:1])


@INDEX
def test_transformer(dev, monkeypatch, coo, index_dtype):
    from pytorch_geometric_amd._functions import TransformerAttendFunction
    graph, rowptr, col = _handle(coo, dev, index_dtype)
    inputs = [_randn(1, ROWS, H, C), _randn(2, N_SRC, H, C), _randn(3, N_SRC, H, C)]
    _agree(monkeypatch, dev, 'pygamd_transformer_', inputs,
           lambda q, k, v: (TransformerAttendFunction.apply(q, k, v, graph, 0.3, N_DST), ),
           lambda q, k, v: torch.ops.pyg_amd.transformer_attend(q, k, v, rowptr, col, 0.3)[:1])


@INDEX
def test_transformer_edge(dev, monkeypatch, coo, index_dtype):
    from pytorch_geometric_amd._functions import TransformerEdgeAttendFunction
    graph, rowptr, col = _handle(coo, dev, index_dtype)
    inputs = [_randn(1, ROWS, H, C), _randn(2, N_SRC, H, C), _randn(3, N_SRC, H, C),
              _randn(4, coo.size(1), DE), _randn(5, ROWS, H, DE)]
    # ('pygamd_transformer_': the edge calls and the by-source launch of the plain family)
    _agree(monkeypatch, dev, 'pygamd_transformer_', inputs,
           lambda q, k, v, ea, b: TransformerEdgeAttendFunction.apply(q, k, v, ea, b, graph, 0.3,
                                                                      N_DST),
           lambda q, k, v, ea, b: torch.ops.pyg_amd.transformer_edge_attend(q, k, v, ea, b, rowptr,
                                                                            col, 0.3)[:2])


@INDEX
@pytest.mark.parametrize('mode', ['wide', 'linear'])
def test_gine(dev, monkeypatch, coo, index_dtype, mode):
    from pytorch_geometric_amd._functions import GineAggregateFunction
    graph, rowptr, col = _handle(coo, dev, index_dtype)
    E = coo.size(1)
    inputs = [_randn(1, N_SRC, W), _randn(2, ROWS, W), torch.tensor([0.3])]
    inputs += ([_randn(3, E, W), None, None] if mode == 'wide'
               else [_randn(3, E, DE), _randn(4, W, DE), _randn(5, W)])
    _agree(monkeypatch, dev, 'pygamd_gine_', inputs,
           lambda *t: (GineAggregateFunction.apply(*t, graph, N_DST), ),
           lambda *t: (torch.ops.pyg_amd.gine_aggregate(*t, rowptr, col, None), ))


@INDEX
def test_pna(dev, monkeypatch, coo, index_dtype):
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd._functions import PnaAggregateFunction
    graph, rowptr, col = _handle(coo, dev, index_dtype)
    inputs = [_randn(1, N_SRC, W), _randn(2, ROWS, W), _randn(3, coo.size(1), DE),
              _randn(4, W, DE)]
    _agree(monkeypatch, dev, 'pygamd_pna_', inputs,
           lambda *t: PnaAggregateFunction.apply(*t, graph, N_DST, _native.PNA_STATS),
           lambda *t: torch.ops.pyg_amd.pna_aggregate(*t, rowptr, col, None, 15)[0].unbind(0))


def test_hgt(dev, monkeypatch):
    from pytorch_geometric_amd._functions import HgtRelationPlan, HGTRelationFunction
    D = 8
    F = H * D
    inputs = [_randn(1, 2 * H, D, D), _randn(2, 2 * H, D, D), _randn(3, 40, 3 * F),
              _randn(4, 50, 3 * F)]
    src_pos, widx = [0, 1], [1, 0]
    _agree(monkeypatch, dev, 'pygamd_hgt_', inputs,
           lambda wk, wv, *kqvs: (HGTRelationFunction.apply(HgtRelationPlan(H, src_pos, widx), wk,
                                                            wv, *kqvs), ),
           lambda wk, wv, *kqvs: (torch.ops.pyg_amd.hgt_relation(list(kqvs), wk, wv, src_pos, widx,
                                                                 H), ))
