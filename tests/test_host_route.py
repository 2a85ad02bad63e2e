"""The host route of ``MessagePassing`` without a GPU: ``nn/_host.py``'s softmax and aggregation
formulas against float64 loops over the groups, the operators still refusing host tensors, the
reference's index errors of ``propagate``, and no ``forward`` writing ``self.fuse``."""
import math

import pytest
import torch

import _host_route_cases as C
import pytorch_geometric_amd as pga
from _aggr_cases import CASES as TEMPERED
from _util import assert_close, assert_close_scaled, gen
from pytorch_geometric_amd.nn import _host, aggr as A

N, E, F = 12, 40, 6
INDEX = torch.randint(0, N, (E, ), generator=gen(70))
INDEX[INDEX == 7] = 3                                    # group 7 is empty
X = torch.randn(E, F, generator=gen(71))
GRAD = torch.randn(N, 16 * F, generator=gen(72))         # cut to the width of each result
DEG_HIST = torch.tensor([1, 3, 6, 9, 7, 4, 2])


# ---- float64 restatements, one group at a time ------------------------------------------------
def grouped(fn, x):
    """``fn(rows of group i)`` stacked over the groups; ``fn`` sees ``[0, F]`` for an empty one"""
    return torch.stack([fn(x[INDEX == i]) for i in range(N)])


def or_zero(fn):
    return lambda rows: fn(rows) if rows.size(0) else rows.new_zeros(rows.shape[1:])


def mean(rows):
    return rows.sum(0) / max(rows.size(0), 1)


def var(rows):
    return mean(rows * rows) - mean(rows) ** 2


def std(rows):
    out = var(rows).clamp(min=1e-5).sqrt()
    return out.masked_fill(out <= math.sqrt(1e-5), 0.0)


def softmax_sum(t, semi_grad):
    def fn(rows):
        z = rows * t
        e = (z - z.detach().max(0).values).exp()
        w = e / (e.sum(0) + 1e-16)
        return (rows * (w.detach() if semi_grad else w)).sum(0)
    return or_zero(fn)


def powermean(p, lo=1e-4, hi=100.):
    if not isinstance(p, torch.Tensor) and p == 1:
        return mean
    return lambda rows: mean(rows.clamp(lo, hi).pow(p)).clamp(lo, hi).pow(1. / p)


SIMPLE = {'sum': lambda rows: rows.sum(0), 'mean': mean,
          'min': or_zero(lambda rows: rows.min(0).values),
          'max': or_zero(lambda rows: rows.max(0).values), 'var': var, 'std': std}
COMBINE = {'cat': lambda s: torch.cat(list(s), dim=-1), 'sum': lambda s: s.sum(0),
           'mean': lambda s: s.mean(0), 'max': lambda s: s.max(0).values,
           'min': lambda s: s.min(0).values}


def degree_scaled(out, scalers):
    deg = torch.bincount(INDEX, minlength=N).double().view(-1, 1)
    hist, bins = DEG_HIST.double(), torch.arange(DEG_HIST.numel()).double()
    # (the module keeps the two averages in float32)
    lin = float(torch.tensor(float((bins * hist).sum() / hist.sum()), dtype=torch.float32))
    log = float(torch.tensor(float(((bins + 1).log() * hist).sum() / hist.sum()),
                             dtype=torch.float32))
    by_name = {'identity': out, 'amplification': out * ((deg + 1).log() / log),
               'attenuation': out * (log / (deg.clamp(min=1) + 1).log()),
               'linear': out * (deg / lin), 'inverse_linear': out * (lin / deg.clamp(min=1))}
    return torch.cat([by_name[s] for s in scalers], dim=-1)


def tempered_case(name):
    kind, kw, _, positive = TEMPERED[name]
    module = (A.SoftmaxAggregation if kind == 'softmax' else A.PowerMeanAggregation)(**kw)

    def ref(x, params):
        value = params[0] if params else kw.get('t', kw.get('p', 1.0))
        fn = softmax_sum(value, kw.get('semi_grad', False)) if kind == 'softmax' \
            else powermean(value)
        return grouped(fn, x)
    return module, ref, positive


SCALERS = ['identity', 'amplification', 'attenuation', 'linear', 'inverse_linear']
MEMBERS = ['sum', 'mean', 'min', 'max', 'var', 'std']
# name -> (module, float64 restatement of (x, parameters), positive inputs)
MODULES = {
    **{n: (lambda n=n: (A.aggregation_resolver(n), lambda x, p: grouped(SIMPLE[n], x), False))
       for n in ('sum', 'mean', 'min', 'max')},
    'var': lambda: (A.VarAggregation(), lambda x, p: grouped(var, x), False),
    'std': lambda: (A.StdAggregation(), lambda x, p: grouped(std, x), False),
    **{n: (lambda n=n: tempered_case(n)) for n in TEMPERED},
    **{f'multi_{mode}': (lambda mode=mode: (
        A.MultiAggregation(MEMBERS, mode=mode),
        lambda x, p: COMBINE[mode](torch.stack([grouped(SIMPLE[m], x) for m in MEMBERS])),
        False)) for mode in COMBINE},
    'multi_one': lambda: (A.MultiAggregation(['max']),
                          lambda x, p: grouped(SIMPLE['max'], x), False),
    'degree_scaler': lambda: (
        A.DegreeScalerAggregation(['mean', 'min', 'std'], SCALERS, DEG_HIST),
        lambda x, p: degree_scaled(torch.cat([grouped(SIMPLE[m], x)
                                              for m in ('mean', 'min', 'std')], dim=-1), SCALERS),
        False),
}


@pytest.mark.parametrize('name', list(MODULES))
def test_aggregate_against_a_float64_loop(name):
    """Results and gradients are float32 sums of at most 40 terms of magnitude O(1) set against
    float64: a rounding error of some ``40 * 2^-24 = 2.4e-6`` of the magnitude, inside the
    project's 1e-5 (results, per element) and 2e-5 of the tensor's scale (gradients)."""
    module, ref, positive = MODULES[name]()
    x = (X.abs() + 0.1 if positive else X).clone().requires_grad_(True)
    params = list(module.parameters())
    out = _host.aggregate(module, x, INDEX.int(), N)
    x64 = x.detach().double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    want = ref(x64, p64)
    assert_close(out, want.float(), what=name)
    grad = GRAD[:, :out.size(1)]
    got = torch.autograd.grad(out, [x] + params, grad)
    exp = torch.autograd.grad(want, [x64] + p64, grad.double())
    for g, e, what in zip(got, exp, ['x'] + [n for n, _ in module.named_parameters()]):
        assert_close_scaled(g, e.float(), what=f'{name} grad {what}')


def test_semi_grad_holds_the_softmax_weights_constant():
    x = X.clone().requires_grad_(True)
    grads = []
    for semi in (False, True):
        module = A.SoftmaxAggregation(t=2.0, semi_grad=semi)
        out = _host.aggregate(module, x, INDEX, N)
        grads.append(torch.autograd.grad(out, x, GRAD[:, :F])[0])
        x64 = X.double().requires_grad_(True)
        want = torch.autograd.grad(grouped(softmax_sum(2.0, semi), x64), x64,
                                   GRAD[:, :F].double())[0]
        assert_close_scaled(grads[-1], want.float(), what=f'semi_grad={semi}')
    assert not torch.allclose(grads[0], grads[1], atol=1e-3)


def test_aggregate_takes_trailing_dimensions_and_refuses_unknown_modules():
    x = torch.randn(E, 3, F, generator=gen(73))
    out = _host.aggregate(A.SumAggregation(), x, INDEX, N)
    assert_close(out, grouped(lambda rows: rows.sum(0), x.double()).float())
    with pytest.raises(NotImplementedError, match='MulAggregation'):
        _host.aggregate(A.MulAggregation(), X, INDEX, N)


@pytest.mark.parametrize('heads', [None, 3])
def test_softmax_against_a_float64_loop(heads):
    """Same bound as above: at most 40 terms in a group's denominator."""
    src = torch.randn((E, ) if heads is None else (E, heads), generator=gen(74)) * 3
    src.requires_grad_(True)
    out = _host.softmax(src, INDEX.int(), None, N)
    s64 = src.detach().double().requires_grad_(True)
    want = torch.zeros_like(s64)
    for i in range(N):
        rows = s64[INDEX == i]
        if rows.size(0):
            e = (rows - rows.detach().max(0).values).exp()
            want = want.index_put((torch.nonzero(INDEX == i).view(-1), ), e / (e.sum(0) + 1e-16))
    assert_close(out, want.float())
    grad = torch.randn(src.shape, generator=gen(75))
    assert_close_scaled(torch.autograd.grad(out, src, grad)[0],
                        torch.autograd.grad(want, s64, grad.double())[0].float())
    # the number of groups defaults to the largest index + 1
    assert torch.equal(_host.softmax(src, INDEX), out)
    assert _host.softmax(src[:0], INDEX[:0]).shape == src[:0].shape


def test_the_operators_still_refuse_host_tensors():
    for module in (A.SumAggregation(), A.MeanAggregation(), A.MaxAggregation(),
                   A.StdAggregation(), A.SoftmaxAggregation(), A.PowerMeanAggregation(p=2.0),
                   A.MultiAggregation(['mean', 'max']),
                   A.DegreeScalerAggregation(['mean'], ['identity'], DEG_HIST)):
        with pytest.raises(pga.PygAmdError, match='no CPU fallback'):
            module(X, INDEX, dim_size=N)
    with pytest.raises(pga.PygAmdError, match='no CPU fallback'):
        pga.utils.softmax(X, INDEX, num_nodes=N)
    with pytest.raises(pga.PygAmdError, match='no CPU fallback'):
        pga.utils.scatter(X, INDEX, dim_size=N)


def test_propagate_on_host_tensors_raises_the_reference_index_errors():
    conv = pga.nn.GINConv(torch.nn.Linear(F, 4))
    x = torch.randn(5, F)
    with pytest.raises(IndexError, match=r"larger than 4 \(got 9\)"):
        conv(x, torch.tensor([[0, 9], [1, 2]]))
    with pytest.raises(IndexError, match=r"negative indices in 'edge_index' \(got -2\)"):
        conv(x, torch.tensor([[0, -2], [1, 2]]))


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64], ids=['int32', 'int64'])
@pytest.mark.parametrize('name', C.NAMES)
def test_forward_does_not_write_fuse(name, dtype):
    layer, inputs = C.make(name)
    writes = C.recording(layer)
    before = layer.fuse
    outs = C.run(name, layer, inputs, dtype)
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    assert writes == [] and layer.fuse is before
