"""Live-source lists (`pygamd_live_lists_flag` / `pygamd_live_lists_build`, csrc/graph.hip) and the
kernels that walk them through `rowend`: the builder against a stable filter on the host, the row
kernels and the one-kernel SAGE layer on the lists against the same launch on the stored lists, and
the fused GraphSAGE stack with `PYGAMD_LIVE_LISTS=1` against `=0`.  Every comparison is
`torch.equal`.

Where that can hold.  A kernel that gives a whole wave to one source row (more than 128 columns as
16-byte pieces: F = 256 here, and F = 47 / 256 at the headline) adds a row's entries one after the
other, so leaving out rows of exact zeros changes no bit, and those cases run on random floats.  A
narrower row (F = 48, F = 100) is summed as 64 / LPR interleaved partial sums, and which partial
sum an entry joins depends on its POSITION in the list: there the stored and the live lists agree
only up to the order of the additions.  Those cases run on small integers, where every order gives
the same float — they pin which entries are read, which is what the lists change."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 301
FORCED = {3: 0, 10: 1, 20: 63, 40: 64, 77: 65, 150: 129, 299: 300}  # row -> stored entries
BITMAPS = ('none', 'all', 'eight_percent', 'bit300')


def _graph(dtype):
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(0, 41, (N, ), generator=g)
    for r, d in FORCED.items():
        deg[r] = d
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = deg.cumsum(0)
    col = torch.randint(0, N, (int(rowptr[-1]), ), generator=g)
    return rowptr.to(dtype), col.to(dtype)


def _bitmap(kind):
    g = torch.Generator().manual_seed(5)
    if kind == 'none':
        live = torch.zeros(N, dtype=torch.bool)
    elif kind == 'all':
        live = torch.ones(N, dtype=torch.bool)
    elif kind == 'eight_percent':
        live = torch.rand(N, generator=g) < 0.08
    else:
        live = torch.zeros(N, dtype=torch.bool)
        live[300] = True
    return live


def _pack(live):
    words = (live.numel() + 31) // 32
    a = np.zeros(words * 32, dtype=np.uint8)
    a[:live.numel()] = live.numpy().astype(np.uint8)
    return torch.from_numpy(np.packbits(a, bitorder='little').view(np.int32).copy())


def _unpack(bits, n):
    a = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder='little')
    return torch.from_numpy(a[:n].astype(bool))


def _hub(rowptr_d, threshold):
    from pytorch_geometric_amd import _native
    if threshold == 0:
        return None
    hub = _native.hub_plan(rowptr_d, threshold, 64)
    assert hub.n_hub == 2   # the 129- and the 300-entry row
    return hub


def _build(dev, rowptr, col, live, hub, flag_value=1, n_set=None, sentinel=None):
    from pytorch_geometric_amd import _native
    rp, cl = rowptr.to(dev), col.to(dev)
    flag = torch.full((1, ), flag_value, dtype=torch.int32, device=dev)
    fill = -7 if sentinel is None else sentinel
    col_live = torch.full_like(cl, fill)
    end_live = torch.full((N, ), fill, dtype=rp.dtype, device=dev)
    has = torch.full(((N + 31) // 32, ), fill, dtype=torch.int32, device=dev)
    _native.live_lists_build(rp, cl, N, _pack(live).to(dev), flag, hub=hub, n_set=n_set,
                             col_live=col_live, rowend_live=end_live, row_has_live=has)
    torch.cuda.synchronize()
    return col_live, end_live, has


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('threshold', [0, 128])
@pytest.mark.parametrize('kind', BITMAPS)
def test_builder_equals_a_stable_filter(dev, dtype, threshold, kind):
    rowptr, col = _graph(dtype)
    live = _bitmap(kind)
    hub = _hub(rowptr.to(dev), threshold)
    col_live, end_live, has = _build(dev, rowptr, col, live, hub)
    col_live, end_live = col_live.cpu(), end_live.cpu()
    has = _unpack(has, N)
    assert col_live.dtype == dtype and end_live.dtype == dtype
    for r in range(N):
        s, e = int(rowptr[r]), int(rowptr[r + 1])
        stored = col[s:e]
        keep = live[stored.long()]
        assert bool(has[r]) == bool(keep.any()), f'row_has_live of row {r}'
        if threshold > 0 and e - s > threshold:     # a hub row: copied whole
            assert int(end_live[r]) == e, f'hub row {r} was cut'
            assert torch.equal(col_live[s:e], stored), f'hub row {r} was reordered'
            continue
        want = stored[keep]
        assert int(end_live[r]) == s + want.numel(), f'rowend_live of row {r}'
        assert torch.equal(col_live[s:s + want.numel()], want), f'live prefix of row {r}'
        # the slots behind the prefix: the row's other entries, so always valid column ids
        rest = col_live[s + want.numel():e]
        assert bool(((rest >= 0) & (rest < N)).all()), f'row {r}: a slot is no column id'
        assert torch.equal(rest.sort().values, stored[~keep].sort().values), f'tail of row {r}'
    words = _pack(has)  # the bits past the last row are clear
    assert int(words[-1].item()) >> (N & 31) == 0


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_builder_leaves_everything_alone_when_the_flag_says_unchanged(dev, dtype):
    rowptr, col = _graph(dtype)
    col_live, end_live, has = _build(dev, rowptr, col, _bitmap('eight_percent'), None,
                                     flag_value=0, sentinel=-7)
    assert bool((col_live == -7).all()) and bool((end_live == -7).all())
    assert bool((has == -7).all())


def test_dense_bitmap_gives_pass_through_lists(dev):
    rowptr, col = _graph(torch.int64)
    live = torch.rand(N, generator=torch.Generator().manual_seed(2)) < 0.6
    n_set = torch.tensor([int(live.sum())], dtype=torch.int64, device=dev)
    assert 2 * int(n_set) >= N
    col_live, end_live, _ = _build(dev, rowptr, col, live, None, n_set=n_set)
    assert torch.equal(col_live.cpu(), col) and torch.equal(end_live.cpu(), rowptr[1:])
    # ... and a sparse one under the same test is filtered
    live = _bitmap('eight_percent')
    n_set = torch.tensor([int(live.sum())], dtype=torch.int64, device=dev)
    _, end_live, _ = _build(dev, rowptr, col, live, None, n_set=n_set)
    assert int((rowptr[1:] - end_live.cpu()).sum()) == int((~live[col.long()]).sum())


def test_the_compare_kernel_sees_one_bit_anywhere_and_ignores_the_tail(dev):
    from pytorch_geometric_amd import _native
    assert N % 32 != 0
    live = _bitmap('eight_percent')
    live[300] = False
    live[0] = False
    bits = _pack(live).to(dev)
    stored = torch.zeros_like(bits)
    flag = torch.full((1, ), 5, dtype=torch.int32, device=dev)

    def changed(b, force=False):
        _native.live_lists_flag(b, stored, N, flag, force=force)
        return int(flag.item())

    assert changed(bits) == 1 and torch.equal(stored, bits)   # against the empty copy
    assert changed(bits) == 0
    last = live.clone()
    last[300] = True                                          # only the last word differs
    assert changed(_pack(last).to(dev)) == 1
    assert torch.equal(stored, _pack(last).to(dev))
    assert changed(_pack(last).to(dev)) == 0
    first = last.clone()
    first[0] = True                                           # one bit of the first word
    assert changed(_pack(first).to(dev)) == 1
    assert changed(_pack(first).to(dev)) == 0
    tail = _pack(first).clone()
    tail[-1] |= 1 << 20                                       # bit 308: past the last row
    assert changed(tail.to(dev)) == 0
    assert changed(_pack(first).to(dev), force=True) == 1


def _source(F, live, exact, dev):
    g = torch.Generator().manual_seed(3)
    if exact:
        x = torch.randint(-8, 9, (N, F), generator=g).to(torch.float32)
    else:
        x = torch.randn(N, F, generator=g)
    x[~live] = 0.0      # exact zeros where the bit is clear
    return x.to(dev)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('threshold', [0, 128])
@pytest.mark.parametrize('kind', BITMAPS)
@pytest.mark.parametrize('F,sparse,exact', [(48, True, True), (256, False, False),
                                            (100, False, True)])
def test_row_kernels_on_the_lists_equal_the_stored_lists(dev, dtype, threshold, kind, F, sparse,
                                                         exact):
    from pytorch_geometric_amd import _native
    rowptr, col = _graph(dtype)
    live = _bitmap(kind)
    rp, cl = rowptr.to(dev), col.to(dev)
    hub = _hub(rp, threshold)
    col_live, end_live, _ = _build(dev, rowptr, col, live, hub)
    x = _source(F, live, exact, dev)
    more = {}
    if sparse:  # the R-rows-per-wave kernel of the sparse source
        more = dict(src_bits=_pack(live).to(dev),
                    src_bits_set=torch.tensor([int(live.sum())], dtype=torch.int64, device=dev))
    want = _native.spmm_csr(rp, cl, x, 'sum', n_rows=N, hub=hub, **more)
    got = _native.spmm_csr(rp, col_live, x, 'sum', n_rows=N, hub=hub, rowend=end_live, **more)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_rowend_with_a_hub_plan_stays_refused_off_the_plain_sum(dev):
    from pytorch_geometric_amd import _native
    rowptr, col = _graph(torch.int64)
    rp, cl = rowptr.to(dev), col.to(dev)
    hub = _hub(rp, 128)
    live = _bitmap('all')
    col_live, end_live, _ = _build(dev, rowptr, col, live, hub)
    x = _source(48, live, True, dev)
    w = torch.ones(cl.numel(), device=dev)
    for kw in (dict(reduce='mean'), dict(reduce='sum', w=w),
               dict(reduce='sum', src_scale=torch.ones(N, device=dev)), dict(reduce='min')):
        reduce = kw.pop('reduce')
        with pytest.raises(_native.PygAmdError, match='(?i)unsupported'):
            _native.spmm_csr(rp, col_live, x, reduce, n_rows=N, hub=hub, rowend=end_live, **kw)
    with pytest.raises(_native.PygAmdError, match='(?i)unsupported'):  # min: with or without hubs
        _native.spmm_csr(rp, col_live, x, 'min', n_rows=N, rowend=end_live)


@pytest.mark.parametrize('mode', ['split', 'fp32'])
@pytest.mark.parametrize('kind', ['eight_percent', 'bit300'])
def test_fused_launch_on_the_lists_equals_the_stored_lists(dev, mode, kind):
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd import _native
    F = 256
    rowptr, col = _graph(torch.int64)
    rp, cl = rowptr.to(dev), col.to(dev)
    hub = _hub(rp, 128)
    live = _bitmap(kind)
    col_live, end_live, _ = _build(dev, rowptr, col, live, hub)
    x = _source(F, live, False, dev)
    g = torch.Generator().manual_seed(9)
    root = torch.randn(N, F, generator=g).to(dev)
    w = (torch.randn(F, 2 * F, generator=g) / 16).to(dev)
    mask = torch.randint(-2 ** 31, 2 ** 31 - 1, _native.relu_bits_like(N, F, dev).shape,
                         generator=g, dtype=torch.int64).to(torch.int32).to(dev)
    before = pga.get_gemm_mode()
    pga.set_gemm_mode(mode)
    try:
        outs = []
        for c, end in ((cl, None), (col_live, end_live)):
            scratch = torch.zeros(N, F, device=dev)
            out = torch.empty(N, F, device=dev)
            _native.sage_layer_forward(rp, c, x, root, w, None, 'sum', False, scratch, out,
                                       hub=hub, save_agg=False, mask_bits=mask, rowend=end)
            outs.append(out)
        torch.cuda.synchronize()
    finally:
        pga.set_gemm_mode(before)
    assert torch.equal(outs[1], outs[0])
    assert bool(outs[0].abs().sum() > 0)


# ---- the stack ------------------------------------------------------------------------------------
@pytest.fixture
def data(dev):
    from pytorch_geometric_amd.datasets import products_like
    x, y, ei, c = products_like(seed=1, scale=1 / 1024)
    return x.to(dev), y.to(dev), ei.to(dev), c


@pytest.fixture
def lists_env(monkeypatch):
    import pytorch_geometric_amd as pga
    pga.clear_aggregation_cache()

    def switch(on: bool):
        monkeypatch.setenv('PYGAMD_LIVE_LISTS', '1' if on else '0')

    yield switch
    pga.clear_aggregation_cache()


def _model(dev, c):
    from pytorch_geometric_amd.nn import GraphSAGE
    torch.manual_seed(0)
    return GraphSAGE(100, 256, num_layers=3, out_channels=c).to(dev)


def _splits(n, dev):
    g = torch.Generator().manual_seed(7)
    a = torch.randperm(n, generator=g)[:max(int(0.08 * n), 1)].to(dev)
    b = torch.randperm(n, generator=g)[:max(int(0.08 * n), 1)].to(dev)
    return a, b


def _steps(dev, data, counts=None):
    """gradients of: three steps on split a, one on split b, a dense loss, split a again"""
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.nn.functional import cross_entropy
    x, y, ei, c = data
    model = _model(dev, c)
    a, b = _splits(x.size(0), dev)
    rec = []
    for idx in (a, a, a, b, None, a):
        model.zero_grad(set_to_none=True)
        out = model(x, ei)
        loss = out.sum() if idx is None else cross_entropy(out, y, idx)
        loss.backward()
        torch.cuda.synchronize()
        if counts is not None:
            counts.append(_native.live_lists_builds())
        rec.append([p.grad.clone() for p in model.parameters()])
    return rec


def test_stack_gradients_equal_the_run_without_lists_and_builds_follow_the_pattern(
        dev, data, lists_env):
    from pytorch_geometric_amd import _native
    lists_env(False)
    want = _steps(dev, data)
    lists_env(True)
    torch.cuda.synchronize()
    counts = [_native.live_lists_builds()]
    got = _steps(dev, data, counts)
    for step, (ga, gb) in enumerate(zip(got, want)):
        for i, (ta, tb) in enumerate(zip(ga, gb)):
            assert torch.equal(ta, tb), f'step {step}, gradient {i} differs from the run without'
    # one real build (its two launches: the rows that reach the split, then the lists) per change
    # of pattern, none on a repeated one
    assert [b - a for a, b in zip(counts, counts[1:])] == [2, 0, 0, 2, 2, 2]


def test_clearing_the_cache_and_dropping_the_graph_release_the_buffers(
        dev, data, lists_env, monkeypatch):
    import pytorch_geometric_amd as pga
    from pytorch_geometric_amd.nn.functional import cross_entropy
    monkeypatch.setenv('PYGAMD_CACHE_AGG0', '0')   # (only the lists are kept between steps)
    lists_env(True)
    from pytorch_geometric_amd.edge_index import EdgeIndex
    x, y, ei, c = data
    n = x.size(0)
    graph = EdgeIndex(ei.clone(), (n, n))   # (a handle of the test's own: no cache entry holds it)
    model = _model(dev, c)
    a, _ = _splits(n, dev)

    def step():
        model.zero_grad(set_to_none=True)
        cross_entropy(model(x, graph), y, a).backward()
        torch.cuda.synchronize()

    step()
    handle = graph.by_src()
    assert handle._live is not None and handle._live.col.numel() == handle.idx.numel()
    held = sum(t.numel() * t.element_size() for t in (handle._live.col, handle._live.end))
    before = torch.cuda.memory_allocated()
    pga.clear_aggregation_cache()
    assert handle._live is None
    assert before - torch.cuda.memory_allocated() >= held
    step()
    assert handle._live is not None
    before = torch.cuda.memory_allocated()
    del handle, graph
    gc.collect()
    assert before - torch.cuda.memory_allocated() >= held


def test_a_captured_step_bypasses_the_lists_and_equals_eager(dev, data, lists_env):
    """The eager leg walks the lists, the captured one the stored lists: equal bit for bit.  Both
    legs take the loss as `F.cross_entropy(out[a], y[a])`: the package's one-pass
    `cross_entropy(out, y, a)` switches to exactly that form by itself under capture
    (_functions.cross_entropy), and the two forms differ in the last bits of the loss gradient
    (1e-10 .. 4e-9 in the parameter gradients of this model, with the lists on or off alike) —
    a difference of the loss routes, not of the stack under test."""
    from pytorch_geometric_amd import _native
    from pytorch_geometric_amd.hipgraph import CapturedStep
    lists_env(True)
    x, y, ei, c = data
    model = _model(dev, c)
    a, _ = _splits(x.size(0), dev)
    ya = y[a]
    for p in model.parameters():
        p.grad = torch.zeros_like(p)

    def step():
        model.zero_grad(set_to_none=False)
        out = model(x, ei)
        torch.nn.functional.cross_entropy(out[a], ya).backward()
        return out

    step()
    torch.cuda.synchronize()
    want = [p.grad.clone() for p in model.parameters()]
    import pytorch_geometric_amd as pga
    n = x.size(0)
    assert pga.as_edge_index(ei, n, n).by_src()._live is not None   # the eager step used them
    replay = CapturedStep(step, warmup=1)
    torch.cuda.synchronize()
    builds = _native.live_lists_builds()
    replay()
    replay()
    torch.cuda.synchronize()
    assert _native.live_lists_builds() == builds   # nothing of the lists is in the graph
    for p, w in zip(model.parameters(), want):
        assert torch.equal(p.grad, w)
