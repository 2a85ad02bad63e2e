"""Generates tests/golden/golden_nonfinite_v1.pt by running the REAL reference (PyG) on CPU on
inputs with -inf masks, +inf, NaN, 1e4- and 3e38-magnitude values, subnormals, signed zeros and
empty segments (layout: tests/_nonfinite_cases.py).  Build container only:

    PYTHONPATH=/root/reference python tests/golden/make_golden_nonfinite.py

Per width H: the input, the same input with the special values replaced by ``randn`` (only the
special column differs: ``clean_col``), and per call the reference's output and its autograd
gradient for a fixed ``grad_out``.  Every call here works column by column, so for H > 3 only the
columns ``cols`` (the special one and its neighbours) of inputs and results are kept;
``_nonfinite_cases.full`` rebuilds a full-width input around them.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.environ.get('PYG_REFERENCE', '/root/reference'))
import torch_geometric  # noqa: E402
import torch_geometric.typing as pyg_typing  # noqa: E402
from torch_geometric.utils import scatter, segment, softmax  # noqa: E402
from torch_geometric.utils._segment import segment_logsumexp  # noqa: E402

from tests import _nonfinite_cases as NF  # noqa: E402

assert not pyg_typing.WITH_TORCH_SCATTER and not pyg_typing.WITH_PYG_LIB \
    and not pyg_typing.WITH_SOFTMAX, "goldens must come from the plain CPU scatter path"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def build_input(H, seed):
    g = gen(seed)
    segs = NF.layout(H)
    kinds = [k for k, _ in segs]
    lens = torch.tensor([n for _, n in segs])
    ptr = torch.zeros(len(segs) + 1, dtype=torch.long)
    ptr[1:] = lens.cumsum(0)
    n, c = int(ptr[-1]), NF.special_col(H)
    cols = NF.kept_cols(H)
    src = NF.full(torch.randn(n, len(cols), generator=g) * 3, H, cols, seed)
    clean_col = src[:, c].clone()
    for i, kind in enumerate(kinds):
        if kind:
            src[ptr[i]:ptr[i + 1], c] = torch.tensor(NF.special_values(kind, H))
    NF.check_layout(H, kinds, ptr)
    index = torch.arange(len(segs)).repeat_interleave(lens)
    perm = torch.randperm(n, generator=g)
    return dict(H=H, col=c, cols=cols, seed=seed, kinds=kinds, ptr=ptr, index=index, perm=perm,
                src=src, clean_col=clean_col, grad_row=torch.randn(n, H, generator=g),
                grad_seg=torch.randn(len(segs), H, generator=g))


def run(fn, src, grad_out):
    x = src.clone().requires_grad_(True)
    out = fn(x)
    (grad, ) = torch.autograd.grad(out, [x], grad_out)
    return out.detach(), grad


G = {'meta': {'torch': torch.__version__, 'pyg': torch_geometric.__version__}}
for H in NF.WIDTHS:
    I = build_input(H, 7000 + H)
    src, ptr, index, perm, S = I['src'], I['ptr'], I['index'], I['perm'], len(I['kinds'])
    g_row, g_seg, cols = I['grad_row'], I['grad_seg'], I['cols']
    src_u, index_u, g_u = src[perm], index[perm], g_row[perm]
    R = {}

    def keep(name, out, grad):  # [rows, H] results, reduced to the kept columns
        R[name] = {'out': out[:, cols].clone(), 'grad': grad[:, cols].clone()}

    keep('softmax_ptr', *run(lambda s: softmax(s, None, ptr), src, g_row))
    keep('softmax_index', *run(lambda s: softmax(s, index, num_nodes=S), src, g_row))
    keep('softmax_shuffled', *run(lambda s: softmax(s, index_u, num_nodes=S), src_u, g_u))
    out, grad = run(lambda s: softmax(s, index, num_nodes=S, dim=-1), src.t().contiguous(),
                    g_row.t().contiguous())
    keep('softmax_dim1', out.t(), grad.t())
    keep('lse_dim0', *run(lambda s: segment_logsumexp(s, ptr, 0), src, g_seg))
    out, grad = run(lambda s: segment_logsumexp(s, ptr, 1), src.t().contiguous(),
                    g_seg.t().contiguous())
    R['lse_dim1'] = {'out': out.t()[:, cols].clone(), 'grad': grad.t()[:, cols].clone()}
    for r in ('sum', 'mean', 'min', 'max'):
        keep(f'segment_{r}', *run(lambda s: segment(s, ptr, r), src, g_seg))
    for r in ('sum', 'mean', 'min', 'max', 'mul'):
        keep(f'scatter_{r}', *run(lambda s: scatter(s, index_u, 0, S, r), src_u, g_seg))
    for k in ('src', 'grad_row', 'grad_seg'):
        I[k] = I[k][:, cols].clone()
    I['results'] = R
    G[f'H{H}'] = I

out = os.path.join(HERE, 'golden_nonfinite_v1.pt')
torch.save(G, out)
print('wrote', out, os.path.getsize(out), 'bytes')
