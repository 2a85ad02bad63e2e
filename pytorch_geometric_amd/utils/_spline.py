"""``spline_basis`` and ``spline_weighting`` with the arguments of ``pyg_lib.ops`` as
``torch_geometric/nn/conv/spline_conv.py:150-153`` calls them.  They back SplineConv's generic
route; the fused route (csrc/spline.hip) forms neither of their tensors."""
from typing import Tuple

import torch
from torch import Tensor

# floats of one chunk's [edges, K * F_in] plane in spline_weighting
_CHUNK_FLOATS = 1 << 24


def _polynomials(f: Tensor, degree: int) -> Tensor:
    """``B_degree(f, k)`` for every ``k``: ``[..., degree + 1]``"""
    if degree == 1:
        polys = [1 - f, f]
    elif degree == 2:
        polys = [0.5 * f * f - f + 0.5, -f * f + f + 0.5, 0.5 * f * f]
    elif degree == 3:
        polys = [(1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f * f + 4) / 6,
                 (-3 * f ** 3 + 3 * f * f + 3 * f + 1) / 6, f ** 3 / 6]
    else:
        raise ValueError(f"'degree' must be 1, 2 or 3 (got {degree})")
    return torch.stack(polys, dim=-1)


def _basis_torch(pseudo: Tensor, kernel_size: Tensor, is_open_spline: Tensor,
                 degree: int) -> Tuple[Tensor, Tensor]:
    """The definition as tensor code (differentiable by ``pseudo``): ``v`` in the dtype of
    ``pseudo``, every index wrapped into its dimension non-negatively, NaN to offset 0."""
    E, dim = pseudo.shape
    dev = pseudo.device
    ks = kernel_size.to(dev, torch.int64)
    span = (ks - degree * is_open_spline.to(dev, torch.int64)).to(pseudo.dtype)
    v = pseudo * span
    polys = _polynomials(v - v.floor(), degree)                       # [E, dim, degree + 1]
    s = torch.arange((degree + 1) ** dim, device=dev)
    powers = (degree + 1) ** torch.arange(dim, device=dev)
    digits = (s.view(-1, 1) // powers) % (degree + 1)                 # [S, dim]
    basis = polys[:, torch.arange(dim, device=dev), digits].prod(-1)  # [E, S]
    whole = torch.where(v.detach().abs() < 9.0e18, v.detach(), torch.zeros_like(v)).long()
    idx = torch.remainder(whole.view(E, 1, dim) + digits, ks)
    offset = torch.cumprod(torch.cat([ks.new_ones(1), ks[:-1]]), 0)
    return basis, (idx * offset).sum(-1)


def spline_basis(pseudo: Tensor, kernel_size: Tensor, is_open_spline: Tensor,
                 degree: int) -> Tuple[Tensor, Tensor]:
    r"""``(basis [E, S], weight_index [E, S])`` with ``S = (degree + 1)^dim``: for entry ``s`` with
    digits ``k_d`` in base ``degree + 1``, ``v_d = pseudo_d (kernel_size_d - degree open_d)``,
    ``basis = \prod_d B_degree(v_d - floor(v_d), k_d)`` and ``weight_index = \sum_d ((int(v_d) +
    k_d) mod kernel_size_d) \prod_{d' < d} kernel_size_{d'}``.  float32 device ``pseudo`` that
    takes no gradient: one kernel launch; everything else (host tensors, other dtypes, a gradient
    by ``pseudo``): the same definition as tensor code."""
    if pseudo.dim() != 2:
        raise ValueError("'pseudo' must be two-dimensional")
    fast = (pseudo.is_cuda and pseudo.dtype == torch.float32
            and not (torch.is_grad_enabled() and pseudo.requires_grad)
            and (degree + 1) ** pseudo.size(1) <= 64)
    if fast:
        from .. import _native
        dev = pseudo.device
        return _native.spline_basis(pseudo, kernel_size.to(dev), is_open_spline.to(dev), degree)
    return _basis_torch(pseudo, kernel_size, is_open_spline, degree)


def spline_weighting(x: Tensor, weight: Tensor, basis: Tensor, weight_index: Tensor) -> Tensor:
    """``out[e] = sum_s basis[e, s] * x[e] @ weight[weight_index[e, s]]`` with ``x [E, F_in]`` and
    ``weight [K, F_in, F_out]``, in chunks of edges: a chunk scatters its basis values into dense
    coefficients ``[c, K]`` and takes ONE product ``(coef (x) x) [c, K * F_in] @ weight``, so no
    ``[E, S, F_in, F_out]`` tensor is formed."""
    (E, S), (K, F, M) = basis.shape, weight.shape
    flat = weight.reshape(K * F, M)
    step = max(1, _CHUNK_FLOATS // (K * F))
    outs = []
    for a in range(0, E, step):
        b, wi, xs = basis[a:a + step], weight_index[a:a + step], x[a:a + step]
        coef = torch.zeros(b.size(0), K, dtype=b.dtype, device=b.device).scatter_add(1, wi, b)
        outs.append((coef.unsqueeze(2) * xs.unsqueeze(1)).reshape(-1, K * F) @ flat)
    return torch.cat(outs) if outs else x.new_zeros(0, M)
