"""SplineConv restated in plain float64 torch from the definition (the reference's operators are
pyg-lib's and not importable): basis, weighting, layer.  ``v = pseudo * span`` is taken in
float32, as the definition says, so that bins agree with the kernels at the knots."""
import torch


def _poly(f, degree, k):
    if degree == 1:
        return (1 - f, f)[k]
    if degree == 2:
        return (0.5 * f * f - f + 0.5, -f * f + f + 0.5, 0.5 * f * f)[k]
    return ((1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f * f + 4) / 6,
            (-3 * f ** 3 + 3 * f * f + 3 * f + 1) / 6, f ** 3 / 6)[k]


def basis(pseudo, kernel_size, is_open_spline, degree):
    """``(basis [E, S] float64, weight_index [E, S] int64)``; differentiable by ``pseudo``"""
    E, dim = pseudo.shape
    S = (degree + 1) ** dim
    span = [float(kernel_size[d] - degree * int(bool(is_open_spline[d]))) for d in range(dim)]
    cols_b, cols_w = [], []
    for s in range(S):
        b = torch.ones(E, dtype=torch.float64, device=pseudo.device)
        wi = torch.zeros(E, dtype=torch.int64, device=pseudo.device)
        offset, digits = 1, s
        for d in range(dim):
            k, digits = digits % (degree + 1), digits // (degree + 1)
            v32 = pseudo[:, d].detach().float() * span[d]
            whole = v32.long()
            v = pseudo[:, d].double() * span[d]
            f = v - v32.floor().double()       # (the float32 floor: the same bin as `whole`)
            b = b * _poly(f, degree, k)
            wi = wi + ((whole + k) % int(kernel_size[d])) * offset
            offset *= int(kernel_size[d])
        cols_b.append(b)
        cols_w.append(wi)
    return torch.stack(cols_b, 1), torch.stack(cols_w, 1)


def weighting(x_j, weight, b, wi):
    """``out[e] = sum_s b[e, s] * x_j[e] @ weight[wi[e, s]]``"""
    out = 0
    for s in range(b.size(1)):
        out = out + b[:, s:s + 1] * torch.einsum('ef,efm->em', x_j, weight[wi[:, s]])
    return out


def layer(weight, lin_weight, bias, x_src, x_dst, pseudo, ei, n_dst, kernel_size, is_open_spline,
          degree, aggr):
    """the layer's output in the dtype of its (float64) arguments; ``lin_weight`` / ``bias`` None:
    without that term"""
    b, wi = basis(pseudo, kernel_size, is_open_spline, degree)
    msg = weighting(x_src[ei[0]], weight, b.to(x_src.dtype), wi)
    idx = ei[1].view(-1, 1).expand_as(msg)
    out = msg.new_zeros(n_dst, msg.size(1))
    if aggr == 'max':
        out = out.scatter_reduce(0, idx, msg, 'amax', include_self=False)
    else:
        out = out.scatter_add(0, idx, msg)
        if aggr == 'mean':
            out = out / torch.bincount(ei[1], minlength=n_dst).clamp(min=1).view(-1, 1)
    if lin_weight is not None:
        out = out + x_dst[:n_dst] @ lin_weight.t()
    return out if bias is None else out + bias
