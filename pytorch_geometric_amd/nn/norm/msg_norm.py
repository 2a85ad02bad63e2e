import torch
import torch.nn.functional as F
from torch import Tensor


class MessageNorm(torch.nn.Module):
    r"""Message normalisation of DeeperGCN with the constructor arguments, the state-dict key
    (``scale``) and the ``__repr__`` of ``torch_geometric.nn.norm.MessageNorm``
    (torch_geometric/nn/norm/msg_norm.py:9-53):

    .. math:: s \cdot \|x_i\|_p \cdot \frac{m_i}{\|m_i\|_p}

    ``scale`` is always a parameter; it takes a gradient only with ``learn_scale``.  Pure torch."""

    def __init__(self, learn_scale: bool = False, device=None):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.empty(1, device=device), requires_grad=learn_scale)
        self.reset_parameters()

    def reset_parameters(self):
        self.scale.data.fill_(1.0)

    def forward(self, x: Tensor, msg: Tensor, p: float = 2.0) -> Tensor:
        unit = F.normalize(msg, p=p, dim=-1)
        return unit * x.norm(p=p, dim=-1, keepdim=True) * self.scale

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}(learn_scale={self.scale.requires_grad})'
