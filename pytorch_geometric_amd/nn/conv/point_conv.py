from typing import Callable, Optional, Tuple, Union

import torch
from torch import Tensor

from ...utils.loop import add_self_loops, remove_self_loops
from ..inits import reset
from .message_passing import MessagePassing


class PointNetConv(MessagePassing):
    r"""The PointNet set layer of PointNet / PointNet++
    (torch_geometric/nn/conv/point_conv.py:19-121):

    .. math::
        \mathbf{x}^{\prime}_i = \gamma_{\mathbf{\Theta}} \left( \max_{j \in
        \mathcal{N}(i) \cup \{ i \}} h_{\mathbf{\Theta}} ( \mathbf{x}_j,
        \mathbf{p}_j - \mathbf{p}_i) \right)

    ``local_nn`` = :math:`h_{\mathbf{\Theta}}` maps ``[-1, in_channels + num_dimensions]`` rows,
    ``global_nn`` = :math:`\gamma_{\mathbf{\Theta}}` the aggregated ones; either may be ``None``.
    ``x`` is a tensor, ``None`` or a pair, ``pos`` a tensor or a pair ``(pos_source, pos_target)``.
    With ``add_self_loops`` the self loops of a plain ``edge_index`` are removed and one is added for
    each of the first ``min(N_source, N_target)`` nodes.  The layer runs on the gather ->
    ``message`` -> aggregate route of :class:`MessagePassing`; its state dict is the reference's
    (``local_nn.*``, ``global_nn.*``)."""

    def __init__(self, local_nn: Optional[Callable] = None, global_nn: Optional[Callable] = None,
                 add_self_loops: bool = True, **kwargs):
        kwargs.setdefault('aggr', 'max')
        super().__init__(**kwargs)
        self.local_nn = local_nn
        self.global_nn = global_nn
        self.add_self_loops = add_self_loops
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        reset(self.local_nn)
        reset(self.global_nn)

    def forward(self, x: Union[Optional[Tensor], Tuple[Optional[Tensor], Optional[Tensor]]],
                pos: Union[Tensor, Tuple[Tensor, Tensor]], edge_index) -> Tensor:
        if not isinstance(x, tuple):
            x = (x, None)
        if isinstance(pos, Tensor):
            pos = (pos, pos)
        if self.add_self_loops and isinstance(edge_index, Tensor):
            edge_index, _ = remove_self_loops(edge_index)
            edge_index, _ = add_self_loops(edge_index,
                                           num_nodes=min(pos[0].size(0), pos[1].size(0)))
        out = self.propagate(edge_index, x=x, pos=pos)
        if self.global_nn is not None:
            out = self.global_nn(out)
        return out

    def message(self, x_j: Optional[Tensor], pos_i: Tensor, pos_j: Tensor) -> Tensor:
        msg = pos_j - pos_i
        if x_j is not None:
            msg = torch.cat([x_j, msg], dim=1)
        if self.local_nn is not None:
            msg = self.local_nn(msg)
        return msg

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}(local_nn={self.local_nn}, '
                f'global_nn={self.global_nn})')


PointConv = PointNetConv
