from typing import Callable, Optional, Tuple, Union

import torch
from torch import Tensor

from ..inits import reset
from .message_passing import MessagePassing


class EdgeConv(MessagePassing):
    r"""The edge convolution of "Dynamic Graph CNN for Learning on Point Clouds"
    (torch_geometric/nn/conv/edge_conv.py:13-64):

    .. math::
        \mathbf{x}^{\prime}_i = \mathrm{aggr}_{j \in \mathcal{N}(i)}
        h_{\mathbf{\Theta}}(\mathbf{x}_i \, \Vert \, \mathbf{x}_j - \mathbf{x}_i)

    with ``nn`` = :math:`h_{\mathbf{\Theta}}` mapping ``[-1, 2 * in_channels]`` to
    ``[-1, out_channels]`` and ``aggr`` one of ``"add"``, ``"mean"``, ``"max"``.  The layer runs on
    the gather -> ``message`` -> aggregate route of :class:`MessagePassing`; its state dict is the
    reference's (``nn.*``)."""

    def __init__(self, nn: Callable, aggr: str = 'max', **kwargs):
        super().__init__(aggr=aggr, **kwargs)
        self.nn = nn
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        reset(self.nn)

    def forward(self, x: Union[Tensor, Tuple[Tensor, Tensor]], edge_index) -> Tensor:
        if isinstance(x, Tensor):
            x = (x, x)
        return self.propagate(edge_index, x=x)

    def message(self, x_i: Tensor, x_j: Tensor) -> Tensor:
        return self.nn(torch.cat([x_i, x_j - x_i], dim=-1))

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}(nn={self.nn})'


class DynamicEdgeConv(MessagePassing):
    r""":class:`EdgeConv` on the graph of the ``k`` nearest neighbours in FEATURE space, rebuilt in
    every forward (torch_geometric/nn/conv/edge_conv.py:67-148; the reference needs pyg-lib's
    ``knn`` operator and raises ``ImportError`` without it).  ``x`` is a tensor or a pair
    ``(x_source, x_target)``, ``batch`` a vector or a pair; the search is
    :func:`pytorch_geometric_amd.nn.knn` of the targets among the sources, which includes the point
    itself.  Static-graph (3-D) input raises ``ValueError``.  ``num_workers`` is accepted and
    ignored."""

    def __init__(self, nn: Callable, k: int, aggr: str = 'max', num_workers: int = 1, **kwargs):
        super().__init__(aggr=aggr, flow='source_to_target', **kwargs)
        self.nn = nn
        self.k = k
        self.num_workers = num_workers
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.nn)

    def forward(self, x: Union[Tensor, Tuple[Tensor, Tensor]],
                batch: Union[Optional[Tensor], Tuple[Optional[Tensor], Optional[Tensor]]] = None
                ) -> Tensor:
        from ..pool.cluster import knn
        if isinstance(x, Tensor):
            x = (x, x)
        if x[0].dim() != 2:
            raise ValueError("Static graphs not supported in DynamicEdgeConv")
        b = (None, None)
        if isinstance(batch, Tensor):
            b = (batch, batch)
        elif isinstance(batch, tuple):
            b = (batch[0], batch[1])
        with torch.no_grad():
            edge_index = knn(x[0], x[1], self.k, b[0], b[1]).flip([0])
        return self.propagate(edge_index, x=x)

    def message(self, x_i: Tensor, x_j: Tensor) -> Tensor:
        return self.nn(torch.cat([x_i, x_j - x_i], dim=-1))

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}(nn={self.nn}, k={self.k})'
