from .base import Connect, ConnectOutput
from .filter_edges import FilterEdges, filter_adj

__all__ = ['Connect', 'ConnectOutput', 'FilterEdges', 'filter_adj']
