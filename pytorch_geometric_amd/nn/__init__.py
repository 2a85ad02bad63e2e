from .aggr import (Aggregation, DegreeScalerAggregation, FusedAggregation, MaxAggregation, MeanAggregation,
                   MinAggregation, MulAggregation, MultiAggregation, PowerMeanAggregation,
                   SoftmaxAggregation, StdAggregation, SumAggregation, VarAggregation)
from .conv import (CGConv, FastRGCNConv, FiLMConv, GINConv, GINEConv, GATConv, GATv2Conv, GCNConv, GraphConv, HANConv, HeteroConv, HGTConv,
                   GENConv, GMMConv, MessagePassing, NNConv, PNAConv, ResGatedGraphConv, RGATConv, RGCNConv, SAGEConv, TransformerConv,
                   gcn_norm, group)
from .conv import APPNP, GCN2Conv, LGConv, SGConv, SSGConv, TAGConv
from .conv import DynamicEdgeConv, EdgeConv, PointConv, PointNetConv
from .dense import HeteroDictLinear, HeteroLinear, Linear
from .models import GAT, GCN, BasicGNN, DeepGCNLayer, GraphSAGE
from .norm import BatchNorm, GraphNorm, LayerNorm, MessageNorm
from .pool import global_add_pool, global_max_pool, global_mean_pool
from .pool import fps, knn, knn_graph, nearest, radius, radius_graph
from .pool import SAGPooling, TopKPooling, filter_adj, topk
from . import functional  # noqa: F401

__all__ = [
    'Aggregation', 'SumAggregation', 'MeanAggregation', 'MaxAggregation', 'MinAggregation',
    'MulAggregation', 'VarAggregation', 'StdAggregation', 'FusedAggregation',
    'MultiAggregation', 'SoftmaxAggregation', 'PowerMeanAggregation', 'MessagePassing', 'SAGEConv', 'GCNConv', 'gcn_norm', 'GATConv', 'GATv2Conv', 'TransformerConv', 'RGCNConv', 'FastRGCNConv', 'GraphConv', 'Linear', 'HeteroLinear',
    'HeteroDictLinear', 'HeteroConv', 'group', 'HGTConv', 'GINConv', 'GINEConv',
    'PNAConv', 'DegreeScalerAggregation', 'GENConv', 'MessageNorm', 'DeepGCNLayer',
    'ResGatedGraphConv', 'HANConv', 'GMMConv', 'NNConv', 'CGConv', 'FiLMConv', 'RGATConv',
    'BasicGNN', 'GCN', 'GraphSAGE', 'GAT', 'GraphNorm', 'LayerNorm', 'BatchNorm',
    'global_add_pool', 'global_mean_pool', 'global_max_pool',
    'APPNP', 'SGConv', 'SSGConv', 'TAGConv', 'LGConv', 'GCN2Conv',
    'EdgeConv', 'DynamicEdgeConv', 'PointNetConv', 'PointConv',
    'fps', 'knn', 'knn_graph', 'radius', 'radius_graph', 'nearest',
    'TopKPooling', 'SAGPooling', 'topk', 'filter_adj',
]
