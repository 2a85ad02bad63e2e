from .basic_gnn import GAT, GCN, BasicGNN, GraphSAGE
from .deepgcn import DeepGCNLayer
from .graph_unet import GraphUNet

__all__ = ['BasicGNN', 'GCN', 'GraphSAGE', 'GAT', 'DeepGCNLayer', 'GraphUNet']
