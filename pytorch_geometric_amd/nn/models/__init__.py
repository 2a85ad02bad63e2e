from .basic_gnn import GAT, GCN, BasicGNN, GraphSAGE
from .deepgcn import DeepGCNLayer

__all__ = ['BasicGNN', 'GCN', 'GraphSAGE', 'GAT', 'DeepGCNLayer']
