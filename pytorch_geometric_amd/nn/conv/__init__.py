from .message_passing import MessagePassing
from .sage_conv import SAGEConv
from .gcn_conv import GCNConv, gcn_norm
from .gat_conv import GATConv
from .gatv2_conv import GATv2Conv
from .transformer_conv import TransformerConv
from .rgcn_conv import FastRGCNConv, RGCNConv
from .graph_conv import GraphConv
from .hetero_conv import HeteroConv, group
from .hgt_conv import HGTConv
from .han_conv import HANConv
from .gin_conv import GINConv, GINEConv
from .pna_conv import PNAConv
from .gen_conv import GENConv
from .res_gated_graph_conv import ResGatedGraphConv
from .gmm_conv import GMMConv
from .nn_conv import NNConv
from .cg_conv import CGConv
from .film_conv import FiLMConv
from .rgat_conv import RGATConv
from .appnp import APPNP
from .sg_conv import SGConv
from .ssg_conv import SSGConv
from .tag_conv import TAGConv
from .lg_conv import LGConv
from .gcn2_conv import GCN2Conv
from .edge_conv import DynamicEdgeConv, EdgeConv
from .point_conv import PointConv, PointNetConv

__all__ = ['MessagePassing', 'SAGEConv', 'GCNConv', 'gcn_norm', 'GATConv', 'GATv2Conv', 'TransformerConv', 'RGCNConv', 'FastRGCNConv',
           'GraphConv', 'HeteroConv', 'group', 'HGTConv', 'GINConv', 'GINEConv',
           'PNAConv', 'GENConv', 'ResGatedGraphConv', 'HANConv', 'GMMConv', 'NNConv', 'CGConv',
           'FiLMConv', 'RGATConv', 'APPNP', 'SGConv', 'SSGConv', 'TAGConv', 'LGConv', 'GCN2Conv',
           'EdgeConv', 'DynamicEdgeConv', 'PointNetConv', 'PointConv']
