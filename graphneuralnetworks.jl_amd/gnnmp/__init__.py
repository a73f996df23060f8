"""gnnmp — MI355X-native message-passing engine behind the GNNlib.jl / GNNGraphs.jl API for the
propagate / apply_edges / aggregate_neighbors hot path (include/gnnmp.h).

Host side only: every arithmetic step is a call into libgnnmp.so (hand-written HIP for gfx950).
"""
from ._lib import GnnmpError, Knob, Variant, knob, load, tune, tuned, tuned_bits  # noqa: F401
from . import placement  # noqa: F401
from .graph import (GNNGraph, Plan, add_self_loops, batch, batch_arrays, check_num_edges, check_num_nodes, degree,  # noqa: F401
                    edge_index, get_edge_weight, get_graph_type, graph_indicator, set_edge_weight)
from .layers import (Dense, GATConv, GCNConv, GlobalPool, GNNChain, GraphConv, SAGEConv, bias_act, dense, fused_conv,  # noqa: F401
                     gat_conv, gcn_conv, global_pool, glorot_uniform, graph_conv, sage_conv)
from .msgpass import (aggregate_neighbors, apply_edges, copy_xi, copy_xj, e_mul_xj, propagate, w_mul_xj,  # noqa: F401
                      xi_dot_xj, xi_sub_xj, xj_sub_xi)
from .layers_attn import (AGNNConv, GATv2Conv, GINConv, TransformerConv, agnn_conv, gatv2_conv, gin_conv,  # noqa: F401
                          transformer_conv)
from .layers_khop import (GlobalAttentionPool, ResGatedGraphConv, SGConv, TAGConv, global_attention_pool,  # noqa: F401
                          res_gated_graph_conv, sg_conv, tag_conv)
from .layers_more import (CGConv, ChebConv, DConv, EdgeConv, EGNNConv, GatedGraphConv, GMMConv, MEGNetConv,  # noqa: F401
                          NNConv, Set2Set, cg_conv, cheb_conv, d_conv, edge_conv, egnn_conv, gated_graph_conv, gmm_conv,
                          megnet_conv, nn_conv, set2set_pool)
from .temporal_graph import TemporalSnapshotsGNNGraph, add_snapshot, remove_snapshot  # noqa: F401
from .layers_temporal import (DCGRU, TGCN, DCGRUCell, EvolveGCNO, EvolveGCNOCell, GConvGRU, GConvGRUCell, GConvLSTM,  # noqa: F401
                              GConvLSTMCell, GNNRecurrence, LSTMCell, TGCNCell, poly_hop_ld, tgcn_forward)
from .backward_temporal import tgcn_ad  # noqa: F401
from .backward_recurrent import dcgru_ad, gconv_gru_ad, gconv_lstm_ad  # noqa: F401
from .backward_evolve import evolve_gcno_ad, outer_accum  # noqa: F401
from .linkpred import (DotDecoder, WithGraph, dot_decoder, dot_decoder_ad, edge_dot_ad, edge_dot_grad,  # noqa: F401
                       negative_sample, rand_edge_split)
from .neighbors import knn_graph, radius_graph  # noqa: F401
from .generate import hyperbolic_graph, rand_temporal_hyperbolic_graph, rand_temporal_radius_graph  # noqa: F401
from .transform import (EdgeCoalescing, add_edges, add_nodes, coalesce_edges, has_isolated_nodes, has_multi_edges,  # noqa: F401
                        perturb_edges, ppr_diffusion, random_walk_pe, remove_edges, remove_multi_edges, remove_nodes, remove_self_loops,
                        to_bidirected, to_unidirected)
from .pool_topk import TopKPool, topk_index, topk_pool, topk_pool_ad  # noqa: F401
from .hetero import (GNNHeteroGraph, HeteroGraphConv, edge_type_subgraph, hetero_propagate, num_edge_types,  # noqa: F401
                     num_node_types, rand_bipartite_heterograph, rand_heterograph)
from .backward_hetero import hetero_conv_ad, hetero_propagate_ad, hetero_propagate_grad  # noqa: F401
from .backward_edge import edge_conv_ad  # noqa: F401
from .backward_cg import cg_conv_ad  # noqa: F401
from .backward_nn import nn_conv_ad  # noqa: F401
from .backward_egnn import egnn_conv_ad  # noqa: F401
from .backward_gmm import gmm_conv_ad  # noqa: F401
from .backward_megnet import aggregate_neighbors_ad, megnet_conv_ad  # noqa: F401
from .backward_readout import global_attention_pool_ad, set2set_ad  # noqa: F401
from .backward_poly import cheb_conv_ad, d_conv_ad  # noqa: F401
from .backward_gated import gated_graph_conv_ad, res_gated_graph_conv_ad  # noqa: F401
from .dataset import DataLoader, GraphDataset, concat_plans  # noqa: F401
from .sampling import (NeighborLoader, NodeSet, has_self_loops, induced_subgraph, is_bidirected, sample_neighbors,  # noqa: F401
                       sort_edge_index)
from .utils import (broadcast_edges, broadcast_nodes, expand_srcdst, reduce_edges, reduce_nodes,  # noqa: F401
                    softmax_edge_neighbors, softmax_edges, softmax_nodes)

__version__ = "0.1.0"
