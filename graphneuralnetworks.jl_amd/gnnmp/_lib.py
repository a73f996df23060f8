"""ctypes binding of libgnnmp.so (include/gnnmp.h) — the same symbols the Julia extension `@ccall`s.

torch is used only as plumbing: it owns device memory and the HIP stream.  Every compute call goes through the
C ABI; there is NO CPU fallback — if the library is missing or no GPU is visible, calls raise.
"""
from __future__ import annotations

import contextlib
import ctypes
import os

from .knobs import Knob, Variant  # noqa: F401

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("GNNMP_LIB") or os.path.join(_PKG, "lib", "libgnnmp.so")   # GNNMP_LIB: another build of the same ABI

OK, EINVAL, EBOUNDS, EALLOC, ELAUNCH, EUNSUPPORTED = 0, -1, -2, -3, -4, -5
SUM, MEAN, MAX, MIN = 0, 1, 2, 3
COPY_XJ, W_MUL_XJ = 0, 1
ACT_IDENTITY, ACT_RELU, ACT_SOFTPLUS, ACT_TANH, ACT_SWISH = 0, 1, 2, 3, 4
LONG_ROW = 512

# every symbol include/gnnmp.h declares (tests check the library exports exactly these)
SYMBOLS = (
    "gnnmp_version", "gnnmp_last_error",
    "gnnmp_plan_create", "gnnmp_plan_from_csc", "gnnmp_plan_destroy", "gnnmp_plan_info", "gnnmp_plan_export", "gnnmp_plan_export64",
    "gnnmp_plan_concat", "gnnmp_plan_select", "gnnmp_plan_release", "gnnmp_plan_status", "gnnmp_plan_edge_index",
    "gnnmp_plan_remove_nodes", "gnnmp_plan_add_edges", "gnnmp_plan_keep_nodes",
    "gnnmp_chain_jobs_pack", "gnnmp_chain_jobs_release", "gnnmp_chain_jobs_export",
    "gnnmp_arena_create", "gnnmp_arena_destroy", "gnnmp_arena_alloc", "gnnmp_arena_reset", "gnnmp_arena_class_of", "gnnmp_arena_info",
    "gnnmp_add_self_loops", "gnnmp_batch_coo",
    "gnnmp_sort_edge_index", "gnnmp_is_bidirected", "gnnmp_has_self_loops", "gnnmp_sample_neighbors",
    "gnnmp_unique_append", "gnnmp_induced_subgraph",
    "gnnmp_gather_f32", "gnnmp_edge_sub_f32", "gnnmp_scatter_f32", "gnnmp_scatter_atomic_f32",
    "gnnmp_propagate_f32", "gnnmp_propagate_emul_f32", "gnnmp_propagate_gated_f32", "gnnmp_propagate_slots_f32", "gnnmp_propagate_slots_act_f32", "gnnmp_plan_slot_gather_f32",
    "gnnmp_degree_f32", "gnnmp_inv_sqrt_f32",
    "gnnmp_edge_softmax_f32", "gnnmp_segment_softmax_f32", "gnnmp_gat_node_scores_f32", "gnnmp_gat_aggregate_f32", "gnnmp_gat_conv_f32",
    "gnnmp_gat_conv_edge_f32", "gnnmp_gat_conv_stats_f32", "gnnmp_gat_conv_grad_f32", "gnnmp_attn_conv_f32",
    "gnnmp_gat_conv_train_f32", "gnnmp_gat_conv_grad2_f32",
    "gnnmp_gat_conv_drop_f32", "gnnmp_dropout_keep_u8", "gnnmp_gat_conv_grad_drop_f32", "gnnmp_attn_conv_drop_f32", "gnnmp_attn_conv_grad_drop_f32",
    "gnnmp_attn_conv_grad_f32",
    "gnnmp_bias_act_f32",
    "gnnmp_segment_pool_f32", "gnnmp_segment_bounds", "gnnmp_segment_pool_ptr_f32", "gnnmp_dense_f32", "gnnmp_fused_conv_f32",
    "gnnmp_graphconv_chain_scratch_floats", "gnnmp_graphconv_chain_f32", "gnnmp_chain_jobs_create", "gnnmp_chain_jobs_destroy",
    "gnnmp_chain_jobs_info", "gnnmp_shard_by_size", "gnnmp_allgather_f32",
    "gnnmp_edge_dot_f32", "gnnmp_edge_dot_plan_f32", "gnnmp_propagate_maxmin_grad_f32",
    "gnnmp_head_mean_f32", "gnnmp_head_mean_grad_f32", "gnnmp_add_f32", "gnnmp_axpy_f32", "gnnmp_mul_rows_f32", "gnnmp_is_sorted",
    "gnnmp_act_grad_f32", "gnnmp_dense_grad_workspace", "gnnmp_dense_grad_w_f32",
    "gnnmp_dense_grad_w2_workspace", "gnnmp_dense_grad_w2_f32", "gnnmp_pool_grad_act_f32", "gnnmp_propagate_add_mask_f32",
    "gnnmp_row_normalize_f32", "gnnmp_row_normalize_grad_f32", "gnnmp_propagate_cg_f32", "gnnmp_gru_pointwise_f32", "gnnmp_propagate_nn_f32", "gnnmp_gmm_weights_f32", "gnnmp_row_sqnorm_normalize_f32", "gnnmp_lstm_pointwise_f32", "gnnmp_rowdot_f32",
    "gnnmp_plan_reset_counters",
    "gnnmp_propagate_f64", "gnnmp_gather_f64", "gnnmp_scatter_f64",
    "gnnmp_tgcn_recurrence_f32", "gnnmp_tgcn_recurrence_grad_f32", "gnnmp_tgcn_step_f32", "gnnmp_tgcn_step_grad_f32",
    "gnnmp_negative_sample", "gnnmp_rand_edge_split", "gnnmp_edge_dot_grad_f32",
    "gnnmp_knn_graph_f32", "gnnmp_radius_graph_f32", "gnnmp_hyperbolic_graph_f32",
    "gnnmp_hetero_propagate_f32", "gnnmp_hetero_propagate_grad_f32", "gnnmp_hetero_attn_f32",
    "gnnmp_coalesce_edges", "gnnmp_compact_edges", "gnnmp_has_multi_edges", "gnnmp_has_isolated_nodes",
    "gnnmp_random_walk_pe_f32", "gnnmp_ppr_diffusion_f32",
    "gnnmp_edge_conv_f32", "gnnmp_edge_conv_grad_f32", "gnnmp_cg_conv_grad_f32", "gnnmp_nn_conv_grad_f32",
    "gnnmp_egnn_edge_f32", "gnnmp_egnn_coord_f32", "gnnmp_egnn_coord_grad_f32", "gnnmp_act_grad_z_f32",
    "gnnmp_gmm_conv_f32", "gnnmp_gmm_conv_grad_f32", "gnnmp_gmm_weights_grad_f32",
    "gnnmp_megnet_edge_f32", "gnnmp_megnet_edge_grad_f32", "gnnmp_aggregate_grad_f32",
    "gnnmp_segment_attn_pool_f32", "gnnmp_segment_attn_pool_grad_f32", "gnnmp_lstm_pointwise_grad_f32",
    "gnnmp_poly_hop_f32", "gnnmp_gru_pointwise_grad_f32",
    "gnnmp_poly_hop_ld_f32", "gnnmp_gru_cell_f32", "gnnmp_gru_cell_grad_f32", "gnnmp_lstm_cell_f32", "gnnmp_lstm_cell_grad_f32",
    "gnnmp_lstm_matvec_cell_f32", "gnnmp_lstm_matvec_grad_workspace", "gnnmp_lstm_matvec_grad_f32", "gnnmp_outer_accum_f32",
    "gnnmp_attn_conv_edge_f32", "gnnmp_attn_conv_edge_grad_f32",
    "gnnmp_topk_score_f32", "gnnmp_topk_select_f32", "gnnmp_topk_gate_f32", "gnnmp_topk_gate_grad_f32",
    "gnnmp_gat_conv_edge_stats_f32", "gnnmp_gat_conv_edge_grad_f32", "gnnmp_gat_edge_fold_f32", "gnnmp_gat_edge_fold_grad_f32",
    # the GNNMP_INTERNAL section of the header: experiment / test hooks, exported but not part of the drop-in surface
    "gnnmp_tune", "gnnmp_tune_get", "gnnmp_debug_mock_device", "gnnmp_debug_device_once", "gnnmp_debug_plan_block", "gnnmp_debug_pool_pick",
    "gnnmp_debug_random_walk_pe_f32", "gnnmp_debug_dense_route",
)


HETERO_MAX_REL = 16                       # include/gnnmp.h: GNNMP_HETERO_MAX_REL


class HeteroRel(ctypes.Structure):
    """gnnmp_hetero_rel_t: one relation of a destination type (plan = NULL: an identity relation)"""
    _fields_ = [("plan", ctypes.c_void_p), ("x", ctypes.c_void_p), ("w", ctypes.c_void_p), ("aggr", ctypes.c_int)]


class HeteroDst(ctypes.Structure):
    """gnnmp_hetero_dst_t: one destination type of a gnnmp_hetero_propagate_f32 call"""
    _fields_ = [("out", ctypes.c_void_p), ("n_dst", ctypes.c_int64), ("combine", ctypes.c_int), ("n_rel", ctypes.c_int),
                ("rels", ctypes.POINTER(HeteroRel))]


class HeteroRelGrad(ctypes.Structure):
    """gnnmp_hetero_rel_grad_t: one relation that leaves a source type (plan_t = NULL: an identity / masked identity term)"""
    _fields_ = [("plan_t", ctypes.c_void_p), ("dy", ctypes.c_void_p), ("w", ctypes.c_void_p), ("sd", ctypes.c_void_p),
                ("y", ctypes.c_void_p), ("out", ctypes.c_void_p)]


class HeteroSrc(ctypes.Structure):
    """gnnmp_hetero_src_t: one source type of a gnnmp_hetero_propagate_grad_f32 call"""
    _fields_ = [("dx", ctypes.c_void_p), ("x", ctypes.c_void_p), ("n_src", ctypes.c_int64), ("n_rel", ctypes.c_int),
                ("rels", ctypes.POINTER(HeteroRelGrad))]


class HeteroAttnRel(ctypes.Structure):
    """gnnmp_hetero_attn_rel_t: one attention relation of a destination type (plan = NULL: an identity relation, row i of K as it is)"""
    _fields_ = [("plan", ctypes.c_void_p), ("mode", ctypes.c_int), ("Q", ctypes.c_void_p), ("K", ctypes.c_void_p), ("a", ctypes.c_void_p),
                ("bias", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("negative_slope", ctypes.c_float), ("act", ctypes.c_int)]


class HeteroAttnDst(ctypes.Structure):
    """gnnmp_hetero_attn_dst_t: one destination type of a gnnmp_hetero_attn_f32 call"""
    _fields_ = [("out", ctypes.c_void_p), ("n_dst", ctypes.c_int64), ("combine", ctypes.c_int), ("n_rel", ctypes.c_int),
                ("rels", ctypes.POINTER(HeteroAttnRel))]


COALESCE_DIRECTED, COALESCE_MIRRORED, COALESCE_UNDIRECTED = 0, 1, 2      # include/gnnmp.h: gnnmp_coalesce_mode
COMPACT_SELF_LOOPS, COMPACT_LIST, COMPACT_RANDOM = 0, 1, 2               # include/gnnmp.h: gnnmp_compact_rule


class CoalesceJob(ctypes.Structure):
    """gnnmp_coalesce_t: one gnnmp_coalesce_edges call (a host record of device pointers)"""
    _fields_ = [("s", ctypes.c_void_p), ("t", ctypes.c_void_p), ("idx_bytes", ctypes.c_int), ("index_base", ctypes.c_int),
                ("n_edges", ctypes.c_int64), ("n_nodes", ctypes.c_int64), ("mode", ctypes.c_int), ("s_out", ctypes.c_void_p),
                ("t_out", ctypes.c_void_p), ("colptr", ctypes.c_void_p), ("rowval", ctypes.c_void_p)]


class CompactJob(ctypes.Structure):
    """gnnmp_compact_t: one gnnmp_compact_edges call"""
    _fields_ = [("s", ctypes.c_void_p), ("t", ctypes.c_void_p), ("w", ctypes.c_void_p), ("idx_bytes", ctypes.c_int),
                ("index_base", ctypes.c_int), ("n_edges", ctypes.c_int64), ("rule", ctypes.c_int), ("remove", ctypes.c_void_p),
                ("n_remove", ctypes.c_int64), ("p", ctypes.c_float), ("seed", ctypes.c_uint64), ("s_out", ctypes.c_void_p),
                ("t_out", ctypes.c_void_p), ("w_out", ctypes.c_void_p), ("eid_out", ctypes.c_void_p)]


RWPE_TILE, RWPE_MAX_WALK = 16, 1024      # include/gnnmp.h: GNNMP_RWPE_TILE, GNNMP_RWPE_MAX_WALK


class RwpeJob(ctypes.Structure):
    """gnnmp_rwpe_t: one gnnmp_random_walk_pe_f32 call"""
    _fields_ = [("w", ctypes.c_void_p), ("graph_ptr", ctypes.c_void_p), ("idx_bytes", ctypes.c_int), ("n_graphs", ctypes.c_int64),
                ("walk_length", ctypes.c_int64), ("out", ctypes.c_void_p)]


PPR_MAX_NODES = 4096                     # include/gnnmp.h: GNNMP_PPR_MAX_NODES


class PprJob(ctypes.Structure):
    """gnnmp_ppr_t: one gnnmp_ppr_diffusion_f32 call"""
    _fields_ = [("w", ctypes.c_void_p), ("graph_ptr", ctypes.c_void_p), ("idx_bytes", ctypes.c_int), ("n_graphs", ctypes.c_int64),
                ("alpha", ctypes.c_float), ("lds_budget_bytes", ctypes.c_int64), ("out", ctypes.c_void_p)]


TOPK_TIES_FIRST, TOPK_TIES_ALL = 0, 1                                    # include/gnnmp.h: GNNMP_TOPK_TIES_*
TOPK_ACT_SIGMOID, TOPK_ACT_TANH, TOPK_ACT_IDENTITY = 0, 1, 2             # include/gnnmp.h: GNNMP_TOPK_ACT_*
TOPK_GRAD_ROWS = 64                                                      # include/gnnmp.h: GNNMP_TOPK_GRAD_ROWS


class TopkJob(ctypes.Structure):
    """gnnmp_topk_t: one gnnmp_topk_select_f32 call"""
    _fields_ = [("score", ctypes.c_void_p), ("graph_ptr", ctypes.c_void_p), ("idx_bytes", ctypes.c_int), ("n_graphs", ctypes.c_int64),
                ("k", ctypes.c_int64), ("ratio", ctypes.c_float), ("ties", ctypes.c_int), ("lds_budget_bytes", ctypes.c_int64),
                ("keep", ctypes.c_void_p), ("rank", ctypes.c_void_p)]


class TopkGateJob(ctypes.Structure):
    """gnnmp_topk_gate_t: one gnnmp_topk_gate_f32 call"""
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("node_map", ctypes.c_void_p), ("act", ctypes.c_int),
                ("out", ctypes.c_void_p)]


class TopkGateGradJob(ctypes.Structure):
    """gnnmp_topk_gate_grad_t: one gnnmp_topk_gate_grad_f32 call (part: ceil(N / TOPK_GRAD_ROWS) * (C + 1) floats when dp is given)"""
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("p", ctypes.c_void_p), ("dout", ctypes.c_void_p),
                ("node_new", ctypes.c_void_p), ("act", ctypes.c_int), ("dx", ctypes.c_void_p), ("dy", ctypes.c_void_p),
                ("dp", ctypes.c_void_p), ("part", ctypes.c_void_p)]


class EdgeConvJob(ctypes.Structure):
    """gnnmp_edge_conv_t: one gnnmp_edge_conv_f32 call (p [N][2C] planar, y [N][C])"""
    _fields_ = [("p", ctypes.c_void_p), ("y", ctypes.c_void_p), ("aggr", ctypes.c_int), ("act", ctypes.c_int)]


class EdgeConvGradJob(ctypes.Structure):
    """gnnmp_edge_conv_grad_t: one gnnmp_edge_conv_grad_f32 call (p, y, dy read; dp [N][2C] written)"""
    _fields_ = [("p", ctypes.c_void_p), ("y", ctypes.c_void_p), ("dy", ctypes.c_void_p), ("dp", ctypes.c_void_p),
                ("aggr", ctypes.c_int), ("act", ctypes.c_int)]


class CGConvGradJob(ctypes.Structure):
    """gnnmp_cg_conv_grad_t: one gnnmp_cg_conv_grad_f32 call (fs_i, fs_j, fs_e | None, dy read; dfs_i, dfs_j, dfs_e | None written)"""
    _fields_ = [("fs_i", ctypes.c_void_p), ("fs_j", ctypes.c_void_p), ("fs_e", ctypes.c_void_p), ("dy", ctypes.c_void_p),
                ("dfs_i", ctypes.c_void_p), ("dfs_j", ctypes.c_void_p), ("dfs_e", ctypes.c_void_p), ("act", ctypes.c_int)]


class NNConvGradJob(ctypes.Structure):
    """gnnmp_nn_conv_grad_t: one gnnmp_nn_conv_grad_f32 call (x, we | None, dm read; dx | None, dwe | None written)"""
    _fields_ = [("x", ctypes.c_void_p), ("we", ctypes.c_void_p), ("dm", ctypes.c_void_p), ("dx", ctypes.c_void_p),
                ("dwe", ctypes.c_void_p)]


class EgnnEdgeJob(ctypes.Structure):
    """gnnmp_egnn_edge_t: one gnnmp_egnn_edge_f32 call (s, t, x, P, Q, F | None, c read; q, a0, z0 | None written)"""
    _fields_ = [("s", ctypes.c_void_p), ("t", ctypes.c_void_p), ("idx_bytes", ctypes.c_int), ("index_base", ctypes.c_int),
                ("x", ctypes.c_void_p), ("P", ctypes.c_void_p), ("Q", ctypes.c_void_p), ("F", ctypes.c_void_p), ("c", ctypes.c_void_p),
                ("q", ctypes.c_void_p), ("a0", ctypes.c_void_p), ("z0", ctypes.c_void_p), ("act", ctypes.c_int)]


class EgnnCoordJob(ctypes.Structure):
    """gnnmp_egnn_coord_t: one gnnmp_egnn_coord_f32 call (x, mx read; xo = x' written)"""
    _fields_ = [("x", ctypes.c_void_p), ("mx", ctypes.c_void_p), ("xo", ctypes.c_void_p)]


class EgnnCoordGradJob(ctypes.Structure):
    """gnnmp_egnn_coord_grad_t: one gnnmp_egnn_coord_grad_f32 call (x, dxo, mx | None, dq | None read; dmx | None, dx | None written)"""
    _fields_ = [("x", ctypes.c_void_p), ("dxo", ctypes.c_void_p), ("mx", ctypes.c_void_p), ("dq", ctypes.c_void_p),
                ("dmx", ctypes.c_void_p), ("dx", ctypes.c_void_p)]


class ActGradZJob(ctypes.Structure):
    """gnnmp_act_grad_z_t: one gnnmp_act_grad_z_f32 call (dy, z | None read; dz written)"""
    _fields_ = [("dy", ctypes.c_void_p), ("z", ctypes.c_void_p), ("dz", ctypes.c_void_p), ("act", ctypes.c_int)]


GMM_PARTS, GMM_MAX_K = 256, 16      # include/gnnmp.h: GNNMP_GMM_PARTS; K = 1 .. 16


class GmmConvJob(ctypes.Structure):
    """gnnmp_gmm_conv_t: one gnnmp_gmm_conv_f32 call (w, xk, bias | None read; y, z | None written)"""
    _fields_ = [("w", ctypes.c_void_p), ("xk", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p), ("z", ctypes.c_void_p),
                ("act", ctypes.c_int)]


class GmmConvGradJob(ctypes.Structure):
    """gnnmp_gmm_conv_grad_t: one gnnmp_gmm_conv_grad_f32 call (w | None, xk | None, dz read; dxk | None, dw | None written)"""
    _fields_ = [("w", ctypes.c_void_p), ("xk", ctypes.c_void_p), ("dz", ctypes.c_void_p), ("dxk", ctypes.c_void_p), ("dw", ctypes.c_void_p)]


class GmmWeightsGradJob(ctypes.Structure):
    """gnnmp_gmm_weights_grad_t: one gnnmp_gmm_weights_grad_f32 call (e, mu, sinv, w, dw read; de | None, dmu, dsinv | None, part written)"""
    _fields_ = [("e", ctypes.c_void_p), ("mu", ctypes.c_void_p), ("sinv", ctypes.c_void_p), ("w", ctypes.c_void_p), ("dw", ctypes.c_void_p),
                ("de", ctypes.c_void_p), ("dmu", ctypes.c_void_p), ("dsinv", ctypes.c_void_p), ("part", ctypes.c_void_p)]


class MegnetEdgeJob(ctypes.Structure):
    """gnnmp_megnet_edge_t: one gnnmp_megnet_edge_f32 call (P, Q, F | None read; a0, z0 | None written)"""
    _fields_ = [("P", ctypes.c_void_p), ("Q", ctypes.c_void_p), ("F", ctypes.c_void_p), ("a0", ctypes.c_void_p), ("z0", ctypes.c_void_p),
                ("act", ctypes.c_int)]


class MegnetEdgeGradJob(ctypes.Structure):
    """gnnmp_megnet_edge_grad_t: one gnnmp_megnet_edge_grad_f32 call (da0, z | None read; dz0 | None, dP and dQ | None written)"""
    _fields_ = [("da0", ctypes.c_void_p), ("z", ctypes.c_void_p), ("dz0", ctypes.c_void_p), ("dP", ctypes.c_void_p), ("dQ", ctypes.c_void_p),
                ("act", ctypes.c_int)]


class AggregateGradJob(ctypes.Structure):
    """gnnmp_aggregate_grad_t: one gnnmp_aggregate_grad_f32 call (dy, m | None, y | None, acc | None read; dm written)"""
    _fields_ = [("dy", ctypes.c_void_p), ("m", ctypes.c_void_p), ("y", ctypes.c_void_p), ("acc", ctypes.c_void_p), ("dm", ctypes.c_void_p)]


READOUT_MAX_D = 4096    # GNNMP_READOUT_MAX_D


class SegmentAttnJob(ctypes.Structure):
    """gnnmp_segment_attn_t: one gnnmp_segment_attn_pool_f32 call (x, seg_ptr, q | gate read; r, stats written)"""
    _fields_ = [("x", ctypes.c_void_p), ("seg_ptr", ctypes.c_void_p), ("q", ctypes.c_void_p), ("gate", ctypes.c_void_p),
                ("r", ctypes.c_void_p), ("stats", ctypes.c_void_p)]


class SegmentAttnGradJob(ctypes.Structure):
    """gnnmp_segment_attn_grad_t: one gnnmp_segment_attn_pool_grad_f32 call (dr, x, seg_ptr, q | gate, r, stats, base | None read;
    dq | None, dx | None, dgate | None written)"""
    _fields_ = [("dr", ctypes.c_void_p), ("x", ctypes.c_void_p), ("seg_ptr", ctypes.c_void_p), ("q", ctypes.c_void_p),
                ("gate", ctypes.c_void_p), ("r", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("base", ctypes.c_void_p),
                ("dq", ctypes.c_void_p), ("dx", ctypes.c_void_p), ("dgate", ctypes.c_void_p)]


class LstmGradJob(ctypes.Structure):
    """gnnmp_lstm_grad_t: one gnnmp_lstm_pointwise_grad_f32 call (gx, gh, b | None, c, dh, dcn | None read; da, dc written)"""
    _fields_ = [("gx", ctypes.c_void_p), ("gh", ctypes.c_void_p), ("b", ctypes.c_void_p), ("c", ctypes.c_void_p), ("dh", ctypes.c_void_p),
                ("dcn", ctypes.c_void_p), ("da", ctypes.c_void_p), ("dc", ctypes.c_void_p)]


class PolyHopJob(ctypes.Structure):
    """gnnmp_poly_hop_t: one gnnmp_poly_hop_f32 call (z, w_slot | None, ss_slot | None, scale_dst | None, self | None, prev | None,
    add | None read; out written; out may be prev or add)"""
    _fields_ = [("z", ctypes.c_void_p), ("w_slot", ctypes.c_void_p), ("ss_slot", ctypes.c_void_p), ("scale_dst", ctypes.c_void_p),
                ("self", ctypes.c_void_p), ("prev", ctypes.c_void_p), ("add", ctypes.c_void_p), ("alpha", ctypes.c_float),
                ("beta", ctypes.c_float), ("gamma", ctypes.c_float), ("out", ctypes.c_void_p)]


class GruGradJob(ctypes.Structure):
    """gnnmp_gru_grad_t: one gnnmp_gru_pointwise_grad_f32 call (gx, gh, b | None, h, dout, base | None read; dgx, dgh, dh written; base
    may be dh)"""
    _fields_ = [("gx", ctypes.c_void_p), ("gh", ctypes.c_void_p), ("b", ctypes.c_void_p), ("h", ctypes.c_void_p), ("dout", ctypes.c_void_p),
                ("base", ctypes.c_void_p), ("dgx", ctypes.c_void_p), ("dgh", ctypes.c_void_p), ("dh", ctypes.c_void_p)]


class PolyHopLdJob(ctypes.Structure):
    """gnnmp_poly_hop_ld_t: one gnnmp_poly_hop_ld_f32 call — PolyHopJob's fields, then a row stride in floats for z, self, prev, add, out"""
    _fields_ = PolyHopJob._fields_ + [("ld_z", ctypes.c_int64), ("ld_self", ctypes.c_int64), ("ld_prev", ctypes.c_int64),
                                      ("ld_add", ctypes.c_int64), ("ld_out", ctypes.c_int64)]


class GruCellJob(ctypes.Structure):
    """gnnmp_gru_cell_t: one gnnmp_gru_cell_f32 call (P, a, h | None read; gates, hout (| None in phase 1), y written)"""
    _fields_ = [("P", ctypes.c_void_p), ("a", ctypes.c_void_p), ("h", ctypes.c_void_p), ("ldh", ctypes.c_int64), ("gates", ctypes.c_void_p),
                ("hout", ctypes.c_void_p), ("ldhout", ctypes.c_int64), ("rep", ctypes.c_int), ("y", ctypes.c_void_p)]


class GruCellGradJob(ctypes.Structure):
    """gnnmp_gru_cell_grad_t: one gnnmp_gru_cell_grad_f32 call (dy, carry | None, carry2 | None, gates, h | None, drh read; dP, dac, darz,
    part written)"""
    _fields_ = [("dy", ctypes.c_void_p), ("carry", ctypes.c_void_p), ("carry2", ctypes.c_void_p), ("ldc2", ctypes.c_int64),
                ("gates", ctypes.c_void_p), ("h", ctypes.c_void_p), ("ldh", ctypes.c_int64), ("drh", ctypes.c_void_p),
                ("lddrh", ctypes.c_int64), ("rep", ctypes.c_int), ("dP", ctypes.c_void_p), ("dac", ctypes.c_void_p),
                ("darz", ctypes.c_void_p), ("part", ctypes.c_void_p)]


class LstmCellJob(ctypes.Structure):
    """gnnmp_lstm_cell_t: one gnnmp_lstm_cell_f32 call (P, a, w, c | None read; gates, cnew, hout | None, y written)"""
    _fields_ = [("P", ctypes.c_void_p), ("a", ctypes.c_void_p), ("w", ctypes.c_void_p), ("c", ctypes.c_void_p), ("ldc", ctypes.c_int64),
                ("gates", ctypes.c_void_p), ("cnew", ctypes.c_void_p), ("hout", ctypes.c_void_p), ("ldhout", ctypes.c_int64),
                ("y", ctypes.c_void_p)]


class LstmCellGradJob(ctypes.Structure):
    """gnnmp_lstm_cell_grad_t: one gnnmp_lstm_cell_grad_f32 call (dy, carry_h | None, carry_c | None, gates, w, c | None, cnew read; dP, da,
    dc, peep | None written)"""
    _fields_ = [("dy", ctypes.c_void_p), ("carry_h", ctypes.c_void_p), ("ldch", ctypes.c_int64), ("carry_c", ctypes.c_void_p),
                ("gates", ctypes.c_void_p), ("w", ctypes.c_void_p), ("c", ctypes.c_void_p), ("ldc", ctypes.c_int64),
                ("cnew", ctypes.c_void_p), ("dP", ctypes.c_void_p), ("da", ctypes.c_void_p), ("dc", ctypes.c_void_p),
                ("peep", ctypes.c_void_p)]


class LstmMatvecJob(ctypes.Structure):
    """gnnmp_lstm_matvec_t: one gnnmp_lstm_matvec_cell_f32 call (Wi, Wh, x, h | None, c | None, b | None read; h_out, c_out, a_out | None
    written)"""
    _fields_ = [("Wi", ctypes.c_void_p), ("Wh", ctypes.c_void_p), ("x", ctypes.c_void_p), ("h", ctypes.c_void_p), ("c", ctypes.c_void_p),
                ("b", ctypes.c_void_p), ("h_out", ctypes.c_void_p), ("c_out", ctypes.c_void_p), ("a_out", ctypes.c_void_p)]


class LstmMatvecGradJob(ctypes.Structure):
    """gnnmp_lstm_matvec_grad_t: one gnnmp_lstm_matvec_grad_f32 call (Wi, Wh, da, add_x | None, add_h | None read; out_x | None,
    out_h | None written; ws the scratch of gnnmp_lstm_matvec_grad_workspace(D) floats)"""
    _fields_ = [("Wi", ctypes.c_void_p), ("Wh", ctypes.c_void_p), ("da", ctypes.c_void_p), ("add_x", ctypes.c_void_p),
                ("add_h", ctypes.c_void_p), ("out_x", ctypes.c_void_p), ("out_h", ctypes.c_void_p), ("sum", ctypes.c_int),
                ("ws", ctypes.c_void_p), ("ws_floats", ctypes.c_int64)]


class OuterAccumJob(ctypes.Structure):
    """gnnmp_outer_accum_t: one gnnmp_outer_accum_f32 call (A [T][R], B [T][K] read; dW [R][K], db [R] | None written)"""
    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("dW", ctypes.c_void_p), ("db", ctypes.c_void_p)]


class AttnEdgeJob(ctypes.Structure):
    """gnnmp_attn_edge_t: one gnnmp_attn_conv_edge_f32 call (Q | None, K, V | None, F [E][H C], a, bias | None read; out, stats | None
    written)"""
    _fields_ = [("Q", ctypes.c_void_p), ("K", ctypes.c_void_p), ("V", ctypes.c_void_p), ("F", ctypes.c_void_p), ("a", ctypes.c_void_p),
                ("bias", ctypes.c_void_p), ("out", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("negative_slope", ctypes.c_float),
                ("scale", ctypes.c_float), ("act", ctypes.c_int)]


class AttnEdgeGradJob(ctypes.Structure):
    """gnnmp_attn_edge_grad_t: one gnnmp_attn_conv_edge_grad_f32 call (the forward's inputs, stats, dout read; line scratch; dQ, dK,
    dV (DOT), dF, dA and da | None (GATV2) written)"""
    _fields_ = [("Q", ctypes.c_void_p), ("K", ctypes.c_void_p), ("V", ctypes.c_void_p), ("F", ctypes.c_void_p), ("a", ctypes.c_void_p),
                ("stats", ctypes.c_void_p), ("dout", ctypes.c_void_p), ("line", ctypes.c_void_p), ("dQ", ctypes.c_void_p),
                ("dK", ctypes.c_void_p), ("dV", ctypes.c_void_p), ("dF", ctypes.c_void_p), ("dA", ctypes.c_void_p), ("da", ctypes.c_void_p),
                ("negative_slope", ctypes.c_float), ("scale", ctypes.c_float)]


class GatEdgeGradJob(ctypes.Structure):
    """gnnmp_gat_edge_grad_t: one gnnmp_gat_conv_edge_grad_f32 call (Wx_src, Wx_dst | None, a, edge_score, stats, dout read; line scratch;
    dsd, dss, dWx_src, dWx_dst (bipartite), da | None and dscore written)"""
    _fields_ = [("Wx_src", ctypes.c_void_p), ("Wx_dst", ctypes.c_void_p), ("a", ctypes.c_void_p), ("edge_score", ctypes.c_void_p),
                ("stats", ctypes.c_void_p), ("dout", ctypes.c_void_p), ("line", ctypes.c_void_p), ("dsd", ctypes.c_void_p),
                ("dss", ctypes.c_void_p), ("dWx_src", ctypes.c_void_p), ("dWx_dst", ctypes.c_void_p), ("da", ctypes.c_void_p),
                ("dscore", ctypes.c_void_p), ("negative_slope", ctypes.c_float)]


class GnnmpError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"libgnnmp status {status}: {msg}")
        self.status = status


_lib = None


def load():
    """Load libgnnmp.so; raises (loudly) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  gnnmp has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    u64 = ctypes.c_uint64
    L.gnnmp_version.restype = i
    L.gnnmp_last_error.restype = ctypes.c_char_p
    sig = {
        "gnnmp_plan_create": [ctypes.POINTER(vp), vp, vp, i, i, i64, i64, i64, i, i, vp],
        "gnnmp_plan_from_csc": [ctypes.POINTER(vp), vp, vp, i, i, i64, i64, i64, i, vp],
        "gnnmp_plan_destroy": [vp],
        "gnnmp_plan_info": [vp, ctypes.POINTER(i64)],
        "gnnmp_plan_export": [vp, vp, vp, vp, vp],
        "gnnmp_plan_export64": [vp, vp, vp, vp, vp],
        "gnnmp_plan_concat": [ctypes.POINTER(vp), ctypes.POINTER(vp), i64, vp, vp, i, i, vp],
        "gnnmp_plan_select": [ctypes.POINTER(vp), vp, vp, i64, vp, i, i, i64, i64, i64, vp, vp, vp, vp],
        "gnnmp_plan_release": [vp, vp],
        "gnnmp_plan_status": [vp, vp],
        "gnnmp_plan_edge_index": [vp, i, i, vp, vp, vp],
        "gnnmp_plan_remove_nodes": [ctypes.POINTER(vp), vp, vp, i, i, i64, f, u64, vp, vp, vp, ctypes.POINTER(i64), vp],
        "gnnmp_plan_add_edges": [ctypes.POINTER(vp), vp, vp, vp, i, i, i64, i64, u64, vp, vp, vp],
        "gnnmp_chain_jobs_pack": [ctypes.POINTER(vp), vp, i64, i64, i64, i, vp],
        "gnnmp_chain_jobs_release": [vp, vp],
        "gnnmp_chain_jobs_export": [vp, vp, i64, vp, vp],
        "gnnmp_arena_create": [ctypes.POINTER(vp), i64, i, i64, vp],
        "gnnmp_arena_destroy": [vp],
        "gnnmp_arena_alloc": [vp, i, i64, ctypes.POINTER(vp)],
        "gnnmp_arena_reset": [vp],
        "gnnmp_arena_class_of": [vp, vp, i64, ctypes.POINTER(i), vp],
        "gnnmp_arena_info": [vp, ctypes.POINTER(i64)],
        "gnnmp_add_self_loops": [vp, vp, i, i, i64, i64, vp, vp, vp, vp, vp],
        "gnnmp_batch_coo": [vp, vp, i, i, vp, vp, i64, vp, vp, vp, vp],
        "gnnmp_sort_edge_index": [vp, vp, i, i, i64, vp, vp, vp],
        "gnnmp_is_bidirected": [vp, vp, i, i, i64, ctypes.POINTER(i), vp],
        "gnnmp_has_self_loops": [vp, vp, i, i64, ctypes.POINTER(i), vp],
        "gnnmp_sample_neighbors": [vp, vp, i, i, i64, i64, i, ctypes.c_uint64, vp, vp, i64, ctypes.POINTER(i64), vp],
        "gnnmp_unique_append": [vp, vp, i64, vp, i, i, i64, i64, vp, ctypes.POINTER(i64), vp],
        "gnnmp_induced_subgraph": [vp, vp, vp, i, i, i64, vp, vp, vp, vp, i64, ctypes.POINTER(i64), vp],
        "gnnmp_gather_f32": [vp, vp, i, i, i64, vp, i64, vp],
        "gnnmp_edge_sub_f32": [vp, vp, vp, vp, i, i, i64, i, vp, i64, vp],
        "gnnmp_scatter_f32": [vp, i, vp, vp, i64, vp],
        "gnnmp_scatter_atomic_f32": [i, vp, vp, i, i, i64, vp, i64, vp],
        "gnnmp_propagate_f32": [vp, i, i, vp, vp, vp, vp, vp, i64, vp],
        "gnnmp_propagate_emul_f32": [vp, i, vp, vp, vp, i64, vp],
        "gnnmp_propagate_gated_f32": [vp, i, vp, vp, vp, i64, vp],
        "gnnmp_propagate_slots_f32": [vp, i, vp, vp, vp, vp, vp, i64, vp],
        "gnnmp_propagate_slots_act_f32": [vp, i, vp, vp, vp, vp, vp, i, vp, i64, vp],
        "gnnmp_plan_slot_gather_f32": [vp, i, vp, vp, vp],
        "gnnmp_gat_conv_f32": [vp, vp, vp, vp, f, vp, i, vp, i64, i64, vp],
        "gnnmp_gat_conv_edge_f32": [vp, vp, vp, vp, vp, f, vp, i, vp, i64, i64, vp],
        "gnnmp_gat_conv_stats_f32": [vp, vp, vp, vp, f, vp, i, vp, vp, i64, i64, vp],
        "gnnmp_gat_conv_train_f32": [vp, vp, vp, vp, f, vp, i, vp, vp, vp, vp, i64, i64, vp],
        "gnnmp_gat_conv_grad2_f32": [vp, vp, vp, vp, vp, f, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp],
        "gnnmp_attn_conv_f32": [vp, i, vp, vp, vp, vp, f, f, vp, i, vp, vp, i64, i64, vp],
        "gnnmp_attn_conv_grad_f32": [vp, vp, i, vp, vp, vp, vp, f, f, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp],
        "gnnmp_gat_conv_grad_f32": [vp, vp, vp, vp, vp, f, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp],
        "gnnmp_gat_conv_drop_f32": [vp, vp, vp, vp, f, f, u64, vp, i, vp, vp, i64, i64, vp],
        "gnnmp_dropout_keep_u8": [u64, f, i64, i64, vp, vp],
        "gnnmp_attn_conv_drop_f32": [vp, i, vp, vp, vp, vp, f, f, f, u64, vp, i, vp, vp, i64, i64, vp],
        "gnnmp_attn_conv_grad_drop_f32": [vp, vp, i, vp, vp, vp, vp, f, f, f, u64, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp],
        "gnnmp_gat_conv_grad_drop_f32": [vp, vp, vp, vp, vp, f, f, u64, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp],
        "gnnmp_degree_f32": [vp, vp, vp, vp],
        "gnnmp_inv_sqrt_f32": [vp, vp, i64, vp],
        "gnnmp_edge_softmax_f32": [vp, vp, vp, i64, vp],
        "gnnmp_segment_softmax_f32": [vp, vp, vp, i64, f, vp],
        "gnnmp_gat_node_scores_f32": [vp, vp, vp, vp, i64, i64, i64, vp],
        "gnnmp_gat_aggregate_f32": [vp, vp, vp, vp, f, vp, i, vp, vp, i64, i64, vp],
        "gnnmp_bias_act_f32": [vp, vp, i, vp, i64, i64, vp],
        "gnnmp_segment_pool_f32": [i, vp, vp, i, i, vp, i64, i64, i64, vp],
        "gnnmp_segment_bounds": [vp, i, i, i64, i64, vp, vp],
        "gnnmp_segment_pool_ptr_f32": [i, vp, vp, vp, i64, i64, i64, vp],
        "gnnmp_dense_f32": [vp, vp, i64, i64, vp, vp, i64, i64, i, vp, i, vp, i64, i64, vp],
        "gnnmp_fused_conv_f32": [vp, i, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, i, vp, i, vp, i64, vp, vp],
        "gnnmp_edge_dot_f32": [vp, vp, vp, vp, i, i, i64, i64, vp, vp],
        "gnnmp_edge_dot_plan_f32": [vp, vp, vp, vp, i64, vp],
        "gnnmp_head_mean_f32": [vp, vp, i, vp, i64, i64, i64, vp],
        "gnnmp_head_mean_grad_f32": [vp, vp, i64, i64, i64, vp],
        "gnnmp_row_normalize_f32": [vp, vp, vp, i64, i64, vp],
        "gnnmp_propagate_cg_f32": [vp, vp, vp, vp, i, vp, i64, vp],
        "gnnmp_propagate_nn_f32": [vp, i, vp, vp, vp, i64, i64, vp],
        "gnnmp_gmm_weights_f32": [vp, vp, vp, vp, i64, i64, i64, i64, vp],
        "gnnmp_row_sqnorm_normalize_f32": [vp, vp, vp, f, i64, i64, vp],
        "gnnmp_lstm_pointwise_f32": [vp, vp, vp, vp, vp, vp, i64, i64, vp],
        "gnnmp_rowdot_f32": [vp, vp, vp, i64, i64, vp],
        "gnnmp_gru_pointwise_f32": [vp, vp, vp, vp, vp, i64, i64, vp],
        "gnnmp_row_normalize_grad_f32": [vp, vp, vp, vp, vp, vp, vp, f, i64, i64, vp],
        "gnnmp_add_f32": [vp, vp, vp, i64, vp],
        "gnnmp_axpy_f32": [f, vp, vp, vp, i64, vp],
        "gnnmp_mul_rows_f32": [vp, i64, vp, vp, i64, i64, vp],
        "gnnmp_is_sorted": [vp, i, i64, ctypes.POINTER(i), vp],
        "gnnmp_propagate_maxmin_grad_f32": [vp, vp, vp, vp, vp, i64, vp],
        "gnnmp_act_grad_f32": [vp, vp, i, vp, i64, vp],
        "gnnmp_dense_grad_w_f32": [vp, vp, i64, i64, i64, vp, vp, vp, i64, vp],
        "gnnmp_dense_grad_w2_f32": [vp, vp, i64, vp, i64, i64, i64, vp, vp, i64, vp],
        "gnnmp_pool_grad_act_f32": [vp, vp, i, i, vp, vp, i, vp, i64, i64, i64, vp],
        "gnnmp_propagate_add_mask_f32": [vp, i, vp, vp, vp, vp, vp, i64, vp],
        "gnnmp_shard_by_size": [ctypes.POINTER(i64), i64, i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64), ctypes.POINTER(i64)],
        "gnnmp_allgather_f32": [vp, vp, vp, i64, vp],
        "gnnmp_chain_jobs_create": [ctypes.POINTER(vp), vp, i64, vp],
        "gnnmp_chain_jobs_destroy": [vp],
        "gnnmp_chain_jobs_info": [vp, ctypes.POINTER(i64)],
        "gnnmp_graphconv_chain_f32": [vp, vp, vp, i64, vp, i, ctypes.POINTER(i64), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                      ctypes.POINTER(vp), ctypes.POINTER(i), i, i, i, vp, vp, i64, vp, vp, vp],
        "gnnmp_tune": [i, i],
        "gnnmp_tune_get": [i, ctypes.POINTER(i), ctypes.POINTER(i)],
        "gnnmp_plan_reset_counters": [vp, vp],
        "gnnmp_propagate_f64": [vp, i, i, vp, vp, vp, vp, vp, i64, vp],
        "gnnmp_gather_f64": [vp, vp, i, i, i64, vp, i64, vp],
        "gnnmp_scatter_f64": [vp, i, vp, vp, i64, vp],
        "gnnmp_tgcn_recurrence_f32": [vp, vp, vp, vp, i64, vp, vp, i64, i64, i64, vp],
        "gnnmp_tgcn_recurrence_grad_f32": [vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, i64, i64, i64, vp],
        "gnnmp_tgcn_step_f32": [i, vp, vp, vp, i64, vp, vp, vp, i64, i64, i64, i64, vp],
        "gnnmp_tgcn_step_grad_f32": [i, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp],
        "gnnmp_negative_sample": [vp, vp, i, i, i64, i64, i64, i, i, u64, vp, vp, i64, ctypes.POINTER(i64), vp],
        "gnnmp_rand_edge_split": [vp, vp, i, i, i64, i, i64, u64, vp, vp, vp, vp, vp],
        "gnnmp_edge_dot_grad_f32": [vp, vp, vp, vp, vp, vp, vp, i64, vp],
        "gnnmp_knn_graph_f32": [ctypes.POINTER(vp), vp, i64, i64, i64, vp, i, i, i64, i, vp],
        "gnnmp_radius_graph_f32": [ctypes.POINTER(vp), vp, i64, i64, f, vp, i, i, i64, i, vp],
        "gnnmp_hyperbolic_graph_f32": [ctypes.POINTER(vp), vp, i64, f, f, vp, i, i, i64, i, vp],
        "gnnmp_hetero_propagate_f32": [ctypes.POINTER(HeteroDst), i, i64, vp],
        "gnnmp_hetero_propagate_grad_f32": [ctypes.POINTER(HeteroSrc), i, i64, vp],
        "gnnmp_hetero_attn_f32": [ctypes.POINTER(HeteroAttnDst), i, i64, i64, vp],
        "gnnmp_coalesce_edges": [ctypes.POINTER(CoalesceJob), ctypes.POINTER(i64), vp],
        "gnnmp_compact_edges": [ctypes.POINTER(CompactJob), ctypes.POINTER(i64), vp],
        "gnnmp_has_multi_edges": [vp, vp, i, i, i64, ctypes.POINTER(i), vp],
        "gnnmp_has_isolated_nodes": [vp, ctypes.POINTER(i), vp],
        "gnnmp_random_walk_pe_f32": [vp, ctypes.POINTER(RwpeJob), vp],
        "gnnmp_ppr_diffusion_f32": [vp, ctypes.POINTER(PprJob), vp],
        "gnnmp_edge_conv_f32": [vp, ctypes.POINTER(EdgeConvJob), i64, vp],
        "gnnmp_edge_conv_grad_f32": [vp, vp, ctypes.POINTER(EdgeConvGradJob), i64, vp],
        "gnnmp_cg_conv_grad_f32": [vp, vp, ctypes.POINTER(CGConvGradJob), i64, vp],
        "gnnmp_nn_conv_grad_f32": [vp, ctypes.POINTER(NNConvGradJob), i64, i64, vp],
        "gnnmp_egnn_edge_f32": [ctypes.POINTER(EgnnEdgeJob), i64, i64, i64, vp],
        "gnnmp_egnn_coord_f32": [vp, ctypes.POINTER(EgnnCoordJob), i64, vp],
        "gnnmp_egnn_coord_grad_f32": [vp, vp, ctypes.POINTER(EgnnCoordGradJob), i64, vp],
        "gnnmp_act_grad_z_f32": [ctypes.POINTER(ActGradZJob), i64, vp],
        "gnnmp_gmm_conv_f32": [vp, ctypes.POINTER(GmmConvJob), i64, i64, vp],
        "gnnmp_gmm_conv_grad_f32": [vp, vp, ctypes.POINTER(GmmConvGradJob), i64, i64, vp],
        "gnnmp_gmm_weights_grad_f32": [ctypes.POINTER(GmmWeightsGradJob), i64, i64, i64, vp],
        "gnnmp_megnet_edge_f32": [vp, ctypes.POINTER(MegnetEdgeJob), i64, vp],
        "gnnmp_megnet_edge_grad_f32": [vp, vp, ctypes.POINTER(MegnetEdgeGradJob), i64, vp],
        "gnnmp_aggregate_grad_f32": [vp, ctypes.POINTER(AggregateGradJob), i, i64, vp],
        "gnnmp_segment_attn_pool_f32": [ctypes.POINTER(SegmentAttnJob), i64, i64, i64, i64, vp],
        "gnnmp_segment_attn_pool_grad_f32": [ctypes.POINTER(SegmentAttnGradJob), i64, i64, i64, i64, vp],
        "gnnmp_lstm_pointwise_grad_f32": [ctypes.POINTER(LstmGradJob), i64, i64, vp],
        "gnnmp_poly_hop_f32": [vp, ctypes.POINTER(PolyHopJob), i64, vp],
        "gnnmp_gru_pointwise_grad_f32": [ctypes.POINTER(GruGradJob), i64, i64, vp],
        "gnnmp_poly_hop_ld_f32": [vp, ctypes.POINTER(PolyHopLdJob), i64, vp],
        "gnnmp_gru_cell_f32": [i, ctypes.POINTER(GruCellJob), i64, i64, i64, i64, vp],
        "gnnmp_gru_cell_grad_f32": [i, ctypes.POINTER(GruCellGradJob), i64, i64, i64, i64, vp],
        "gnnmp_lstm_cell_f32": [ctypes.POINTER(LstmCellJob), i64, i64, i64, i64, vp],
        "gnnmp_lstm_cell_grad_f32": [ctypes.POINTER(LstmCellGradJob), i64, i64, i64, i64, vp],
        "gnnmp_lstm_matvec_cell_f32": [ctypes.POINTER(LstmMatvecJob), i64, vp],
        "gnnmp_lstm_matvec_grad_f32": [ctypes.POINTER(LstmMatvecGradJob), i64, vp],
        "gnnmp_outer_accum_f32": [ctypes.POINTER(OuterAccumJob), i64, i64, i64, vp],
        "gnnmp_attn_conv_edge_f32": [vp, i, ctypes.POINTER(AttnEdgeJob), i64, i64, vp],
        "gnnmp_attn_conv_edge_grad_f32": [vp, vp, i, ctypes.POINTER(AttnEdgeGradJob), i64, i64, vp],
        "gnnmp_plan_keep_nodes": [ctypes.POINTER(vp), vp, vp, vp, vp, vp, ctypes.POINTER(i64), vp],
        "gnnmp_topk_score_f32": [vp, vp, vp, i64, i64, vp],
        "gnnmp_topk_select_f32": [ctypes.POINTER(TopkJob), i64, vp],
        "gnnmp_topk_gate_f32": [ctypes.POINTER(TopkGateJob), i64, i64, vp],
        "gnnmp_topk_gate_grad_f32": [ctypes.POINTER(TopkGateGradJob), i64, i64, vp],
        "gnnmp_gat_conv_edge_stats_f32": [vp, vp, vp, vp, vp, f, vp, i, vp, vp, i64, i64, vp],
        "gnnmp_gat_conv_edge_grad_f32": [vp, vp, ctypes.POINTER(GatEdgeGradJob), i64, i64, vp],
        "gnnmp_gat_edge_fold_f32": [vp, vp, vp, i64, i64, i64, vp],
        "gnnmp_gat_edge_fold_grad_f32": [vp, vp, vp, vp, vp, i64, i64, i64, vp],
        "gnnmp_debug_random_walk_pe_f32": [vp, ctypes.POINTER(RwpeJob), i64, vp],
        "gnnmp_debug_dense_route": [ctypes.POINTER(i)],
    }
    for name, args in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            # an OLDER build named by GNNMP_LIB for a same-box A/B run may predate an entry point; the library of this tree must
            # export every one of them (tests/test_abi.py checks that)
            if os.environ.get("GNNMP_LIB"):
                continue
            raise
        fn.argtypes = args
        fn.restype = i
    L.gnnmp_dense_grad_workspace.argtypes = [i64, i64, i64]
    L.gnnmp_dense_grad_workspace.restype = i64
    try:
        L.gnnmp_dense_grad_w2_workspace.argtypes = [i64, i64, i64, i64]
        L.gnnmp_dense_grad_w2_workspace.restype = i64
    except AttributeError:
        if not os.environ.get("GNNMP_LIB"):
            raise
    try:
        L.gnnmp_lstm_matvec_grad_workspace.argtypes = [i64]
        L.gnnmp_lstm_matvec_grad_workspace.restype = i64
    except AttributeError:
        if not os.environ.get("GNNMP_LIB"):
            raise
    try:
        L.gnnmp_graphconv_chain_scratch_floats.argtypes = [i64, i, ctypes.POINTER(i64), i64]
        L.gnnmp_graphconv_chain_scratch_floats.restype = i64
    except AttributeError:
        if not os.environ.get("GNNMP_LIB"):
            raise
    # GNNMP_KNOBS="0=1,5=2": tuning knobs applied at load (test runs that force the narrow-vector / other template variants of
    # every kernel: `GNNMP_KNOBS=0=1 python -m pytest tests -m gpu`)
    _lib = L
    for kv in filter(None, os.environ.get("GNNMP_KNOBS", "").split(",")):
        k, v = kv.split("=")
        tune(int(k), int(v))
    return L


def check(rc):
    if rc != OK:
        raise GnnmpError(rc, load().gnnmp_last_error().decode())


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("gnnmp needs an AMD GPU (gfx950); there is no CPU fallback on the product path")


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """device pointer of a tensor (None -> NULL)"""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


# ---- kernel probe: HIP events around named launches, on the stream they are launched on -------------------------------------------------
# bench.py times the dominant kernels INSIDE its timed steps with this (the roofline figure of the bench line is the in-step duration, the
# one a rocprofv3 kernel trace of the same command shows); off (None) it costs one global read per call.
_probe = None


class EventProbe:
    """spans[name] = list of (start, end) torch.cuda.Event pairs recorded around every launch of `name` while the probe is set"""

    def __init__(self):
        self.spans = {}

    def begin(self):
        import torch
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, name, e0):
        import torch
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.spans.setdefault(name, []).append((e0, e1))

    def times_ms(self, name):
        """call after a synchronisation"""
        return [a.elapsed_time(b) for a, b in self.spans.get(name, [])]


def set_probe(p):
    global _probe
    _probe = p


KNOB_TGCN, KNOB_EDGE_DOT_GRAD, KNOB_HETERO = Knob.TGCN, Knob.EDGE_DOT_GRAD, Knob.HETERO      # (the names older callers use)


def knob(k: int) -> int:
    """the library's current value of a knob (csrc/knobs.h): whoever set it, tune() here or a raw gnnmp_tune"""
    v = ctypes.c_int()
    check(load().gnnmp_tune_get(k, ctypes.byref(v), None))
    return v.value


def knob_default(k: int) -> int:
    """the value a knob starts at (the table of csrc/knobs.h, as compiled into the library)"""
    d = ctypes.c_int()
    check(load().gnnmp_tune_get(k, None, ctypes.byref(d)))
    return d.value


def tune(knob: int, value: int):
    """perf-experiment hook (csrc/knobs.h); not part of the drop-in surface"""
    check(load().gnnmp_tune(knob, value))


@contextlib.contextmanager
def tuned(k: int, value: int):
    """a knob set to `value` inside the block; the value the library held before comes back on the way out, on an exception too"""
    before = knob(k)
    tune(k, value)
    try:
        yield
    finally:
        tune(k, before)


def tuned_bits(k: int, set: int = 0, clear: int = 0):
    """tuned() for a bit field (Knob.VARIANT): the current value with the bits of `set` on and those of `clear` off"""
    return tuned(k, (knob(k) | int(set)) & ~int(clear))
