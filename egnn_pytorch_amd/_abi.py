"""ctypes binding of libegnn_hip.so (C ABI declared in include/egnn_hip.h).

The library is the product: there is NO fallback.  If it is missing or does not export the
symbols of the header this module raises, and every forward call raises with it.

`import torch` happens before `ctypes.CDLL` on purpose: torch bundles its own libamdhip64.so.7
(same SONAME as /opt/rocm's); loading torch first makes our library bind to the HIP runtime torch
already initialised, so `torch.cuda.current_stream().cuda_stream` and `tensor.data_ptr()` are valid
inside the library (two HIP runtimes in one process would make stream handles unusable).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import torch  # noqa: F401  (must precede CDLL, see module docstring)

ABI_VERSION = 44
_LIB_NAME = "libegnn_hip.so"
_PKG_DIR = os.path.dirname(os.path.abspath(__file__))


class EdgeArgs(Structure):
    """Mirror of `struct egnn_edge_args` (include/egnn_hip.h) -- field order and types must match."""
    _fields_ = [
        ("B", c_int32), ("N", c_int32), ("K", c_int32), ("dim", c_int32), ("m_dim", c_int32),
        ("H", c_int32), ("Hp", c_int32), ("fourier", c_int32), ("edge_dim", c_int32),
        ("S", c_int32), ("pi_split", c_int32),
        ("Pi", c_void_p), ("Pj", c_void_p), ("ldp", c_int64),
        ("Wst", c_void_p), ("wst_terms", c_int32), ("ws_inv_scale", c_float), ("W2h", c_void_p), ("w2_inv_scale", c_float), ("b2", c_void_p),
        ("gate_w", c_void_p), ("gate_b", c_void_p),
        ("W3h", c_void_p), ("w3_inv_scale", c_float), ("b3", c_void_p), ("W4", c_void_p), ("b4", c_void_p),
        ("coors_scale", c_void_p),
        ("coors", c_void_p), ("coor_dim", c_int32), ("edges", c_void_p), ("mask", c_void_p), ("idx", c_void_p), ("rank", c_void_p),
        ("order", c_void_p),
        ("valid_radius", c_float), ("clamp", c_float), ("pool_mean", c_int32),
        ("m_i", c_void_p), ("coors_out", c_void_p),
        ("node_hi", c_void_p), ("node_lo", c_void_p), ("node_kp", c_int32),
        ("status", c_void_p),
        ("U_out", c_void_p),
        ("edges_by_k", c_int32),
        ("slots", c_void_p),
        ("drop_thr", c_uint32), ("drop_seed", c_uint32), ("drop_inv_keep", c_float),
        ("algo", c_int32),
    ]


class EdgeExactArgs(Structure):
    """Mirror of `struct egnn_edge_exact_args` (include/egnn_hip.h): the edge pass in plain fp32 (wide-range path) / float64."""
    _fields_ = [
        ("B", c_int32), ("N", c_int32), ("K", c_int32), ("m_dim", c_int32), ("H", c_int32), ("fourier", c_int32),
        ("edge_dim", c_int32), ("coor_dim", c_int32), ("pool_mean", c_int32), ("edges_by_k", c_int32),
        ("Pi", c_void_p), ("Pj", c_void_p), ("ldp", c_int64), ("Ws", c_void_p), ("ldws", c_int64),
        ("W2", c_void_p), ("b2", c_void_p), ("gate_w", c_void_p), ("gate_b", c_void_p),
        ("W3", c_void_p), ("b3", c_void_p), ("W4", c_void_p), ("b4", c_void_p), ("coors_scale", c_void_p),
        ("coors", c_void_p), ("edges", c_void_p), ("mask", c_void_p), ("idx", c_void_p), ("rank", c_void_p),
        ("valid_radius", c_double), ("clamp", c_double),
        ("m_i", c_void_p), ("coors_out", c_void_p), ("edge_ws", c_void_p), ("U_out", c_void_p),
        ("drop_thr", c_uint32), ("drop_seed", c_uint32), ("drop_inv_keep", c_float), ("drop_eid0", c_int64),
    ]


class EdgeExactBwdArgs(Structure):
    """Mirror of `struct egnn_edge_exact_bwd_args` (include/egnn_hip.h): the E x H work of the plain-fp32 / float64 backward."""
    _fields_ = [
        ("B", c_int32), ("N", c_int32), ("K", c_int32), ("m_dim", c_int32), ("H", c_int32), ("fourier", c_int32),
        ("edge_dim", c_int32), ("coor_dim", c_int32), ("edges_by_k", c_int32), ("reserved", c_int32),
        ("Pi", c_void_p), ("Pj", c_void_p), ("ldp", c_int64), ("Ws", c_void_p), ("ldws", c_int64),
        ("W2", c_void_p), ("coors", c_void_p), ("edges", c_void_p), ("idx", c_void_p), ("gU", c_void_p),
        ("A_T", c_void_p), ("DZ_T", c_void_p), ("g_scal", c_void_p),
        ("drop_thr", c_uint32), ("drop_seed", c_uint32), ("drop_inv_keep", c_float), ("drop_eid0", c_int64),
    ]


class EdgeTailExactArgs(Structure):
    """Mirror of `struct egnn_edge_tail_exact_args` (include/egnn_hip.h): the per-edge chain behind u in closed form, any head / C."""
    _fields_ = [
        ("B", c_int32), ("N", c_int32), ("K", c_int32), ("m_dim", c_int32), ("coor_dim", c_int32), ("norm_coors", c_int32),
        ("eps", c_double), ("clamp", c_double),
        ("u", c_void_p), ("coors", c_void_p), ("idx", c_void_p), ("pair_mask", c_void_p), ("g_coors_out", c_void_p), ("g_msum", c_void_p),
        ("W3", c_void_p), ("b3", c_void_p), ("W4", c_void_p), ("b4", c_void_p), ("scale", c_void_p), ("gate_w", c_void_p), ("gate_b", c_void_p),
        ("gU", c_void_p), ("g_rel", c_void_p), ("ghid_t", c_void_p), ("a3_t", c_void_p), ("mm_t", c_void_p), ("m0_t", c_void_p),
        ("g_w", c_void_p), ("g_scale", c_void_p), ("g_gate", c_void_p),
        ("drop_thr", c_uint32), ("drop_seed", c_uint32), ("drop_inv_keep", c_float), ("drop_eid0", c_int64),
    ]


class EdgeHiddenArgs(Structure):
    """Mirror of `struct egnn_edge_hidden_args` (include/egnn_hip.h): the E x H block as a twice-differentiable op."""
    _fields_ = [
        ("B", c_int32), ("N", c_int32), ("K", c_int32), ("m_dim", c_int32), ("H", c_int32), ("S", c_int32),
        ("idx", c_void_p), ("Pi", c_void_p), ("Pj", c_void_p), ("s", c_void_p), ("Ws", c_void_p), ("W2", c_void_p), ("b2", c_void_p),
        ("gU", c_void_p), ("cPi", c_void_p), ("cPj", c_void_p), ("cs", c_void_p), ("cWs", c_void_p), ("cW2", c_void_p), ("cb2", c_void_p),
        ("u", c_void_p), ("A_T", c_void_p), ("DZ_T", c_void_p), ("g_s", c_void_p), ("g_gU", c_void_p), ("DAV_T", c_void_p), ("R_T", c_void_p),
        ("drop_thr", c_uint32), ("drop_seed", c_uint32), ("drop_inv_keep", c_float), ("drop_eid0", c_int64),
    ]


class EdgeBwdArgs(Structure):
    """Mirror of `struct egnn_edge_bwd_args` (include/egnn_hip.h) -- field order and types must match."""
    _fields_ = [
        ("B", c_int32), ("N", c_int32), ("K", c_int32), ("Hp", c_int32), ("S", c_int32), ("by_dest", c_int32),
        ("n_slabs", c_int32), ("wst_terms", c_int32),
        ("L", c_int64), ("E", c_int64),
        ("ent", c_void_p), ("Pi", c_void_p), ("Pj", c_void_p), ("ldp", c_int64),
        ("Wst", c_void_p), ("ws_inv_scale", c_float), ("idx", c_void_p), ("W2Th", c_void_p), ("gU", c_void_p),
        ("gu_scale", c_float), ("inv_scale", c_float), ("scal", c_void_p), ("Ws", c_void_p), ("scal_scale", c_void_p),
        ("part_rows", c_void_p), ("ld_rows", c_int64),
        ("dW2_part", c_void_p), ("dWs_part", c_void_p), ("ds_part", c_void_p),
        ("WsTh", c_void_p), ("wst_inv_scale", c_float),
        ("drop_thr", c_uint32), ("drop_seed", c_uint32), ("drop_inv_keep", c_float), ("drop_eid0", c_int64),
        ("row_pairs", c_int32), ("rows_amax", c_void_p), ("work", c_void_p), ("work_bytes", c_int64),
    ]


class EdgeTailArgs(Structure):
    """Mirror of `struct egnn_edge_tail_args` (include/egnn_hip.h)."""
    _fields_ = [
        ("B", c_int32), ("N", c_int32), ("K", c_int32), ("norm_coors", c_int32), ("clamp", c_float), ("eps", c_float),
        ("u", c_void_p), ("coors", c_void_p), ("idx", c_void_p), ("pair_mask", c_void_p), ("g_coors_out", c_void_p),
        ("g_msum", c_void_p), ("W3", c_void_p), ("b3", c_void_p), ("W4", c_void_p), ("b4", c_void_p), ("scale", c_void_p),
        ("gU", c_void_p), ("g_rel", c_void_p), ("g_hid", c_void_p), ("a3", c_void_p), ("g_w", c_void_p), ("g_scale", c_void_p),
        ("gate_w", c_void_p), ("gate_b", c_void_p), ("g_gate", c_void_p),
        ("part", c_void_p), ("rel_out", c_void_p), ("dist_out", c_void_p), ("amax_gu", c_void_p),
        ("drop_thr", c_uint32), ("drop_seed", c_uint32), ("drop_inv_keep", c_float), ("drop_eid0", c_int64),
    ]


class LayerDesc(Structure):
    """Mirror of `struct egnn_layer_desc` (include/egnn_hip.h)."""
    _fields_ = [("dim", c_int32), ("edge_dim", c_int32), ("m_dim", c_int32), ("fourier_features", c_int32),
                ("num_nearest_neighbors", c_int32), ("norm_feats", c_int32), ("norm_coors", c_int32), ("update_feats", c_int32),
                ("update_coors", c_int32), ("only_sparse_neighbors", c_int32), ("soft_edges", c_int32), ("pool_mean", c_int32),
                ("valid_radius", c_float), ("coor_weights_clamp_value", c_float), ("ln_eps", c_float)]


PARAM_FIELDS = ("edge_mlp_0_weight", "edge_mlp_0_bias", "edge_mlp_3_weight", "edge_mlp_3_bias", "edge_gate_0_weight",
                "edge_gate_0_bias", "node_norm_weight", "node_norm_bias", "coors_norm_scale", "node_mlp_0_weight",
                "node_mlp_0_bias", "node_mlp_3_weight", "node_mlp_3_bias", "coors_mlp_0_weight", "coors_mlp_0_bias",
                "coors_mlp_3_weight", "coors_mlp_3_bias")


class LayerParams(Structure):
    """Mirror of `struct egnn_layer_params`: host pointers to the reference's state_dict tensors (field = key with '.' -> '_')."""
    _fields_ = [(f, c_void_p) for f in PARAM_FIELDS]


INFO_OFFSETS = ("wcat_hi", "wcat_lo", "bcat", "wst", "w2h", "b2", "gate_w", "gate_b", "w3h", "b3", "w4", "b4", "coors_scale",
                "w5_hi", "w5_lo", "b5", "w6_hi", "w6_lo", "b6", "gamma", "beta")


class PackedInfo(Structure):
    """Mirror of `struct egnn_packed_info`."""
    _fields_ = [("H", c_int32), ("Hp", c_int32), ("S", c_int32), ("NM", c_int32),
                ("wcat_rows", c_int32), ("w5_rows", c_int32), ("w6_rows", c_int32),
                ("wcat_inv_scale", c_float), ("ws_inv_scale", c_float), ("w2_inv_scale", c_float), ("w3_inv_scale", c_float),
                ("w5_inv_scale", c_float), ("w6_inv_scale", c_float)] + \
               [(f, c_uint64) for f in INFO_OFFSETS] + [("bytes", c_uint64)]


class ForwardOpts(Structure):
    """Mirror of `struct egnn_forward_opts`."""
    _fields_ = [("side_stream", c_void_p), ("ev_fork", c_void_p), ("ev_join", c_void_p), ("order", c_void_p), ("nmf_img", c_void_p),
                ("order_is_hint", c_int32), ("status_words", c_int32), ("status_pub", c_void_p), ("status_seq", c_int32),
                ("reserved", c_int32)]


# (header struct name, mirror), in the order of egnn_struct_bytes(which): load() compares the sizes.  (LayerParams mirrors
# egnn_layer_params, which egnn_struct_bytes does not cover.)
STRUCTS = (
    ("egnn_edge_args", EdgeArgs), ("egnn_edge_bwd_args", EdgeBwdArgs), ("egnn_edge_tail_args", EdgeTailArgs),
    ("egnn_layer_desc", LayerDesc), ("egnn_packed_info", PackedInfo), ("egnn_edge_exact_args", EdgeExactArgs),
    ("egnn_edge_exact_bwd_args", EdgeExactBwdArgs), ("egnn_edge_tail_exact_args", EdgeTailExactArgs),
    ("egnn_forward_opts", ForwardOpts), ("egnn_edge_hidden_args", EdgeHiddenArgs),
)

_LAYER_FORWARD = (POINTER(LayerDesc), POINTER(PackedInfo), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                  c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p)

# Every prototype of include/egnn_hip.h, once: (names that share the signature, restype, argtypes).  This table is the whole
# binding -- load() applies it in one loop -- and tests/test_abi_agreement.py checks it against the header type by type.
SIGNATURES = {name: (restype, argtypes) for names, restype, argtypes in (
    ("egnn_abi_version egnn_edge_tail_part_floats egnn_edge_bwd_chunk_steps", c_int, ()),
    ("egnn_struct_bytes", c_int64, (c_int,)),
    ("egnn_status_publish", c_int, (c_void_p, c_void_p, c_int, c_int32, c_void_p)),
    ("egnn_error_string", c_char_p, (c_int,)),
    ("egnn_padded_hidden egnn_edge_mfmas egnn_token_attn_bwd_chunks", c_int, (c_int,)),
    # neighbour selection
    ("egnn_knn_select_f32 egnn_knn_select_f64 egnn_knn_select_stream_f32 egnn_knn_select_stream_f64", c_int,
     (c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p)),
    ("egnn_knn_select_csr_f32 egnn_knn_select_csr_f64", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p)),
    ("egnn_knn_grid_workspace_bytes egnn_knn_grid_workspace_bytes_f64 egnn_dest_lists_capacity", c_size_t, (c_int, c_int, c_int)),
    ("egnn_knn_grid_rowflag_offset_f64", c_size_t, (c_int, c_int)),
    ("egnn_knn_select_grid_f32 egnn_knn_select_grid_f64", c_int,
     (c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p)),
    ("egnn_knn_select_grid_csr_f32 egnn_knn_select_grid_csr_f64", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p)),
    ("egnn_knn_select_segments_f32 egnn_knn_select_segments_f64", c_int,
     (c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p)),
    ("egnn_knn_segments_lds_nodes", c_int, (c_int,)),
    # per-graph readout of a packed batch
    ("egnn_segment_reduce_chunk_rows", c_int, ()),
    ("egnn_segment_reduce_workspace_bytes", c_size_t, (c_int, c_int64, c_int, c_int)),
    ("egnn_segment_reduce_f32 egnn_segment_reduce_f64", c_int,
     (c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_int, c_void_p,
      c_void_p, c_void_p, c_size_t, c_void_p)),
    ("egnn_segment_broadcast_f32 egnn_segment_broadcast_f64", c_int, (c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p)),
    ("egnn_segment_scatter_rows_f32 egnn_segment_scatter_rows_f64", c_int,
     (c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p)),
    ("egnn_segment_gather_rows_f32 egnn_segment_gather_rows_f64", c_int, (c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p)),
    # per-graph softmax of a packed batch
    ("egnn_segment_softmax_stats_f32 egnn_segment_softmax_stats_f64", c_int,
     (c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p,
      c_void_p, c_size_t, c_void_p)),
    ("egnn_segment_softmax_apply_f32 egnn_segment_softmax_apply_f64", c_int,
     (c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p)),
    ("egnn_segment_pool_f32 egnn_segment_pool_f64", c_int,
     (c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
      c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p)),
    ("egnn_segment_pool_bwd_f32 egnn_segment_pool_bwd_f64", c_int,
     (c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p,
      c_void_p, c_void_p)),
    # adjacency: CSR expansion, degrees, dense expansion
    ("egnn_adj_csr_workspace_bytes egnn_adj_expand_workspace_bytes", c_size_t, (c_int, c_int)),
    ("egnn_adj_csr_square_count", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p)),
    ("egnn_adj_csr_square_fill", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
      c_int64, c_void_p, c_size_t, c_int, c_void_p)),
    ("egnn_csr_slot_labels_u8", c_int, (c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p)),
    ("egnn_adj_max_degree_u8", c_int, (c_void_p, c_int64, c_int, c_void_p, c_void_p)),
    ("egnn_adj_expand_u8 egnn_adj_expand_wide_u8", c_int,
     (c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p)),
    # scheduling aids and the backward's transposed neighbour list
    ("egnn_spatial_order_f32", c_int, (c_void_p, c_int, c_int, c_void_p, c_void_p)),
    ("egnn_spatial_order_masked_f32", c_int, (c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p)),
    ("egnn_dest_lists_i32", c_int,
     (c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p)),
    ("egnn_slot_prep_f32", c_int, (c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_int, c_void_p, c_void_p)),
    # split-f16 GEMMs and their operand passes
    ("egnn_packed_halves egnn_split_scaled_colsum_rows", c_int64, (c_int64, c_int)),
    ("egnn_linear_hl_f32", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64,
      c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p)),
    ("egnn_linear_hl_lda_f32", c_int,
     (c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int,
      c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p)),
    ("egnn_linear_hl_lda_rows_f32", c_int,
     (c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int,
      c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p)),
    ("egnn_linear_hl_drop_f32", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64,
      c_int, c_int, c_int, c_int, c_int, c_uint32, c_uint32, c_float, c_void_p, c_void_p)),
    ("egnn_edge_pw_covers", c_int, (c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64)),
    ("egnn_edge_fused_covers", c_int, (c_int, c_int, c_int64)),
    ("egnn_split_scaled_f16", c_int,
     (c_void_p, c_int64, c_int64, c_int, c_float, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p)),
    ("egnn_split_scaled_both_f16", c_int,
     (c_void_p, c_int64, c_int64, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64,
      c_void_p)),
    ("egnn_silu_bwd_f32 egnn_gelu_bwd_f32", c_int, (c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p)),
    ("egnn_silu_bwd_drop_f32", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_uint32, c_uint32, c_float, c_int64, c_int, c_void_p)),
    ("egnn_linear_hl_splitk_f32", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_void_p)),
    ("egnn_sum_parts_f32", c_int, (c_void_p, c_int, c_int64, c_float, c_void_p, c_void_p)),
    ("egnn_absmax_f32", c_int, (c_void_p, c_int64, c_void_p, c_void_p)),
    ("egnn_unsplit_words_f32", c_int, (c_void_p, c_int64, c_int64, c_int, c_void_p)),
    ("egnn_node_mlp_fused_halves", c_int64, (c_int, c_int)),
    ("egnn_node_mlp_fused_pack_f16", c_int, (c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p)),
    ("egnn_node_mlp_fused_f32", c_int,
     (c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p)),
    ("egnn_split_f16", c_int, (c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p)),
    ("egnn_node_prep_hl", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int64, c_int, c_int,
      c_void_p, c_void_p)),
    # the fused edge pass, its look-up tables and its backward
    ("egnn_edge_fused_f32", c_int, (POINTER(EdgeArgs), c_void_p)),
    ("egnn_edge_features_gather_f32 egnn_edge_features_gather_f64 egnn_edge_features_gather_slot_f32 egnn_edge_features_gather_slot_f64",
     c_int, (c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p)),
    ("egnn_edge_features_grad_f32 egnn_edge_features_grad_f64 egnn_edge_features_grad_slot_f32 egnn_edge_features_grad_slot_f64", c_int,
     (c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
      c_void_p, POINTER(c_int64), c_void_p)),
    ("egnn_edge_features_gather_csr_f32 egnn_edge_features_gather_csr_f64", c_int,
     (c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
      c_void_p)),
    ("egnn_edge_features_grad_csr_f32 egnn_edge_features_grad_csr_f64", c_int,
     (c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
      c_void_p, c_void_p, POINTER(c_int64), c_void_p)),
    ("egnn_edge_bwd_pass_f32", c_int, (POINTER(EdgeBwdArgs), c_void_p)),
    ("egnn_edge_bwd_work_bytes", c_size_t, (c_int64, c_int, c_int, c_int)),
    ("egnn_edge_tail_bwd_f32", c_int, (POINTER(EdgeTailArgs), c_void_p)),
    ("egnn_edge_pool_f32", c_int, (c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p)),
    ("egnn_rows_gather_sum_f32", c_int, (c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p)),
    # whole layers
    ("egnn_packed_weights_bytes", c_size_t, (POINTER(LayerDesc),)),
    ("egnn_packed_layout", c_int, (POINTER(LayerDesc), POINTER(PackedInfo))),
    ("egnn_pack_weights_host", c_int, (POINTER(LayerDesc), POINTER(LayerParams), c_void_p, POINTER(PackedInfo))),
    ("egnn_workspace_bytes", c_size_t, (POINTER(LayerDesc), c_int, c_int, c_int)),
    ("egnn_layer_forward_f32", c_int, _LAYER_FORWARD),
    ("egnn_layer_forward_opts_f32", c_int, _LAYER_FORWARD + (POINTER(ForwardOpts),)),
    # global attention blocks
    ("egnn_induced_attn_f32", c_int,
     (c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p)),
    ("egnn_token_attn_f32", c_int,
     (c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int64, c_void_p)),
    ("egnn_induced_attn_bwd_f32", c_int,
     (c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p,
      c_void_p)),
    ("egnn_induced_attn_bwd_work_floats", c_int64, (c_int, c_int, c_int, c_int, c_int)),
    ("egnn_token_attn_bwd_f32", c_int,
     (c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p)),
    ("egnn_layer_norm_bwd_parts", c_int, (c_int64,)),
    ("egnn_layer_norm_bwd_f32", c_int,
     (c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p)),
    # plain fp32 / float64 kernels
    ("egnn_linear_f32 egnn_linear_f64", c_int,
     (c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p)),
    ("egnn_node_prep_f32", c_int, (c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int, c_int, c_void_p)),
    ("egnn_node_prep_f64", c_int, (c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_int64, c_int, c_int, c_void_p)),
    ("egnn_drop_silu_f32 egnn_drop_silu_f64", c_int,
     (c_void_p, c_int64, c_int64, c_int, c_uint32, c_uint32, c_float, c_int64, c_void_p)),
    ("egnn_edge_exact_workspace_bytes", c_size_t, (c_int, c_int, c_int, c_int, c_int)),
    ("egnn_edge_exact_f32 egnn_edge_exact_f64", c_int, (POINTER(EdgeExactArgs), c_void_p)),
    ("egnn_edge_exact_bwd_f32 egnn_edge_exact_bwd_f64", c_int, (POINTER(EdgeExactBwdArgs), c_void_p)),
    ("egnn_edge_exact_node_sums_f32 egnn_edge_exact_node_sums_f64", c_int,
     (c_void_p, c_int64, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p)),
    ("egnn_edge_tail_exact_bwd_f32 egnn_edge_tail_exact_bwd_f64", c_int, (POINTER(EdgeTailExactArgs), c_void_p)),
    ("egnn_edge_hidden_fwd_f32 egnn_edge_hidden_fwd_f64 egnn_edge_hidden_bwd_f32 egnn_edge_hidden_bwd_f64 "
     "egnn_edge_hidden_bwd2_f32 egnn_edge_hidden_bwd2_f64", c_int, (POINTER(EdgeHiddenArgs), c_void_p)),
) for name in names.split()}
SYMBOLS = tuple(SIGNATURES)


def layer_desc(layer) -> "LayerDesc":
    """egnn_layer_desc of an egnn_pytorch_amd.EGNN (or reference EGNN-like) module."""
    import math
    d = LayerDesc()
    d.dim, d.edge_dim, d.m_dim, d.fourier_features = layer.dim, layer.edge_dim, layer.m_dim, layer.fourier_features
    d.num_nearest_neighbors = layer.num_nearest_neighbors
    d.norm_feats, d.norm_coors = int(layer.norm_feats), int(layer.norm_coors)
    d.update_feats, d.update_coors = int(layer.node_mlp is not None), int(layer.coors_mlp is not None)
    d.only_sparse_neighbors, d.soft_edges = int(layer.only_sparse_neighbors), int(layer.edge_gate is not None)
    d.pool_mean = int(layer.m_pool_method == "mean")
    d.valid_radius = 3.0e38 if math.isinf(layer.valid_radius) else float(layer.valid_radius)
    cv = layer.coor_weights_clamp_value
    d.coor_weights_clamp_value = -1.0 if cv is None else float(cv)
    d.ln_eps = float(layer.node_norm.eps) if layer.norm_feats else 1e-5
    return d


class EGNNHipError(RuntimeError):
    pass


class EGNNRangeError(EGNNHipError):
    """A finite value left the range the split-fp16 arithmetic of the gfx950 path can carry (include/egnn_hip.h:
    EGNN_RANGE_*).  The outputs of that call are non-finite; the reference (plain fp32) has no such limit.
    origin: "call" (this forward), "backward" (bits an earlier backward left: the forward that reports them is valid and is not
    re-run) or "earlier" (deferred mode: some earlier call); bits: the status bits."""
    origin = "call"
    bits = 0


RANGE_BITS = {
    1: "a GEMM input (feats / [LayerNorm(feats) | m_i] / node_mlp hidden activation) with |x| >= 65504",
    2: "a node projection P_i = -log2(e) (W_i h_i + b) with |P| >= 65504",
    4: "a per-edge scalar (squared distance, fourier term or edge feature) with |s| >= 6e7 * max|its weight column| scale",
    8: "an edge_mlp hidden activation beyond fp16 range (the edge message came out non-finite)",
    16: "an edge message / pooled message with |m| >= 65504",
}


_lib = None


def lib_path() -> str:
    return os.environ.get("EGNN_HIP_LIB", os.path.join(_PKG_DIR, _LIB_NAME))


def load():
    """Load (once) and return the ctypes handle.  Raises EGNNHipError if the library is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise EGNNHipError(
            f"{path} not found: the HIP extension is not built. Build it with "
            f"`python -c 'import __graft_entry__ as g; g.build()'` (or egnn_pytorch_amd/csrc/build.sh). "
            f"egnn_pytorch_amd has no CPU / PyTorch fallback.")
    try:
        lib = ctypes.CDLL(path)
    except OSError as exc:  # pragma: no cover
        raise EGNNHipError(f"cannot load {path}: {exc}") from exc
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise EGNNHipError(f"{path} does not export {missing}; rebuild it")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.egnn_abi_version() != ABI_VERSION:
        raise EGNNHipError(f"{path}: ABI version {lib.egnn_abi_version()} != {ABI_VERSION}; rebuild it")
    for which, (_, mirror) in enumerate(STRUCTS):
        if lib.egnn_struct_bytes(which) != ctypes.sizeof(mirror):
            raise EGNNHipError(f"{path}: sizeof({mirror.__name__}) = {ctypes.sizeof(mirror)} here, {lib.egnn_struct_bytes(which)} in the "
                               f"library: the ctypes mirror in _abi.py and include/egnn_hip.h disagree")
    _lib = lib
    return lib


def check(code: int, what: str):
    """Map a C-ABI return code to an exception (0 = ok, <0 = EGNN_E_*, >0 = hipError_t)."""
    if code == 0:
        return
    msg = load().egnn_error_string(code).decode()
    if code == -5:   # EGNN_E_K_GT_N -- same text torch.topk raises in the reference (egnn_pytorch.py:258)
        raise RuntimeError(f"{what}: {msg}")
    raise EGNNHipError(f"{what} failed with code {code}: {msg}")
