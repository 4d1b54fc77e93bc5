"""Loads lib/libptv3_hip.so and declares the C ABI of include/ptv3_hip.h for ctypes."""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint32, c_void_p

PTV3_F32, PTV3_BF16 = 0, 1
PTV3_PG_TRUNCATED = 16  # ptv3_pg_cluster: a point has more than 1000 neighbours (take the list path)
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
ORDER_IDS = {"z": 0, "z-trans": 1, "hilbert": 2, "hilbert-trans": 3}

_HERE = os.path.dirname(os.path.abspath(__file__))


def library_path():
    return os.environ.get("PTV3_HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libptv3_hip.so"))


P = c_void_p


class BlockTrain(ctypes.Structure):
    """struct ptv3_block_train of include/ptv3_hip.h (field for field)"""
    _fields_ = ([("n", c_int64), ("n_pad", c_int64)] +
                [(k, ctypes.c_int32) for k in ("c", "hidden", "heads", "patch", "kvol", "num_windows", "dtype", "reserved")] +
                [("scale", c_float), ("eps", c_float), ("keep1", c_float), ("keep2", c_float), ("sum_len_sq", c_double)] +
                [(k, P) for k in ("nbr", "row_order", "win_order", "win_inverse", "cu_seqlens", "feat", "conv_feat",
                                  "w_conv", "w_lin", "w_qkv", "w_proj", "w_fc1", "w_fc2",
                                  "wt_conv", "wt_lin", "wt_qkv", "wt_proj", "wt_fc1", "wt_fc2",
                                  "b_conv", "b_lin", "b_qkv", "b_proj", "b_fc1", "b_fc2", "g0", "b0", "g1", "b1", "g2", "b2",
                                  "mask1", "mask2",
                                  "c1", "c2", "f1", "t3", "qkv", "a", "f2", "t5", "h0", "h", "out",
                                  "dout", "dfeat", "dconv_feat",
                                  "dw_conv", "dw_lin", "dw_qkv", "dw_proj", "dw_fc1", "dw_fc2",
                                  "db_conv", "db_lin", "db_qkv", "db_proj", "db_fc1", "db_fc2",
                                  "dln0", "dln1", "dln2", "workspace")] +
                [("workspace_bytes", c_size_t), ("attn_lse", P)])


class ClsHeadParams(ctypes.Structure):
    """struct ptv3_cls_head_params of include/ptv3_hip.h (field for field)"""
    _fields_ = ([(k, P) for k in ("w1", "b1", "bn1_weight", "bn1_bias", "bn1_running_mean", "bn1_running_var",
                                  "w2", "b2", "bn2_weight", "bn2_bias", "bn2_running_mean", "bn2_running_var",
                                  "w3", "b3")] +
                [(k, c_float) for k in ("bn1_momentum", "bn1_eps", "bn2_momentum", "bn2_eps")])


class ClsHeadGrads(ctypes.Structure):
    """struct ptv3_cls_head_grads of include/ptv3_hip.h (field for field)"""
    _fields_ = [(k, P) for k in ("dw1", "db1", "dbn1_weight", "dbn1_bias", "dw2", "db2", "dbn2_weight", "dbn2_bias",
                                 "dw3", "db3")]


# name -> (restype, argtypes); must list every symbol include/ptv3_hip.h declares
SIGNATURES = {
    "ptv3_last_error": (c_char_p, []),
    "ptv3_version": (c_int, []),
    "ptv3_sfc_encode": (c_int, [P, c_int, P, c_int64, c_int, P, c_int, P, P]),
    "ptv3_argsort_workspace_bytes": (c_size_t, [c_int, c_int64]),
    "ptv3_argsort_i64": (c_int, [P, c_int, c_int64, c_int, P, P, P, c_size_t, P]),
    "ptv3_argsort_i64_rows": (c_int, [P, c_int, c_int64, c_int, P, P, P, P, c_size_t, P]),
    "ptv3_argsort_scan_batch": (c_int, []),
    "ptv3_coord_max": (c_int, [P, c_int, c_int64, P, P, P]),
    "ptv3_subm_sites": (c_int, [P, P, c_int, c_int64, P, P, P, c_size_t, P]),
    "ptv3_subm_build_block_table_zeroed": (c_int, [P, c_int64, P, c_size_t, P]),
    "ptv3_pad_plan": (c_int, [P, c_int, c_int64, c_int64, c_int, P, P, P, P]),
    "ptv3_window_maps": (c_int, [P, P, P, P, c_int64, c_int64, P, P, P]),
    "ptv3_window_plan": (c_int, [P, P, P, c_int, c_int, c_int64, c_int64, c_int, P, P, P, P]),
    "ptv3_window_attn_fwd": (c_int, [P, P, P, P, c_int64, c_int64, c_int, c_int, c_int, c_float, P, c_int, P]),
    "ptv3_window_attn_varlen_fwd": (c_int, [P, P, P, P, c_int, P, c_int64, c_int64, c_int, c_int, c_int, c_float,
                                            c_double, c_int, P]),
    "ptv3_window_attn_rpe_fwd": (c_int, [P, P, P, P, c_int64, c_int64, c_int, c_int, c_int, c_float, P, P, c_int,
                                         c_int, P]),
    "ptv3_subm_table_slots": (c_int64, [c_int64]),
    "ptv3_subm_build_table": (c_int, [P, c_int64, P, c_int64, P]),
    "ptv3_subm_neighbors": (c_int, [P, c_int64, P, c_int64, c_int, P, P]),
    "ptv3_subm_block_table_bytes": (c_size_t, [c_int64]),
    "ptv3_subm_build_block_table": (c_int, [P, c_int64, P, c_size_t, P]),
    "ptv3_subm_neighbors_blocks": (c_int, [P, c_int64, P, c_size_t, c_int, P, P]),
    "ptv3_gemm_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int, c_int]),
    "ptv3_gemm": (c_int, [P, P, P, c_int64, c_int, c_int, c_int, P, P, P, P, P, c_int, P, P, P, c_int, P, c_size_t,
                          P]),
    "ptv3_gemm_splits": (c_int, [c_int64, c_int, c_int, c_int, c_int]),
    "ptv3_stem_conv_blocks": (c_int, [P, P, P, c_int64, c_int, c_int, c_int, P, P, c_size_t, P, P, P, P, c_int, c_int,
                                      P]),
    "ptv3_halo_plan_bytes": (c_size_t, [c_int64]),
    "ptv3_halo_plan_shape": (c_int, [P, P]),
    "ptv3_halo_plan_build": (c_int, [P, P, c_int64, P, c_size_t, P]),
    "ptv3_conv_halo_policy": (c_int, [c_int64, c_int, c_int, c_int, c_int]),
    "ptv3_conv_halo": (c_int, [P, P, P, c_int64, c_int, P, P, P, c_size_t, P, P, P, c_int, P, P, P, c_int, P]),
    "ptv3_block_fusable": (c_int, [c_int, c_int, c_int, c_int64]),
    "ptv3_rows_linear_capable": (c_int, [c_int, c_int, c_int, c_int64]),
    "ptv3_rows_linear": (c_int, [P, P, P, P, P, P, P, P, c_int, P, P, P, c_int64, c_int, c_int, c_float, c_int, P]),
    "ptv3_conv_head_halo_policy": (c_int, [c_int64, c_int, c_int]),
    "ptv3_conv_head_halo": (c_int, [P, P, P, c_int64, c_int, P, P, P, c_size_t, P, P, P, P, P, P, P, P, P, c_float, c_int, P]),
    "ptv3_block_head": (c_int, [P, P, c_int, P, P, P, P, P, P, P, P, P, P, c_int64, c_int, c_float, c_int, P]),
    "ptv3_block_tail": (c_int, [P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int, c_int, c_float, c_int, P]),
    "ptv3_block_tail_sliced_policy": (c_int, [c_int, c_int, c_int, c_int64]),
    "ptv3_block_tail_sliced_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "ptv3_block_tail_sliced": (c_int, [P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int, c_int, c_float, c_int, c_int, P,
                                       c_size_t, P]),
    "ptv3_rows_linear_ln_capable": (c_int, [c_int, c_int, c_int]),
    "ptv3_rows_linear_ln": (c_int, [P, P, P, P, P, P, c_int64, c_int, c_int, c_float, c_int, c_int, P]),
    "ptv3_subm_conv_ln_capable": (c_int, [c_int, c_int, c_int]),
    "ptv3_subm_conv_ln": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, c_int, c_float, c_int, c_int, P]),
    "ptv3_res_conv_capable": (c_int, [c_int64, c_int, c_int, c_int, c_int]),
    "ptv3_res_conv_row_tiles": (c_int, [c_int64, c_int]),
    "ptv3_res_conv": (c_int, [P, P, P, P, P, P, P, P, c_int, P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, P]),
    "ptv3_mlp2_fusable": (c_int, [c_int, c_int, c_int, c_int]),
    "ptv3_mlp2": (c_int, [P, P, P, P, P, c_int, P, P, P, c_int, c_int64, c_int, c_int, c_int, c_int, P]),
    "ptv3_layernorm": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, c_float, c_int, P]),
    "ptv3_layernorm_slabs": (c_int, [P, c_int, P, P, P, P, P, P, P, P, c_int64, c_int, c_float, c_int, P]),
    "ptv3_affine_act": (c_int, [P, P, P, c_int, P, c_int64, c_int, c_int, P]),
    "ptv3_cast": (c_int, [P, c_int, P, c_int, c_int64, P]),
    "ptv3_pool_workspace_bytes": (c_size_t, [c_int64]),
    "ptv3_pool_segments": (c_int, [P, P, c_int64, c_int, P, P, P, P, P, P, c_size_t, P]),
    "ptv3_pool_reduce": (c_int, [P, P, P, P, P, c_int, P, P, c_int64, c_int64, c_int, c_int, P, P, c_int, P, P, P,
                                 P, P, P, c_int, P]),
    "ptv3_forward_workspace_bytes": (c_size_t, [P, c_int64, c_int]),
    "ptv3_forward": (c_int, [P, P, c_int, P, P, c_size_t, P]),
    "ptv3_executor_create": (c_void_p, []),
    "ptv3_executor_destroy": (c_int, [P]),
    "ptv3_block_train_workspace_bytes": (c_size_t, [P, c_int]),
    "ptv3_block_train_fwd": (c_int, [P, P]),
    "ptv3_block_train_bwd": (c_int, [P, P]),
    "ptv3_gemm_tn_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "ptv3_gemm_tn": (c_int, [P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    "ptv3_col_reduce_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "ptv3_col_reduce": (c_int, [P, P, P, P, c_float, c_int, P, c_int64, c_int, c_int, P, c_size_t, P]),
    "ptv3_bn_finalize": (c_int, [P, P, c_int64, P, P, P, P, c_float, c_float, P, P, P, P, c_int, P]),
    "ptv3_bn_bwd_coeffs": (c_int, [P, c_int64, P, P, P, P, P, P, c_int, P]),
    "ptv3_layernorm_bwd": (c_int, [P, P, P, P, c_float, P, P, c_int64, c_int, c_int, P, c_size_t, P]),
    "ptv3_act_bwd": (c_int, [P, P, P, P, c_int, P, c_int64, c_int, c_int, P]),
    "ptv3_affine2": (c_int, [P, P, P, P, P, P, c_int64, c_int, c_int, P]),
    "ptv3_pool_max_bwd": (c_int, [P, P, P, P, c_int64, c_int, P, c_int, P]),
    "ptv3_segment_sum": (c_int, [P, P, P, c_int64, c_int, P, c_int, P]),
    "ptv3_window_attn_bwd_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int, c_int]),
    "ptv3_window_attn_bwd": (c_int, [P, P, P, P, P, P, c_int64, c_int64, c_int, c_int, c_int, c_float, c_int, P,
                                     c_size_t, P]),
    "ptv3_window_attn_varlen_bwd": (c_int, [P, P, P, P, P, P, c_int, P, c_int64, c_int64, c_int, c_int, c_int, c_float,
                                            c_int, P, c_size_t, P]),
    "ptv3_window_attn_train_fwd": (c_int, [P, P, P, P, c_int, P, P, c_int64, c_int64, c_int, c_int, c_int, c_float,
                                           c_double, c_int, P]),
    "ptv3_window_attn_train_bwd": (c_int, [P, P, P, P, P, P, P, c_int, P, c_int64, c_int64, c_int, c_int, c_int, c_float,
                                           c_int, P, c_size_t, P]),
    "ptv3_window_attn_drop_fwd": (c_int, [P, P, P, P, c_int, P, c_int64, c_int64, c_int, c_int, c_int, c_float, c_float,
                                          c_uint32, c_int, P]),
    "ptv3_window_attn_drop_bwd": (c_int, [P, P, P, P, P, P, c_int, P, c_int64, c_int64, c_int, c_int, c_int, c_float,
                                          c_float, c_uint32, c_int, P, c_size_t, P]),
    "ptv3_window_attn_rpe_bwd_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int, c_int, c_int, c_int]),
    "ptv3_window_attn_rpe_bwd": (c_int, [P, P, P, P, P, P, P, c_int, P, P, c_int64, c_int64, c_int, c_int, c_int,
                                         c_float, c_int, P, c_size_t, P]),
    "ptv3_adamw_entry_bytes": (c_size_t, []),
    "ptv3_adamw_chunk": (c_int, []),
    "ptv3_adamw_fill_entry": (c_int, [P, P, P, P, P, c_int64, c_int, c_int]),
    "ptv3_adamw_fill_shadow": (c_int, [P, P, P, c_int, c_int, c_int, c_int]),
    "ptv3_adamw_fill_step_lag": (c_int, [P, c_int64]),
    "ptv3_adamw_step": (c_int, [P, c_int, c_int, P, P, c_int, c_float, c_float, c_float, c_int64, c_float, P, P, c_int,
                                c_int, P]),
    "ptv3_adamw_shadow_tiles": (c_int, [c_int, c_int, c_int]),
    "ptv3_adamw_fill_first_tile": (c_int, [P, c_int]),
    "ptv3_grad_sqnorm": (c_int, [P, c_int, c_int, P, P, P, P, P]),
    "ptv3_grid_hash": (c_int, [P, c_int64, c_double, c_int, P, P, P, P]),
    "ptv3_keypoint_aggregate": (c_int, [P, P, P, c_int, c_int, P, P, c_int, c_float, P, P, P]),
    "ptv3_scene_mean_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "ptv3_scene_mean": (c_int, [P, P, c_int64, c_int, c_int, c_int, P, P, c_size_t, P]),
    "ptv3_scene_mean_head": (c_int, [P, P, c_int64, c_int, c_int, c_int, P, P, P, P, c_int, P, P, P, P, c_int, P, P,
                                     c_size_t, P]),
    "ptv3_scene_mean_bwd": (c_int, [P, P, c_int64, c_int, c_int, P, c_int, P]),
    "ptv3_cls_head_capable": (c_int, [c_int, c_int, c_int, c_int]),
    "ptv3_cls_head_eval": (c_int, [P, P, c_int64, c_int, c_int, c_int, P, P, P, P, c_int, P, P, P, P, c_int, P, P, c_int,
                                   P, c_float, c_float, P, P, P, c_size_t, P]),
    "ptv3_cls_head_save_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ptv3_cls_head_train_fwd": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P, c_float, P, c_float, c_float, P,
                                        P, P, P]),
    "ptv3_cls_head_train_bwd": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P, c_float, c_float, P, P, P, P,
                                        P]),
    "ptv3_scene_median_workspace_bytes": (c_size_t, [c_int, c_int]),
    "ptv3_scene_median": (c_int, [P, P, P, c_int64, c_int, c_int, P, P, c_size_t, P]),
    "ptv3_vote_loss_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "ptv3_vote_loss": (c_int, [P, P, P, c_int, P, P, c_int, c_int64, c_int, c_int, c_float, P, P, P, c_size_t, P]),
    "ptv3_vote_loss_bwd": (c_int, [P, P, P, P, c_int, P, P, c_int64, c_int, c_int, c_float, P, P]),
    "ptv3_profile_enable": (c_int, [c_int]),
    "ptv3_profile_collect": (c_int, [P, P, P, P]),
    "ptv3_profile_hint_flops": (c_int, [ctypes.c_double]),
    "ptv3_profile_kernel_count": (c_int, []),
    "ptv3_profile_kernel_name": (c_char_p, [c_int]),
    "ptv3_profile_collect_kernels": (c_int, [P, P, P, P]),
    "ptv3_swin_window_keys": (c_int, [P, c_int64, c_int, c_int, c_int, P, P, P]),
    "ptv3_swin_attn_fwd": (c_int, [P, P, P, P, P, P, P, c_int, P, P, c_int, P, P, c_int64, c_int, c_int, c_int, c_int, P]),
    "ptv3_swin_attn_bwd": (c_int, [P, P, P, P, P, P, P, P, c_int, P, P, c_int, P, P, P, P, P, P, P, c_int64, c_int, c_int,
                                   c_int, c_int, P]),
    "ptv3_knn_query": (c_int, [c_int, c_int, P, P, P, P, c_int, P, P, P]),
    "ptv3_knn_query_cells": (c_int, [c_int, c_int, P, P, P, P, c_int64, P, P, P, c_float, P, P, P]),
    "ptv3_grouping_forward": (c_int, [c_int, c_int, c_int, P, P, P, P]),
    "ptv3_grouping_backward": (c_int, [c_int, c_int, c_int, P, P, P, P]),
    "ptv3_interpolation_forward": (c_int, [c_int, c_int, c_int, P, P, P, P, P]),
    "ptv3_interpolation_backward": (c_int, [c_int, c_int, c_int, P, P, P, P, P]),
    "ptv3_farthest_point_sampling": (c_int, [c_int, c_int, P, P, P, P, P, P]),
    "ptv3_vector_attn_fwd": (c_int, [P, P, P, P, P, c_int64, c_int, c_int, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "ptv3_down2_keys": (c_int, [P, c_int64, c_int, c_int, c_int, c_int64, P, P, P]),
    "ptv3_down2_children": (c_int, [P, P, P, P, P, P, P, c_int64, c_int64, P, P, P, P, P, P]),
    "ptv3_down2_conv": (c_int, [P, P, P, c_int64, c_int64, c_int, c_int, P, P, c_int, P, P]),
    "ptv3_up2_conv": (c_int, [P, P, P, P, P, c_int64, c_int64, c_int, c_int, P, P, c_int, P, P]),
    "ptv3_cluster_keys": (c_int, [P, c_int64, P, c_int, P, P]),
    "ptv3_cluster_center": (c_int, [P, c_int64, P, P, P, c_int64, c_int, P, P]),
    "ptv3_cluster_softmax_sum": (c_int, [P, c_int64, P, c_int64, P, P, P, P, c_int64, c_int, P, P]),
    "ptv3_cluster_mix": (c_int, [P, c_int64, P, P, c_int, P, c_int64, c_int64, c_int, P, c_int64, c_int, P]),
    "ptv3_add_act": (c_int, [P, P, c_int, P, c_int64, P]),
    "ptv3_gva_fwd": (c_int, [P, P, P, P, P, c_int64, c_int, c_int, c_int, P, P, P, P, P, P, P, P, P, P, P, P]),
    "ptv3_grid_keys": (c_int, [P, c_int64, P, c_int, c_float, P, P, P, P, P]),
    "ptv3_segment_mean3": (c_int, [P, P, P, c_int64, P, P]),
    "ptv3_strat_cell_keys": (c_int, [P, c_int64, P, c_int, P, c_float, c_int, P, P, P, P]),
    "ptv3_strat_key_count": (c_int, [P, P, P, P, P, P, P, P, P, P, c_int64, P, P]),
    "ptv3_strat_key_fill": (c_int, [P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, P, P, P, P]),
    "ptv3_strat_rel_index": (c_int, [P, P, P, c_int64, c_float, c_float, c_int, P, P]),
    "ptv3_strat_attn_capable": (c_int, [c_int, c_int, c_int]),
    "ptv3_strat_attn_fwd": (c_int, [P, P, P, c_int64, P, P, P, P, P, P, P, P, c_int64, c_int, c_int, c_int, c_float,
                                    c_float, c_float, P, P]),
    "ptv3_ball_query": (c_int, [P, P, c_int, c_int64, c_float, c_int, P, P]),
    "ptv3_octree_keys": (c_int, [P, P, c_int, c_int64, c_float, c_int, P, P, P]),
    "ptv3_octree_attn_capable": (c_int, [c_int, c_int, c_int, c_int]),
    "ptv3_octree_attn_fwd": (c_int, [P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_int, c_float, P]),
    "ptv3_octree_dwconv": (c_int, [P, P, P, P, P, P, c_int64, c_int, P]),
    "ptv3_lovasz_scan_tile": (c_int, []),
    "ptv3_lovasz_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "ptv3_lovasz_fwd": (c_int, [P, P, c_int64, c_int, c_int64, c_float, P, P, P, P, P, c_size_t, P]),
    "ptv3_lovasz_bwd": (c_int, [P, P, P, P, P, c_int64, c_int, c_int64, c_float, P, P]),
    "ptv3_focal_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "ptv3_focal_fwd": (c_int, [P, P, P, c_int64, c_int, c_int64, c_float, c_float, c_int, P, P, P, c_size_t, P]),
    "ptv3_focal_bwd": (c_int, [P, P, P, P, P, c_int64, c_int, c_int64, c_float, c_float, c_int, P, P]),
    "ptv3_pg_workspace_bytes": (c_size_t, [c_int64]),
    "ptv3_pg_ballquery_batch_p": (c_int, [P, P, P, c_int, c_int64, c_float, P, P, P, P, c_size_t, P]),
    "ptv3_pg_cluster": (c_int, [P, P, P, c_int, c_int64, c_float, c_int, c_int, P, P, P, P, c_size_t, P]),
    "ptv3_pg_bfs_cluster_host": (c_int, [P, P, c_int64, P, c_int64, c_int, P, P, P]),
    "ptv3_pg_head_eval_capable": (c_int, [c_int, c_int]),
    "ptv3_pg_head_eval": (c_int, [P, P, c_int64, c_int, c_int, P, P, P, P, P, P, c_float, P, P, P, P, c_float, P, c_int,
                                  P, P, P, P, P, P, P]),
    "ptv3_pg_bias_loss_fwd": (c_int, [P, P, P, P, c_int64, c_int64, P, P]),
    "ptv3_pg_bias_loss_bwd": (c_int, [P, P, P, P, P, c_int64, c_int64, P, P, P]),
    "ptv3_pg_proposals": (c_int, [P, P, c_int, c_int64, P, c_int, P, P, c_int64, c_int64, c_int, c_int, P, P, P, P, P]),
    "ptv3_cac_capable": (c_int, [c_int, c_int]),
    "ptv3_cac_proto_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "ptv3_cac_proto_fwd": (c_int, [P, P, P, P, c_int, c_int64, c_int, c_int, c_float, P, P, P, P, c_size_t, P]),
    "ptv3_cac_proto_bwd": (c_int, [P, P, P, P, P, c_int, c_int64, c_int, c_int, c_float, P, P]),
    "ptv3_cac_cos_logits_fwd": (c_int, [P, P, P, c_int, c_int64, c_int, c_int, c_int, c_float, P, P]),
    "ptv3_cac_distill_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "ptv3_cac_distill_fwd": (c_int, [P, P, P, c_int64, c_int, P, P, P, P, c_size_t, P]),
    "ptv3_cac_distill_bwd": (c_int, [P, P, P, P, P, c_int64, c_int, P, P]),
    "ptv3_ppt_head_capable": (c_int, [c_int, c_int]),
    "ptv3_ppt_head_fwd": (c_int, [P, P, P, c_float, c_float, c_int64, c_int, c_int, P, P]),
    "ptv3_sonata_capable": (c_int, [c_int]),
    "ptv3_sonata_sk_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "ptv3_sonata_sk_pass": (c_int, [P, c_int, P, c_int, c_int64, c_int64, c_int, c_double, P, c_double, P, P, P, c_size_t,
                                    P]),
    "ptv3_sonata_ce_workspace_bytes": (c_size_t, [c_int64]),
    "ptv3_sonata_ce_fwd": (c_int, [P, c_int, P, c_int, c_int64, P, c_int, P, c_int, c_int64, c_int64, c_int, c_double,
                                   c_double, P, P, c_int, P, P, P, P, P, c_size_t, P]),
    "ptv3_sonata_ce_bwd": (c_int, [P, P, c_int, P, c_int, c_int64, P, c_int, P, c_int, c_int64, c_int64, c_int, c_double,
                                   c_double, P, P, P, P, c_int, P, P, P]),
}


class _Lib:
    """Lazy handle: importing the package on a box without the .so works, using an op does not."""

    def __init__(self):
        self._dll = None

    def load(self):
        if self._dll is None:
            path = library_path()
            if not os.path.exists(path):
                raise ImportError(
                    f"libptv3_hip.so not found at {path}: build it with `make -C pointcept-keypointdetection_amd` "
                    "(or __graft_entry__.build()); there is no CPU fallback for the PTv3 HIP path")
            dll = ctypes.CDLL(path)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(dll, name)
                fn.restype, fn.argtypes = res, args
            self._dll = dll
        return self._dll

    def __getattr__(self, name):
        return getattr(self.load(), name)

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed (code {rc}): {self.load().ptv3_last_error().decode()}")


lib = _Lib()
