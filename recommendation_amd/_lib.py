"""ctypes binding of libgcr.so — the C ABI declared in include/gcr.h.

This is the binding a maintainer of the reference would add.  There is no
CPU fallback: if the HIP library is missing or a call fails, the op raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p

import numpy as np
import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libgcr.so")

_P = c_void_p  # every device / host buffer crosses the ABI as a plain pointer
_Tensor = torch.Tensor

# name -> (restype, argtypes); mirrors include/gcr.h one to one
SIGNATURES = {
    "gcr_version": (c_int32, []),
    "gcr_arch": (c_char_p, []),
    "gcr_spmm_plan_size_host": (c_int32, [_P, c_int64, c_int32, _P, _P, _P]),
    "gcr_spmm_plan_fill_host": (c_int32, [_P, c_int64, c_int32, _P, _P, _P]),
    "gcr_spmm_plan_size_skip_host": (c_int32, [_P, c_int64, c_int32, _P, _P, _P, _P]),
    "gcr_spmm_plan_fill_skip_host": (c_int32, [_P, c_int64, c_int32, _P, _P, _P, _P]),
    "gcr_spmm_hub_reduce_f32": (c_int32, [_P, c_int64, c_int32, _P, c_int32, c_float, _P, _P, _P, c_float, c_int64, _P]),
    "gcr_spmm_hub_parts_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P, _P, _P, c_int32, _P, _P, c_int64, c_int64, _P]),
    "gcr_spmm_rows_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P, _P, c_float, _P, c_int32, _P, _P, _P, c_float, _P,
                                    c_int64, c_int64, _P]),
    "gcr_spmm_windowed_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P, _P, _P,
                                        _P, c_int64, _P, _P, c_int64, _P, _P, _P, _P, _P, c_int64, c_int32, _P,
                                        _P, c_int32, c_float, _P, _P, _P, c_float, c_int32, c_int64, c_int64, _P]),
    "gcr_spmm_rows_mapped_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P, _P, _P, c_float, _P, c_int32, _P, _P, _P,
                                           c_float, _P, c_int64, c_int64, _P]),
    "gcr_spmm_windowed_mapped_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P, _P, _P,
                                               _P, c_int64, _P, _P, c_int64, _P, _P, _P, _P, _P, _P, c_int64, c_int32, _P,
                                               _P, c_int32, c_float, _P, _P, _P, c_float, c_int32, c_int64, c_int64, _P]),
    "gcr_spmm_csr_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P, _P, _P, c_float, _P, c_int32,
                                   _P, _P, _P, c_float, c_uint32, _P, _P, c_int64, c_int64, _P]),
    "gcr_spmm_csr_acc2_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P, _P, _P, c_float, _P, c_int32,
                                        _P, _P, _P, c_float, _P, c_float, c_uint32, _P, _P, c_int64, c_int64, _P, _P]),
    "gcr_bitmap_set": (c_int32, [_P, c_int64, c_int64, _P, _P]),
    "gcr_spmm_csr_dual_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P, _P, _P, c_float, _P, c_int32,
                                        _P, _P, _P, _P, c_int64, c_int64, _P]),
    "gcr_spmm_csr_dual_acc_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, _P, _P, _P, _P, c_float, _P, c_int32,
                                            _P, _P, _P, _P, _P, _P, c_int64, c_int64, _P]),
    "gcr_csr_validate": (c_int32, [_P, _P, c_int64, c_int64, c_int64, _P, _P]),
    "gcr_bpr_workspace_floats": (c_int64, [c_int64]),
    "gcr_bpr_fwd_f32": (c_int32, [_P, _P, c_int32, _P, _P, _P, c_int64, c_int32, c_int32, c_int64, c_int64,
                                  _P, _P, _P, _P]),
    "gcr_bpr_bwd_f32": (c_int32, [_P, _P, c_int32, _P, _P, _P, c_int64, c_int32, c_int64, c_int64,
                                  _P, _P, _P, _P, _P]),
    "gcr_sort_index_workspace_bytes": (c_int64, [c_int64]),
    "gcr_sort_index": (c_int32, [_P, c_int64, c_int64, _P, _P, _P, _P]),
    "gcr_bpr_edge_values_f32": (c_int32, [_P, _P, _P, c_int64, c_int64, _P, _P, _P, _P]),
    "gcr_bpr_bwd_sorted_f32": (c_int32, [_P, _P, c_int32, _P, _P, _P, c_int64, c_int32, c_int64, c_int64, _P, _P,
                                         _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gcr_bpr_neg_block_f32": (c_int32, [_P, _P, _P, c_int64, c_int32, c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "gcr_sort_pairs_u64_workspace_bytes": (c_int64, [c_int64]),
    "gcr_sort_pairs_u64": (c_int32, [_P, _P, c_int64, c_int64, _P, _P, _P, _P]),
    "gcr_bpr_neg_items_sorted_f32": (c_int32, [_P, _P, c_int32, _P, _P, c_int64, c_int64, c_int64, _P, _P, _P]),
    "gcr_neg_sample": (c_int32, [_P, _P, _P, c_int64, c_int32, c_int64, c_int64, c_uint64, c_uint64, c_int32, _P, _P]),
    "gcr_edge_mask_bits": (c_int32, [c_int64, c_float, c_uint64, _P, _P, _P]),
    "gcr_row_inv_norm_f32": (c_int32, [_P, c_int64, c_int32, c_float, _P, _P]),
    "gcr_infonce_engine": (c_int32, [c_int32]),
    "gcr_infonce_fwd_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32]),
    "gcr_infonce_fwd_f32": (c_int32, [_P, _P, c_int64, _P, _P, c_int64, c_int32, c_float, _P, _P, c_float, _P, _P]),
    "gcr_infonce_fwd_ex_f32": (c_int32, [_P, _P, c_int64, _P, _P, c_int64, c_int32, c_float, _P, _P, c_float, _P, c_uint32, _P]),
    "gcr_infonce_fwd_o_supported": (c_int32, [c_int32, c_uint32]),
    "gcr_infonce_fwd_o_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32]),
    "gcr_infonce_fwd_o_f32": (c_int32, [_P, _P, c_int64, _P, _P, c_int64, c_int32, c_float, _P, _P, _P, c_uint32, _P]),
    "gcr_pos_logit_f32": (c_int32, [_P, _P, _P, _P, _P, c_int64, c_int64, c_int32, c_float, _P, _P]),
    "gcr_infonce_bwd_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32]),
    "gcr_infonce_bwd_f32": (c_int32, [_P, _P, c_int64, _P, _P, c_int64, c_int32, c_float, _P, _P, _P, _P, _P, _P, _P]),
    "gcr_infonce_bwd_ex_f32": (c_int32, [_P, _P, c_int64, _P, _P, c_int64, c_int32, c_float, _P, _P, _P, _P, _P, _P, c_uint32, _P]),
    "gcr_infonce_pos_bwd_f32": (c_int32, [_P, _P, _P, _P, _P, _P, c_int64, c_int64, c_int32, c_float, _P, _P, _P]),
    "gcr_normalize_bwd_f32": (c_int32, [_P, _P, _P, c_int64, c_int32, _P, _P]),
    "gcr_normalize_bwd_n_f32": (c_int32, [_P, _P, _P, _P, c_int64, c_int32, _P, _P]),
    "gcr_normalize_bwd_raw_f32": (c_int32, [_P, _P, _P, _P, c_int64, c_int32, _P, _P]),
    "gcr_gram_tn_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32]),
    "gcr_gram_tn_f32": (c_int32, [_P, _P, c_int64, c_int32, c_int32, _P, _P, _P]),
    "gcr_rows_dot_vec_f32": (c_int32, [_P, _P, c_int64, c_int32, _P, _P]),
    "gcr_weighted_colsum_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_weighted_colsum_f32": (c_int32, [_P, _P, c_int64, c_int32, _P, _P, _P]),
    "gcr_gate_fwd_f32": (c_int32, [_P, _P, _P, c_int64, c_int32, _P, _P]),
    "gcr_gate_bwd_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_gate_bwd_f32": (c_int32, [_P, _P, _P, _P, c_int64, c_int32, _P, _P, _P, _P, _P]),
    "gcr_channel_mix_supported": (c_int32, [c_int32]),
    "gcr_channel_mix_fwd_f32": (c_int32, [_P, _P, _P, _P, _P, c_float, c_int64, c_int32, _P, _P, _P]),
    "gcr_channel_mix_bwd_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_channel_mix_bwd_f32": (c_int32, [_P, _P, _P, _P, _P, _P, c_float, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "gcr_mim_supported": (c_int32, [c_int32]),
    "gcr_mim_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_mim_fwd_f32": (c_int32, [_P, _P, _P, _P, _P, c_int64, c_int32, _P, _P, _P, _P, _P]),
    "gcr_mim_bwd_f32": (c_int32, [_P, _P, _P, _P, _P, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "gcr_bce_fwd_o_supported": (c_int32, [c_int32, c_uint32]),
    "gcr_bce_fwd_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32]),
    "gcr_bce_fwd_f32": (c_int32, [_P, c_int64, _P, c_int64, c_int32, _P, _P, _P, c_uint32, _P]),
    "gcr_bce_bwd_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32]),
    "gcr_bce_bwd_f32": (c_int32, [_P, c_int64, _P, c_int64, c_int32, _P, _P, _P, _P, c_uint32, _P]),
    "gcr_kmeans_assign_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, c_int32, _P, _P, _P]),
    "gcr_kmeans_assign_accumulate_f32": (c_int32, [_P, c_int64, _P, _P, c_int64, c_int32, _P, _P, _P, c_int32, _P]),
    "gcr_kmeans_image_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_kmeans_centroid_image_f32": (c_int32, [_P, _P, c_int64, c_int32, _P, _P]),
    "gcr_kmeans_search_image_f32": (c_int32, [_P, c_int64, _P, c_int64, c_int32, _P, _P, _P, c_int32, c_uint32, _P]),
    "gcr_kmeans_search_image_incr_f32": (c_int32, [_P, c_int64, _P, c_int64, c_int32, _P, _P, _P, _P, c_int32, c_uint32, _P]),
    "gcr_kmeans_lloyd_update_q_f32": (c_int32, [_P, _P, _P, c_int64, c_int32, _P, _P, _P, c_int64, c_uint64, c_int32, _P, _P, c_int32,
                                                _P]),
    "gcr_kmeans_update_f32": (c_int32, [_P, c_int64, c_int32, _P, c_int64, _P, _P, _P, _P, _P]),
    "gcr_kmeans_update_sorted_f32": (c_int32, [_P, c_int64, c_int32, _P, _P, c_int64, _P, _P, _P, _P, _P]),
    "gcr_kmeans_lloyd_update_f32": (c_int32, [_P, c_int64, c_int32, _P, _P, _P, c_int64, _P, _P, _P, _P, c_int32, c_uint64,
                                              c_int32, _P, _P]),
    "gcr_score_rows_f32": (c_int32, [_P, _P, c_int64, c_int64, _P, c_int64, c_int32, _P, _P]),
    "gcr_topk_masked_f32": (c_int32, [_P, c_int64, c_int64, _P, c_int64, _P, _P, c_int32, _P, _P, _P]),
    "gcr_rank_fused_supported": (c_int32, [c_int64, c_int32, c_int32]),
    "gcr_rank_fused_workspace_bytes": (c_int64, [c_int64]),
    "gcr_rank_fused_f32": (c_int32, [_P, _P, c_int64, c_int64, _P, c_int64, c_int32, _P, _P, c_int32, _P, _P, _P, _P, _P]),
    "gcr_rank_metrics": (c_int32, [_P, c_int64, c_int32, _P, _P, _P, c_int32, _P, _P, _P, _P]),
    "gcr_coo_to_csr_workspace_bytes": (c_int64, [c_int64]),
    "gcr_coo_to_csr": (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gcr_csr_sym_norm_f32": (c_int32, [_P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, _P]),
    "gcr_csr_row_norm_f32": (c_int32, [_P, _P, _P, c_int64, _P, _P, _P]),
    "gcr_edge_mask_exact_workspace_bytes": (c_int64, [c_int64]),
    "gcr_edge_mask_exact_bits": (c_int32, [c_int64, c_int64, c_uint64, _P, _P, _P]),
    "gcr_adam_step_f32": (c_int32, [_P, _P, _P, _P, _P, _P, c_int64, c_float, c_double, c_double, c_float, c_float, c_int64,
                                    c_float, _P]),
    "gcr_adam_step_dev_f32": (c_int32, [_P, _P, _P, _P, _P, _P, c_int64, c_float, c_double, c_double, c_float, c_float, _P,
                                        c_float, _P]),
    "gcr_sgd_momentum_step_f32": (c_int32, [_P, _P, _P, c_int64, c_float, c_float, c_float, c_int32, _P]),
    "gcr_directau_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_directau_fwd_f32": (c_int32, [_P, _P, c_int32, _P, _P, _P, c_int64, c_int32, c_int64, c_int64, c_float,
                                       _P, _P, _P, _P, _P, _P]),
    "gcr_directau_bwd_f32": (c_int32, [_P, _P, c_int32, _P, _P, _P, c_int64, c_int32, c_int64, c_int64, c_float,
                                       _P, _P, _P, _P, _P, _P, _P]),
    "gcr_tri_supported": (c_int32, [c_int32, c_int32]),
    "gcr_tri_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32]),
    "gcr_tri_member_words": (c_int64, [c_int64]),
    "gcr_tri_fwd_f32": (c_int32, [_P, _P, _P, _P, c_int64, c_int32, _P, c_int64, c_int32, c_float, c_int32, _P, _P, _P, _P, _P,
                                  _P, _P]),
    "gcr_tri_bwd_f32": (c_int32, [_P, _P, _P, _P, c_int64, c_int32, _P, c_int64, c_int32, c_float, _P, _P, _P, _P, _P, _P, _P,
                                  _P, _P]),
    "gcr_buir_supported": (c_int32, [c_int32]),
    "gcr_buir_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_buir_fwd_f32": (c_int32, [_P, _P, _P, _P, c_int64, c_int64, c_int32, _P, _P, c_int64, _P, _P, _P, _P, _P]),
    "gcr_buir_bwd_f32": (c_int32, [_P, _P, _P, _P, c_int64, c_int64, c_int32, _P, _P, c_int64, _P, _P, _P, _P, _P, _P, _P, _P,
                                   _P, _P, _P, _P, _P, _P]),
    "gcr_ema_rows_f32": (c_int32, [_P, _P, _P, c_int64, c_int32, c_int64, c_double, _P, _P]),
    "gcr_col_stats_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_col_stats_f32": (c_int32, [_P, c_int64, c_int32, _P, _P, _P, _P]),
    "gcr_bt_supported": (c_int32, [c_int32]),
    "gcr_bt_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_bt_fwd_f32": (c_int32, [_P, _P, c_int64, c_int32, c_float, c_float, c_int32, _P, _P, _P, _P, _P]),
    "gcr_bt_bwd_f32": (c_int32, [_P, _P, c_int64, c_int32, c_float, c_float, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "gcr_diffuse_supported": (c_int32, [c_int32]),
    "gcr_diffuse_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "gcr_diffuse_fwd_f32": (c_int32, [_P, _P, _P, c_int64, _P, _P, _P, c_int32, _P, _P]),
    "gcr_diffuse_bwd_f32": (c_int32, [_P, _P, _P, c_int64, _P, _P, _P, _P, _P, c_int32, _P, _P, _P, _P, _P]),
    "gcr_gat_supported": (c_int32, [c_int32, c_int32]),
    "gcr_gat_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32, c_int32]),
    "gcr_gat_fwd_f32": (c_int32, [_P, _P, c_int64, _P, _P, _P, c_int32, c_int32, c_float, _P, c_float, _P, _P, _P, _P, _P]),
    "gcr_gat_bwd_f32": (c_int32, [_P, _P, _P, _P, _P, c_int64, _P, _P, _P, _P, _P, c_int32, c_int32, c_float, _P, c_float,
                                  _P, _P, _P, _P, _P]),
    "gcr_sage_supported": (c_int32, [c_int32, c_int32]),
    "gcr_sage_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32]),
    "gcr_sage_fwd_f32": (c_int32, [c_int64, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, _P, c_float, _P, _P, _P, _P]),
    "gcr_sage_bwd_f32": (c_int32, [c_int64, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, _P, c_float, _P, _P, _P,
                                   _P, _P, _P, _P]),
    "gcr_gin_supported": (c_int32, [c_int32, c_int32]),
    "gcr_gin_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32]),
    "gcr_gin_fwd_f32": (c_int32, [c_int64, _P, _P, _P, _P, _P, c_int32, c_int32, _P, c_float, _P, _P, _P]),
    "gcr_gin_bwd_f32": (c_int32, [c_int64, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_float, _P, _P, _P, _P, _P, _P, _P]),
    "gcr_mask_columns_f32":(c_int32, [_P, c_int64, c_int32, _P, _P, _P]),
    "gcr_spgemm_expand_f32": (c_int32, [_P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gcr_csr_lookup_f32": (c_int32, [_P, _P, c_int64, _P, _P, _P, _P, _P]),
    "gcr_gather_rows_f32": (c_int32, [_P, _P, c_int64, c_int32, c_int64, _P, _P]),
    "gcr_scatter_add_rows_f32": (c_int32, [_P, _P, c_int64, c_int32, c_int64, _P, _P]),
    "gcr_gather_dropout_f32": (c_int32, [_P, _P, c_int64, c_int32, c_int64, c_float, c_uint64, c_int32, _P, _P, _P]),
    "gcr_gather_dropout_bwd_f32": (c_int32, [_P, _P, c_int64, c_int32, c_int64, c_float, c_uint64, c_int32, _P, _P, _P]),
    "gcr_dense_ids_workspace_bytes": (c_int64, [c_int64]),
    "gcr_dense_ids_u64": (c_int32, [_P, c_int64, c_int32, _P, _P, _P, _P, _P]),
    "gcr_probe_copy_f32": (c_int32, [_P, _P, c_int64, _P]),
    "gcr_probe_read_f32": (c_int32, [_P, c_int64, _P, _P]),
    "gcr_probe_gather_rows_f32": (c_int32, [_P, c_int64, _P, c_int64, _P, _P]),
    "gcr_probe_policy_rows_f32": (c_int32, [_P, c_int64, _P, c_int64, _P, c_int64, _P, _P, c_uint32, _P]),
}

_lib = None
_exports = {}   # name -> (converter without a stream, converter with one, is the return a status code): `call`'s table

# int32 is libgcr's status code, except for these exports, whose int32 is the answer
INT32_ANSWERS = ("gcr_version", "gcr_infonce_engine", "gcr_infonce_fwd_o_supported", "gcr_channel_mix_supported",
                 "gcr_mim_supported", "gcr_bce_fwd_o_supported", "gcr_rank_fused_supported", "gcr_tri_supported",
                 "gcr_buir_supported", "gcr_bt_supported", "gcr_diffuse_supported", "gcr_gat_supported",
                 "gcr_sage_supported", "gcr_gin_supported")


class GcrError(RuntimeError):
    pass


def _converter(name, argtypes, with_stream):
    """One export's argument converter, `name(a0, a1, ...[, stream]) -> tuple`, as straight-line code generated from its
    argtypes when the library loads (the last slot is the stream's, passed through, when with_stream).  A loop over the
    kinds at every call does the same and costs about 1 us more on a 19-argument launch (EXPERIMENTS.md)."""
    n = len(argtypes) - with_stream
    names = [f"a{i}" for i in range(n)]
    src = [f"def {name}({', '.join(names + ['stream'] * with_stream)}):"]
    for i, a in enumerate(names):
        if argtypes[i] is _P:
            src += [f"    if {a} is not None:",
                    f"        if isinstance({a}, Tensor):",
                    f"            if not {a}.is_contiguous():",
                    "                raise GcrError('libgcr needs contiguous tensors')",
                    f"            {a} = {a}.data_ptr()",
                    "        else:",
                    f"            {a} = other_pointer('{name}', {i}, {a})"]
        else:
            src += [f"    if isinstance({a}, Tensor):",
                    f"        raise TypeError('{name}: argument {i} is a number, got a tensor')"]
    src.append(f"    return ({''.join(x + ', ' for x in names + ['stream'] * with_stream)})")
    scope = {"Tensor": torch.Tensor, "GcrError": GcrError, "other_pointer": _other_pointer}
    exec("\n".join(src), scope)
    return scope[name]


def _bind(handle, signatures):
    """Resolves every export and sets its ctypes prototype (from here on the handle holds the function as a plain
    attribute) and builds `call`'s table, once per load."""
    exports = {}
    for name, (res, args) in signatures.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
        plain = _converter(name, args, False)
        exports[name] = (plain, _converter(name, args, True) if args else plain, res is c_int32 and name not in INT32_ANSWERS)
    return exports


def lib():
    """Loads libgcr.so once; raises loudly when the HIP extension has not been built."""
    global _lib, _exports
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GcrError(
                f"{LIB_PATH} is missing: the HIP extension is not built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`); there is no CPU fallback")
        handle = ctypes.CDLL(LIB_PATH)
        _lib, _exports = handle, _bind(handle, SIGNATURES)
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        if rc <= -1000:
            raise GcrError(f"{what}: HIP runtime error {-(rc + 1000)}")
        raise GcrError(f"{what}: invalid or unsupported arguments (code {rc})")


def dptr(t):
    """Device (or host) pointer of a contiguous tensor, None -> NULL."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise GcrError("libgcr needs contiguous tensors")
    return c_void_p(t.data_ptr())


def _other_pointer(name, pos, a):
    """The pointer kinds `call` meets rarely: a C-contiguous numpy array as its host address (the _host planners), or a
    c_void_p as it is.  Anything else, a plain int included, is refused."""
    if isinstance(a, np.ndarray):
        if not a.flags.c_contiguous:
            raise GcrError("libgcr needs contiguous tensors")
        return a.ctypes.data
    if isinstance(a, c_void_p):
        return a
    raise TypeError(f"{name}: argument {pos} is a pointer (a tensor, a numpy array, a c_void_p or None), got {type(a).__name__}")


def call(name, *args, on=None):
    """The one way the package calls an export of libgcr.so: `name` with `args` converted by the kinds of SIGNATURES[name].

    A pointer slot takes a contiguous tensor (its data_ptr()), None (NULL), a C-contiguous numpy array (its host address) or
    a c_void_p, and refuses a plain int; a numeric slot takes Python and numpy scalars and refuses a tensor.  `on` names the
    stream, which every launch takes as its last argument: a tensor or a device stands for the current stream of that
    device, a pointer from `cur_stream` goes in as it is (loops fetch it once), None appends nothing (host planners, size
    and _supported queries).  A wrong argument count is the converter's own TypeError, before the function is entered.  A
    status return other than 0 raises GcrError under the export's name; any other return (sizes and INT32_ANSWERS) is handed
    back."""
    try:
        plain, streamed, status = _exports[name]
    except KeyError:
        lib()                                    # first call: load and bind (an unknown name is a KeyError again)
        plain, streamed, status = _exports[name]
    if on is None:
        conv = plain(*args)
    else:
        conv = streamed(*args, on if isinstance(on, c_void_p) else cur_stream(on.device if isinstance(on, _Tensor) else on))
    rc = getattr(_lib, name)(*conv)          # the attribute `_bind` resolved; a test may have put a spy in its place
    if status:
        if rc != 0:
            check(rc, name)
        return None
    return rc


def call_on(handle):
    """`call` for another handle than the package's own (the A/B tools time other builds of libgcr.so; a test binds a
    recording stand-in): the same conversions and the same reading of the return, over the exports of SIGNATURES that
    `handle` has.  `.has(name)` tells whether it has one; calling one it lacks is a KeyError."""
    exports = _bind(handle, {name: sig for name, sig in SIGNATURES.items() if hasattr(handle, name)})

    def call(name, *args, on=None):
        plain, streamed, status = exports[name]
        if on is None:
            conv = plain(*args)
        else:
            conv = streamed(*args, on if isinstance(on, c_void_p) else cur_stream(on.device if isinstance(on, _Tensor) else on))
        rc = getattr(handle, name)(*conv)
        if status:
            check(rc, name)
            return None
        return rc

    call.has = exports.__contains__
    return call


_SIZE_UNIT = {"_bytes": 1, "_floats": 4, "_words": 4}     # what a size export counts, by its name's ending


def workspace(query, *args, device, dtype=torch.float32):
    """The scratch buffer of an entry point: `query` names its size export (gcr_*_workspace_bytes, _workspace_floats or
    _words), called with `args`.  Returns an uninitialised `dtype` tensor on `device` of at least that size and at least one
    element, so that a query answering 0 (an empty or unsupported problem, which the entry point refuses itself) still
    yields a pointer."""
    unit = next(u for ending, u in _SIZE_UNIT.items() if query.endswith(ending))
    nbytes = int(call(query, *args)) * unit
    item = torch.empty((), dtype=dtype).element_size()
    return torch.empty(max(-(-nbytes // item), 1), dtype=dtype, device=device)


def cur_stream(device=None):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise GcrError("libgcr operates on HIP device tensors only (no CPU fallback)")
