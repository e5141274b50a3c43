"""ctypes binding of ``liblinkteller_hip.so`` (the C ABI declared in include/linkteller_hip.h).

There is deliberately no CPU fallback: every compute entry point of this package goes through
this library, and loading fails loudly if it has not been built (``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C linkteller_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblinkteller_hip.so")

LT_OK = 0
MODE_FULL, MODE_SPARSE, MODE_DELTA = 0, 1, 2
MODES = {"full": MODE_FULL, "sparse": MODE_SPARSE, "delta": MODE_DELTA}


class LinkTellerHipError(RuntimeError):
    """A negative lt_status came back across the C ABI (mapped to RuntimeError)."""


_lib = None

# name -> (restype, argtypes); must list every symbol include/linkteller_hip.h declares
SIGNATURES = {
    "lt_last_error": (C.c_char_p, []),
    "lt_abi_version": (C.c_int, []),
    "lt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "lt_set_tuning": (C.c_int, [C.c_char_p, C.c_longlong]),
    "lt_graph_create": (C.c_int, [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_void_p)]),
    "lt_graph_destroy": (C.c_int, [C.c_void_p]),
    "lt_graph_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                C.POINTER(C.c_int32)]),
    "lt_graph_records_host": (C.c_int, [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.POINTER(C.c_int64)]),
    "lt_graph_create_device": (C.c_int, [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_void_p)]),
    "lt_graph_table": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "lt_gemm_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                              C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lt_spmm_csr_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                                  C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_spmm_route": (C.c_int, [C.c_void_p, C.c_int32]),
    "lt_spmm_gather_ceiling_bytes": (C.c_size_t, [C.c_void_p]),
    "lt_spmm_gather_ceiling": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.c_int64, C.c_void_p]),
    "lt_gcn2_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lt_gcn2_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_baseline_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.POINTER(C.c_void_p)]),
    "lt_baseline_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_baseline_features_changed": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_baseline_feature_list_entries": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "lt_baseline_attach_s1": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_baseline_refresh_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lt_baseline_enable_fp64": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_baseline_attach_s1d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_baseline_refresh_rows_fp64": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lt_baseline_fp64_route": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "lt_baseline_fp64_arrays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32),
                                          C.c_void_p]),
    "lt_baseline_destroy": (C.c_int, [C.c_void_p]),
    "lt_baseline_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_influence_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lt_influence_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                    C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_influence_pairs_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32]),
    "lt_influence_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_graph_reached_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_baseline_form_rows_fp64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "lt_baseline_gather_rows_fp64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "lt_baseline_scatter_rows_fp64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "lt_influence_rows_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                        C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_influence_matrix_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                           C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t,
                                           C.c_void_p]),
    "lt_influence_step_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                         C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lt_host_landing_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "lt_host_landing_stats2": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "lt_influence_rows_vec": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                        C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_wide_combine": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_int32,
                                  C.c_int32, C.c_void_p]),
    "lt_baseline3_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.POINTER(C.c_void_p)]),
    "lt_baseline3_create_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.POINTER(C.c_void_p)]),
    "lt_baseline3_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_baseline3_features_changed": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_baseline3_destroy": (C.c_int, [C.c_void_p]),
    "lt_baseline3_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_influence3_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "lt_influence3_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_lapgraph_select": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.POINTER(C.c_double), C.c_void_p]),
    "lt_philox_cells_scan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "lt_lapgraph_philox_workspace": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "lt_lapgraph_philox": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_int64, C.c_double, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_edgerand_philox": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p]),
    "lt_sym_csr_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int64]),
    "lt_sym_csr_from_cells": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_normalize_csr": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "lt_top_pairs_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "lt_top_pairs_lower": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "lt_top_stream_create": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]),
    "lt_top_stream_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "lt_top_stream_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "lt_top_stream_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_top_stream_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_top_stream_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_top_stream_destroy": (C.c_int, [C.c_void_p]),
    "lt_pairs_present": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "lt_score_curve_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "lt_score_curve": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_corr_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "lt_corr_square": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_corr_pairs": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_corr_rows_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lt_corr_rows_prepare": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "lt_corr_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_sample_square_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lt_sample_square_labels": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_group_pairs_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "lt_group_pairs": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_upper_edge_count": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "lt_sample_balanced_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int64]),
    "lt_sample_balanced_philox": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_baseline3_enable_fp64": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_influence3_rows_mode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_influence3_pairs_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int64]),
    "lt_influence3_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_baseline2w_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lt_baseline2w_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_baseline2w_features_changed": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_baseline2w_destroy": (C.c_int, [C.c_void_p]),
    "lt_baseline2w_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_influence2w_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "lt_influence2w_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_influence2w_pairs_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int64]),
    "lt_influence2w_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_node_check": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lt_export_rows_f64": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_profile_calls": (C.c_int, [C.POINTER(C.c_int64)]),
    "lt_gcn2_trainer_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                         C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lt_gcn2_trainer_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "lt_gcn2_trainer_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_gcn2_trainer_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_gcn2_trainer_epoch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "lt_gcn2_trainer_destroy": (C.c_int, [C.c_void_p]),
    "lt_gcn3_trainer_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                         C.c_double, C.c_double, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lt_gcn3_trainer_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "lt_gcn3_trainer_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "lt_gcn3_trainer_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_gcn3_trainer_hidden": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_gcn3_trainer_epoch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "lt_gcn3_trainer_destroy": (C.c_int, [C.c_void_p]),
    "lt_adam_step": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                               C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "lt_eval_head_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lt_eval_head": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_size_t, C.c_void_p]),
    "lt_early_stop_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_early_stop_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lt_gcn2_trainer_attach_validation": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                                    C.c_int32, C.c_int32, C.c_void_p]),
    "lt_gcn2_trainer_run_validated": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_gcn2_trainer_val_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "lt_gcn2_trainer_restore_best": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_gcn2_trainer_val_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_gcn3_trainer_attach_validation": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                                    C.c_int32, C.c_int32, C.c_void_p]),
    "lt_gcn3_trainer_run_validated": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_gcn3_trainer_val_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "lt_gcn3_trainer_restore_best": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lt_gcn3_trainer_val_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_eval_head_rows_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lt_eval_head_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_gcn2_trainer_attach_validation_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                                         C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "lt_gcn3_trainer_attach_validation_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                                         C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "lt_gcn2_trainer_create_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                              C.c_double, C.c_double, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lt_gcn2_trainer_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_gcn2_trainer_hidden": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_gcn2_trainer_attach_validation_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                                         C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "lt_eval_head_wide_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lt_eval_head_wide": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lt_gcn3_trainer_create_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_void_p,
                                              C.POINTER(C.c_void_p)]),
    "lt_gcn3_trainer_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_gcn3_trainer_attach_validation_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                                         C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "lt_gcn2_trainer_set_train_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "lt_gcn3_trainer_set_train_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "lt_mlp_trainer_create": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                        C.c_double, C.c_double, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lt_mlp_trainer_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_mlp_trainer_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "lt_mlp_trainer_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_mlp_trainer_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_mlp_trainer_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "lt_mlp_trainer_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_mlp_trainer_destroy": (C.c_int, [C.c_void_p]),
    "lt_mlp_forward_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lt_mlp_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "lt_profile_enable": (C.c_int, [C.c_int]),
    "lt_profile_reset": (C.c_int, []),
    "lt_profile_summary": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
}
KERNEL_IDS = {"gemm": 0, "layer1": 1, "layer2": 2, "perturb": 3, "full_stageA": 4, "full_stageB": 5,
              "item_stageA": 6, "item_stageB": 7, "spmm": 8, "fp64_product": 9, "fp64_spmm": 10, "item_bits": 11,
              "select_hist": 12, "select_collect": 13, "metrics_sort": 14, "metrics_curve": 15}
ABI_VERSION = 5
# lt_normalize_csr: the `norm` values (include/linkteller_hip.h, lt_norm) by the names of graph._NORMALIZERS
NORM_CODES = {"FirstOrderGCN": 0, "BingGeNormAdj": 1, "NormAdj": 2, "AugRWalk": 3, "RWalk": 4, "AugNormAdj": 5}
# lt_graph_table: the `which` values (include/linkteller_hip.h, lt_graph_table_id) and the names of the scalar table's entries
GRAPH_TABLES = {"rowptr": (0, "i4"), "col": (1, "i4"), "val": (2, "f4"), "tptr": (3, "i4"), "trow": (4, "i4"), "tval": (5, "f4"),
                "tpos": (6, "i4"), "cv": (7, "i4"), "dl_meta": (8, "i4"), "dl_rec": (9, "i4"), "p_long_row": (10, "i4"),
                "p_long_segptr": (11, "i4"), "p_seg_long": (12, "i4"), "p_seg_begin": (13, "i4"), "q_long_row": (14, "i4"),
                "q_long_segptr": (15, "i4"), "q_seg_long": (16, "i4"), "q_seg_begin": (17, "i4"), "w_e0": (18, "i4"),
                "w_cnt": (19, "i4"), "w_dst": (20, "i4"), "scalars": (21, "f8")}
GRAPH_SCALARS = ("n", "nnz", "max_row_nnz", "max_col_nnz", "local_frac", "hot_frac", "p_n_long", "p_n_seg", "q_n_long", "q_n_seg",
                 "w_n", "dl_max_t", "dl_max_tu", "dl_touch_frac", "has_tpos", "has_cv", "has_records")


def lib():
    """The loaded library (loads on first use; raises if the shared object is missing)."""
    global _lib
    if _lib is None:
        # torch ships its own libamdhip64.so.7 / libhsa-runtime64.so.1; whichever copy is loaded
        # first serves the whole process.  Load torch's first so that this library, torch's
        # allocator and torch's streams all talk to ONE HIP runtime.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise LinkTellerHipError(
                f"{LIB_PATH} not found: the HIP extension is not built.  Build it with "
                f"`make -C {os.path.join(_HERE, 'csrc')}` (needs hipcc); there is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


LT_ERR_INDEX = -6
LT_ERR_WORKSPACE = -4
STEP_REFRESH, STEP_DST_PINNED = 1, 2      # lt_influence_step_host flags (LT_STEP_*)


def check(status: int, what: str = ""):
    if status != LT_OK:
        msg = lib().lt_last_error().decode("utf-8", "replace")
        if status == LT_ERR_INDEX:      # the reference raises IndexError at grad_mat[test_nodes[j]] (attacker.py:226-229)
            raise IndexError(f"{what or 'liblinkteller_hip'}: {msg}")
        raise LinkTellerHipError(f"{what or 'liblinkteller_hip'} failed with status {status}: {msg}")


TUNING_DEFAULT = -(1 << 63)


def set_tuning(key: str, value=None):
    """Route-selection knob of the library (include/linkteller_hip.h); ``None`` restores the default."""
    check(lib().lt_set_tuning(key.encode(), TUNING_DEFAULT if value is None else int(value)), "lt_set_tuning")


def device_count() -> int:
    n = C.c_int(0)
    check(lib().lt_device_count(C.byref(n)), "lt_device_count")
    return n.value


def require_gpu():
    """Fail loudly when there is nothing to run on (no silent eager/CPU path)."""
    import torch
    if not torch.cuda.is_available() or device_count() == 0:
        raise LinkTellerHipError("no HIP device visible: linkteller_amd runs its hot path only on an "
                                 "MI355X-class GPU through liblinkteller_hip.so (no CPU fallback)")
