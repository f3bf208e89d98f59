"""ctypes binding of the C-ABI (include/sim3opt.h) -- used by tests/ and bench.py.

This is plumbing, not the product: every call lands in libsim3opt.so (HIP, gfx950).
There is no Python/CPU fallback; a missing library raises at import of the symbol table
and a missing GPU makes `Graph.initialize()` raise Sim3OptError(SIM3OPT_ERR_NO_DEVICE).
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SIM3OPT_LIB: another build of the same library, e.g. the host-sanitizer build of scripts/host_asan_suite.sh or an
# experiment build, `python -m sim3opt_amd.build --flags "..." --out PATH`, which never writes the product library)
LIB_PATH = os.environ.get("SIM3OPT_LIB") or os.path.join(_HERE, "libsim3opt.so")

OK, ERR_ARG, ERR_STATE, ERR_NO_DEVICE, ERR_HIP, ERR_IO, ERR_COMM = 0, -1, -2, -3, -4, -5, -6
# robust kernels of an edge (include/sim3opt.h lists rho and rho' of each)
(KERNEL_NONE, KERNEL_HUBER, KERNEL_PSEUDO_HUBER, KERNEL_CAUCHY, KERNEL_GEMAN_MCCLURE, KERNEL_WELSCH, KERNEL_FAIR,
 KERNEL_TUKEY, KERNEL_SATURATED, KERNEL_DCS) = range(10)
KERNEL_NAMES = ("none", "huber", "pseudo_huber", "cauchy", "geman_mcclure", "welsch", "fair", "tukey", "saturated",
                "dcs")
# options.algorithm (g2o's OptimizationAlgorithmLevenberg / GaussNewton / Dogleg) and the dogleg step types
ALGORITHM_LM, ALGORITHM_GAUSS_NEWTON, ALGORITHM_DOGLEG = 0, 1, 2
STEP_UNDEFINED, STEP_SD, STEP_GN, STEP_DL = 0, 1, 2, 3
STEP_NAMES = ("undefined", "SD", "GN", "DL")


class Options(C.Structure):
    _fields_ = [
        ("tau", C.c_double),
        ("user_lambda_init", C.c_double),
        ("good_step_lower", C.c_double),
        ("good_step_upper", C.c_double),
        ("max_trials", C.c_int32),
        ("fd_delta", C.c_double),
        ("exp_eps", C.c_double),
        ("small_rot_half", C.c_int32),
        ("fix_small_angle_b", C.c_int32),
        ("dof_mask", C.c_int32),
        ("pcg_max_iters", C.c_int32),
        ("pcg_rel_tol", C.c_double),
        ("pcg_check_every", C.c_int32),
        ("pcg_graph", C.c_int32),
        ("preconditioner", C.c_int32),
        ("chain_segment", C.c_int32),
        ("device", C.c_int32),
        ("verbose", C.c_int32),
        ("time_kernels", C.c_int32),
        ("linear_solver", C.c_int32),
        ("amg_cycle", C.c_int32 * 4),
        ("amg_passes", C.c_int32 * 3),
        ("amg_additive", C.c_int32),
        ("amg_fp32", C.c_int32),
        ("amg_pivot", C.c_int32),
        ("amg_coarsest", C.c_int32),
        ("adaptive_prec", C.c_int32),
        ("row_order", C.c_int32),
        ("halo_exchange", C.c_int32),
        ("span_grid", C.c_int32),
        ("force_collectives", C.c_int32),
        ("amg_shard_rows", C.c_int32),
        ("amg_virtual_ranks", C.c_int32),
        ("pcg_batch", C.c_int32),
        ("amg_omega", C.c_double),
        ("amg_over", C.c_double * 2),
        ("direct_max_pairs", C.c_int64),
        ("debug_full_arrays", C.c_int32),
        ("jacobians", C.c_int32),
        ("algorithm", C.c_int32),
        ("dl_max_trials", C.c_int32),
        ("dl_delta_init", C.c_double),
        ("dl_lambda_init", C.c_double),
        ("dl_lambda_factor", C.c_double),
        ("cov_workspace_mb", C.c_double),
        ("cov_solver", C.c_int32),
        ("cov_rel_tol", C.c_double),
    ]


class IterStats(C.Structure):
    _fields_ = [
        ("chi2_before", C.c_double),
        ("chi2_after", C.c_double),
        ("lambda_", C.c_double),
        ("rho", C.c_double),
        ("trials", C.c_int32),
        ("pcg_iters", C.c_int32),
        ("pcg_rel_res", C.c_double),
        ("ms_linearize", C.c_double),
        ("ms_solve", C.c_double),
        ("ms_update", C.c_double),
        ("pcg_capped", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class TrustRegionStats(C.Structure):
    """sim3opt_tr_stats: one dogleg iteration."""
    _fields_ = [
        ("delta_before", C.c_double),
        ("delta_after", C.c_double),
        ("alpha", C.c_double),
        ("norm_sd", C.c_double),
        ("norm_gn", C.c_double),
        ("norm_dl", C.c_double),
        ("step", C.c_int32),
        ("was_pd", C.c_int32),
    ]


class BaOptions(C.Structure):
    """sim3opt_ba_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("huber_delta", C.c_double),
        ("pixel_noise", C.c_double),
        ("tau", C.c_double),
        ("user_lambda_init", C.c_double),
        ("max_trials", C.c_int32),
        ("pcg_max_iters", C.c_int32),
        ("pcg_rel_tol", C.c_double),
        ("linear_solver", C.c_int32),
        ("device", C.c_int32),
        ("verbose", C.c_int32),
    ]


class BaBatchOptions(C.Structure):
    """sim3opt_ba_batch_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("huber_delta", C.c_double),
        ("pixel_noise", C.c_double),
        ("tau", C.c_double),
        ("user_lambda_init", C.c_double),
        ("outlier_chi2", C.c_double),
        ("max_iters", C.c_int32),
        ("max_trials", C.c_int32),
        ("device", C.c_int32),
    ]


class PnpBatchOptions(C.Structure):
    """sim3opt_pnp_batch_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("reproj_error", C.c_double),
        ("tau", C.c_double),
        ("seed", C.c_uint64),
        ("iterations", C.c_int32),
        ("min_inliers", C.c_int32),
        ("min_points", C.c_int32),
        ("refine_iters", C.c_int32),
        ("max_trials", C.c_int32),
        ("device", C.c_int32),
    ]


class EssentialBatchOptions(C.Structure):
    """sim3opt_essential_batch_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("threshold", C.c_double),
        ("distance_threshold", C.c_double),
        ("seed", C.c_uint64),
        ("iterations", C.c_int32),
        ("min_points", C.c_int32),
        ("device", C.c_int32),
    ]


class HomographyBatchOptions(C.Structure):
    """sim3opt_homography_batch_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("max_pixel_error", C.c_double),
        ("seed", C.c_uint64),
        ("iterations", C.c_int32),
        ("refine_rounds", C.c_int32),
        ("min_points", C.c_int32),
        ("device", C.c_int32),
    ]


class Sim3BatchOptions(C.Structure):
    """sim3opt_sim3_batch_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("max_pixel_error", C.c_double),
        ("huber_delta", C.c_double),
        ("pixel_noise", C.c_double),
        ("min_triangle_sin2", C.c_double),
        ("tau", C.c_double),
        ("seed", C.c_uint64),
        ("iterations", C.c_int32),
        ("min_points", C.c_int32),
        ("min_inliers", C.c_int32),
        ("refine_iters", C.c_int32),
        ("max_trials", C.c_int32),
        ("device", C.c_int32),
    ]


class MatchBatchOptions(C.Structure):
    """sim3opt_match_batch_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("ratio", C.c_double),
        ("border_ratio", C.c_double),
        ("skew_x", C.c_double),
        ("skew_y", C.c_double),
        ("knn_k", C.c_int32),
        ("device", C.c_int32),
    ]


class PlaceBatchOptions(C.Structure):
    """sim3opt_place_batch_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("alpha", C.c_double),
        ("min_nss_factor", C.c_double),
        ("use_nss", C.c_int32),
        ("k", C.c_int32),
        ("dislocal", C.c_int32),
        ("max_db_results", C.c_int32),
        ("max_intragroup_gap", C.c_int32),
        ("min_matches_per_group", C.c_int32),
        ("max_distance_between_queries", C.c_int32),
        ("max_distance_between_groups", C.c_int32),
        ("accumulate", C.c_int32),
        ("device", C.c_int32),
    ]


class VocabularyOptions(C.Structure):
    """sim3opt_vocabulary_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("seed", C.c_uint64),
        ("k", C.c_int32),
        ("levels", C.c_int32),
        ("max_iters", C.c_int32),
        ("idf", C.c_int32),
        ("device", C.c_int32),
    ]


class SurfBatchOptions(C.Structure):
    """sim3opt_surf_batch_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("hessian_threshold", C.c_double),
        ("n_octaves", C.c_int32),
        ("n_octave_layers", C.c_int32),
        ("upright", C.c_int32),
        ("max_keypoints", C.c_int32),
        ("images_per_pass", C.c_int32),
        ("device", C.c_int32),
    ]


class FrameStoreOptions(C.Structure):
    """sim3opt_frames_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("device", C.c_int32),
    ]


class TrackBatchOptions(C.Structure):
    """sim3opt_track_batch_options (include/sim3opt.h), field for field."""
    _fields_ = [
        ("max_reproj_px", C.c_double),
        ("max_rounds", C.c_int32),
        ("device", C.c_int32),
    ]


class KernelTimes(C.Structure):
    _fields_ = [
        ("ms_spmv", C.c_double), ("n_spmv", C.c_int64),
        ("ms_pcg_vec", C.c_double), ("n_pcg_vec", C.c_int64),
        ("ms_linearize", C.c_double), ("n_linearize", C.c_int64),
        ("ms_chi2", C.c_double), ("n_chi2", C.c_int64),
        ("ms_update", C.c_double), ("n_update", C.c_int64),
        ("ms_replicated_levels", C.c_double), ("n_replicated_visits", C.c_int64),
        ("n_batches", C.c_int64), ("n_batched_solves", C.c_int64),
    ]


class CommTimes(C.Structure):
    _fields_ = [
        ("ms_allreduce", C.c_double), ("n_allreduce", C.c_int64), ("bytes_allreduce", C.c_int64),
        ("ms_allgather", C.c_double), ("n_allgather", C.c_int64), ("bytes_allgather", C.c_int64),
        ("ms_exchange", C.c_double), ("n_exchange", C.c_int64), ("bytes_exchange", C.c_int64),
    ]


# every symbol include/sim3opt.h declares, with its signature
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint8)
_fp = C.POINTER(C.c_float)
_vp = C.c_void_p
SYMBOLS = {
    "sim3opt_version": (C.c_int, []),
    "sim3opt_options_default": (None, [C.POINTER(Options)]),
    "sim3opt_create": (_vp, []),
    "sim3opt_destroy": (None, [_vp]),
    "sim3opt_set_options": (C.c_int, [_vp, C.POINTER(Options)]),
    "sim3opt_get_options": (C.c_int, [_vp, C.POINTER(Options)]),
    "sim3opt_last_error": (C.c_char_p, [_vp]),
    "sim3opt_add_vertex": (C.c_int, [_vp, C.c_int32, _dp, C.c_int32]),
    "sim3opt_add_vertices": (C.c_int, [_vp, C.c_int32, _ip, _dp, _up]),
    "sim3opt_add_edge": (C.c_int, [_vp, C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_double]),
    "sim3opt_add_edges": (C.c_int, [_vp, C.c_int32, _ip, _ip, _dp, _dp, C.c_int32, C.c_double]),
    "sim3opt_set_edge_kernels": (C.c_int, [_vp, C.c_int32, _ip, _ip, _dp]),
    "sim3opt_get_edge_kernels": (C.c_int, [_vp, _ip, _dp]),
    "sim3opt_robustify": (C.c_int, [C.c_int32, C.c_double, C.c_double, _dp]),
    "sim3opt_edge_chi2": (C.c_int, [_vp, _dp, _dp, _dp]),
    "sim3opt_num_vertices": (C.c_int32, [_vp]),
    "sim3opt_num_edges": (C.c_int32, [_vp]),
    "sim3opt_get_edge": (C.c_int, [_vp, C.c_int32, _ip, _ip, _dp]),
    "sim3opt_initialize": (C.c_int, [_vp]),
    "sim3opt_optimize": (C.c_int, [_vp, C.c_int32]),
    "sim3opt_get_vertex": (C.c_int, [_vp, C.c_int32, _dp]),
    "sim3opt_set_vertex": (C.c_int, [_vp, C.c_int32, _dp]),
    "sim3opt_get_vertices": (C.c_int, [_vp, _dp]),
    "sim3opt_set_vertices": (C.c_int, [_vp, _dp]),
    "sim3opt_chi2": (C.c_int, [_vp, _dp]),
    "sim3opt_num_iterations": (C.c_int32, [_vp]),
    "sim3opt_get_stats": (C.c_int, [_vp, C.c_int32, C.POINTER(IterStats)]),
    "sim3opt_get_comm_times": (C.c_int, [_vp, C.POINTER(CommTimes)]),
    "sim3opt_get_kernel_times": (C.c_int, [_vp, C.POINTER(KernelTimes)]),
    "sim3opt_reset_kernel_times": (C.c_int, [_vp]),
    "sim3opt_pcg_schedule_stats": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_int32]),
    "sim3opt_edge_errors": (C.c_int, [_vp, _dp]),
    "sim3opt_get_trust_region_stats": (C.c_int, [_vp, C.c_int32, C.POINTER(TrustRegionStats)]),
    "sim3opt_edge_jacobians": (C.c_int, [_vp, _dp, _dp]),
    "sim3opt_sim3_edge_jacobian": (C.c_int, [_dp, _dp, _dp, C.POINTER(Options), _dp, _dp]),
    "sim3opt_linearize": (C.c_int, [_vp]),
    "sim3opt_debug_linearization_dims": (C.c_int, [_vp, _ip, _ip]),
    "sim3opt_debug_linearization": (C.c_int, [_vp, _dp, _dp, _ip, _dp, _ip, _ip, _ip, _ip, _ip, _dp, _dp]),
    "sim3opt_debug_update": (C.c_int, [_vp, _dp, C.c_double, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "sim3opt_debug_dogleg": (C.c_int, [_vp, _dp, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                       _dp, _dp, _dp]),
    "sim3opt_dogleg_rule": (C.c_int, [_dp, C.c_double, _dp, _dp, _ip]),
    "sim3opt_debug_column_vectors": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64),
                                               C.c_int32, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, _ip, C.c_int32,
                                               _dp]),
    "sim3opt_debug_factor_dims": (C.c_int, [_vp, C.c_int32, _ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sim3opt_debug_factor": (C.c_int, [_vp, C.c_int32, C.c_double, _dp, _dp, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp,
                                       _dp, _dp, _dp, _ip, _dp, _ip, _ip, _ip]),
    "sim3opt_system_dims": (C.c_int, [_vp, _ip, C.POINTER(C.c_int64)]),
    "sim3opt_system_pattern": (C.c_int, [_vp, _ip, C.POINTER(C.c_int64), _ip, _ip]),
    "sim3opt_get_system": (C.c_int, [_vp, _ip, _ip, _dp, _dp]),
    "sim3opt_solve": (C.c_int, [_vp, C.c_double, _dp, _ip, _dp]),
    "sim3opt_bench_spmv": (C.c_int, [_vp, C.c_int32, _dp]),
    "sim3opt_bench_stream": (C.c_int, [_vp, C.c_int32, C.c_int32, _dp]),
    "sim3opt_preconditioner_in_use": (C.c_int, [_vp]),
    "sim3opt_amg_hierarchy": (C.c_int, [_vp, C.c_int32, _ip, _ip, _vp, _ip]),
    "sim3opt_amg_level_structure": (C.c_int, [_vp, C.c_int32, _ip, _ip, C.POINTER(C.c_int64), _ip, _ip, _ip]),
    "sim3opt_amg_level_numbers": (C.c_int, [_vp, C.c_double, C.c_int32, _ip, _ip, _dp, C.POINTER(C.c_float), _dp,
                                            _dp, _dp, _dp]),
    "sim3opt_amg_coarsest_inverse": (C.c_int, [_vp, C.c_double, _dp]),
    "sim3opt_preconditioner_apply": (C.c_int, [_vp, C.c_int32, C.c_double, C.c_int32, _dp, _dp]),
    "sim3opt_spmv_spans": (C.c_int, [_vp, _ip, _ip]),
    "sim3opt_spmv_variant": (C.c_int, [_vp, _ip, _ip]),
    "sim3opt_operator_apply": (C.c_int, [_vp, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp]),
    "sim3opt_linear_solver_in_use": (C.c_int, [_vp]),
    "sim3opt_direct_plan": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int64), _ip, _ip, _ip, _ip, _ip, _ip,
                                      _ip, _ip, _ip, _ip, _ip, _ip]),
    "sim3opt_marginals": (C.c_int, [_vp, C.c_double, C.c_int32, _ip, _ip, _dp]),
    "sim3opt_marginal_covariances": (C.c_int, [_vp, C.c_double, _dp]),
    "sim3opt_covariances": (C.c_int, [_vp, C.c_double, C.c_int32, _ip, _ip, _dp]),
    "sim3opt_covariance_stats": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "sim3opt_gate_edges": (C.c_int, [_vp, C.c_double, C.c_int32, _ip, _ip, _dp, _dp, _dp, _dp, _dp]),
    "sim3opt_covariance_columns_plan": (C.c_int, [_vp, C.c_int32, _ip, _ip, _ip, _ip]),
    "sim3opt_covariance_columns_stats": (C.c_int, [_vp, C.POINTER(C.c_int64), _dp]),
    "sim3opt_marginal_plan": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int64), _ip, _ip, _ip, _ip, _ip, _ip,
                                        _ip, _ip, _ip]),
    "sim3opt_comm_allgather_plan": (C.c_int, [C.c_int32, C.c_int32, _ip, C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64)]),
    "sim3opt_comm_unique_id": (C.c_int, [_up]),
    "sim3opt_comm_init": (C.c_int, [_vp, C.c_int32, C.c_int32, _up]),
    "sim3opt_comm_init_callbacks": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "sim3opt_comm_set_alltoallv": (C.c_int, [_vp, _vp]),
    "sim3opt_amg_in_use": (C.c_int, [_vp, _ip, _ip, _ip]),
    "sim3opt_device_bytes": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "sim3opt_halo_plan": (C.c_int, [_vp, C.c_int32, C.c_int32, _ip, _ip, _ip, _ip, _ip, _ip]),
    "sim3opt_local_rows": (C.c_int, [_vp, _ip, _ip]),
    "sim3opt_set_devices": (C.c_int, [_vp, C.c_int32, _ip, C.c_double]),
    "sim3opt_rank_count": (C.c_int, [_vp]),
    "sim3opt_local_rows_of_rank": (C.c_int, [_vp, C.c_int32, _ip, _ip]),
    "sim3opt_device_bytes_of_rank": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int64)]),
    "sim3opt_comm_apply_allreduce": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int32, _dp, _dp]),
    "sim3opt_comm_apply_allgatherv": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_int32, _dp, _dp]),
    "sim3opt_comm_apply_exchange": (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int32,
                                              _dp, _dp]),
    "sim3opt_comm_local_state": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "sim3opt_partition_plan": (C.c_int, [_vp, C.c_int32, C.c_int32, _ip, _ip, _ip, C.POINTER(C.c_int64)]),
    "sim3opt_partition_rows": (C.c_int, [C.c_int32, _ip, C.c_int32, _ip]),
    "sim3opt_partition_rows_equal": (C.c_int, [C.c_int32, C.c_int32, _ip]),
    "sim3opt_load_kitti_direct": (C.c_int, [_vp, C.c_char_p, C.c_int32]),
    "sim3opt_load_kitti_gt_loops": (C.c_int, [_vp, C.c_char_p]),
    "sim3opt_release_device_cache": (None, []),
    "sim3opt_device_memory_in_use": (None, [C.POINTER(C.c_int64)]),
    "sim3opt_debug_device_memory": (None, [C.c_int32]),
    "sim3opt_debug_device_memory_report": (None, [C.POINTER(C.c_int64)]),
    "sim3opt_debug_device_memory_probe": (C.c_int64, [C.c_int64, C.c_int32, C.c_int64, C.POINTER(C.c_ubyte), C.c_int64]),
    "sim3opt_write_poses": (C.c_int, [_vp, C.c_char_p, _ip]),
    "sim3opt_stepwise_scale_init": (C.c_int, [_vp, _dp]),
    "sim3opt_read_keyframe_bin": (C.c_int, [C.c_char_p, _ip, _dp, _dp, _ip, C.POINTER(C.c_uint32), _dp,
                                            _dp, C.c_int32]),
    "sim3opt_reanchor_points": (C.c_int, [C.c_int32, _dp, _dp, C.c_int32, _dp, C.c_int32, _ip, _ip,
                                          C.c_int32]),
    "sim3opt_write_g2o": (C.c_int, [_vp, C.c_char_p]),
    "sim3opt_write_bal": (C.c_int, [C.c_char_p, C.c_int32, _dp, _dp, _dp, C.c_int32, _dp, C.c_int32, _ip, _ip, _dp]),
    "sim3opt_align_trajectory": (C.c_int, [C.c_int32, _dp, _dp, C.c_int32, _dp, _dp, _dp]),
    "sim3opt_ba_options_default": (None, [C.POINTER(BaOptions)]),
    "sim3opt_ba_create": (_vp, []),
    "sim3opt_ba_destroy": (None, [_vp]),
    "sim3opt_ba_last_error": (C.c_char_p, [_vp]),
    "sim3opt_ba_set_options": (C.c_int, [_vp, C.POINTER(BaOptions)]),
    "sim3opt_ba_set_problem": (C.c_int, [_vp, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _ip, _ip, _dp,
                                         C.c_double, C.c_double, C.c_double]),
    "sim3opt_ba_set_fixed_cameras": (C.c_int, [_vp, _up]),
    "sim3opt_ba_read_bal": (C.c_int, [_vp, C.c_char_p, C.c_double, C.c_double, C.c_double]),
    "sim3opt_ba_dims": (C.c_int, [_vp, _ip, _ip, _ip]),
    "sim3opt_ba_chi2": (C.c_int, [_vp, _dp]),
    "sim3opt_ba_optimize": (C.c_int, [_vp, C.c_int32]),
    "sim3opt_ba_get_cameras": (C.c_int, [_vp, _dp]),
    "sim3opt_ba_get_points": (C.c_int, [_vp, _dp]),
    "sim3opt_ba_num_iterations": (C.c_int32, [_vp]),
    "sim3opt_ba_get_stats": (C.c_int, [_vp, C.c_int32, C.POINTER(IterStats)]),
    "sim3opt_ba_write_poses": (C.c_int, [_vp, C.c_char_p]),
    "sim3opt_ba_debug_pattern": (C.c_int, [_vp, _ip, _ip, _ip]),
    "sim3opt_ba_debug_linearization": (C.c_int, [_vp, _dp]),
    "sim3opt_ba_debug_reduced": (C.c_int, [_vp, C.c_double] + [_dp] * 9),
    "sim3opt_ba_debug_step": (C.c_int, [_vp, C.c_double, C.c_int32, C.c_int32, C.c_double, _dp, _dp, _ip, _dp, _ip]),
    "sim3opt_ba_debug_update": (C.c_int, [_vp, _dp, _dp, C.c_double, C.c_int32, _dp, _dp, _dp, _dp]),
    "sim3opt_ba_covariances": (C.c_int, [_vp, C.c_double, C.c_int32, _ip, _ip, _dp, C.c_int32, _ip, _dp, C.c_int32, _ip,
                                         _ip, _dp]),
    "sim3opt_ba_covariance_stats": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "sim3opt_ba_covariance_plan": (C.c_int, [_vp, _ip, C.POINTER(C.c_int64), _ip, _ip, _ip, _ip]),
    "sim3opt_ba_batch_options_default": (None, [C.POINTER(BaBatchOptions)]),
    "sim3opt_ba_batch_create": (_vp, []),
    "sim3opt_ba_batch_destroy": (None, [_vp]),
    "sim3opt_ba_batch_last_error": (C.c_char_p, [_vp]),
    "sim3opt_ba_batch_set_options": (C.c_int, [_vp, C.POINTER(BaBatchOptions)]),
    "sim3opt_ba_batch_set_problems": (C.c_int, [_vp, C.c_int32, _ip, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_double,
                                                C.c_double]),
    "sim3opt_ba_batch_dims": (C.c_int, [_vp, _ip, _ip]),
    "sim3opt_ba_batch_optimize": (C.c_int, [_vp]),
    "sim3opt_ba_batch_debug_trial": (C.c_int, [_vp, _dp, _dp, _dp, _dp]),
    "sim3opt_ba_batch_get_cameras": (C.c_int, [_vp, _dp, _dp]),
    "sim3opt_ba_batch_get_points": (C.c_int, [_vp, _dp]),
    "sim3opt_ba_batch_num_iterations": (C.c_int32, [_vp, C.c_int32]),
    "sim3opt_ba_batch_get_stats": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(IterStats)]),
    "sim3opt_ba_batch_get_lambda_init": (C.c_int, [_vp, _dp]),
    "sim3opt_ba_batch_get_chi2": (C.c_int, [_vp, _dp, _dp, _dp, _ip]),
    "sim3opt_pnp_batch_options_default": (None, [C.POINTER(PnpBatchOptions)]),
    "sim3opt_pnp_batch_create": (_vp, []),
    "sim3opt_pnp_batch_destroy": (None, [_vp]),
    "sim3opt_pnp_batch_last_error": (C.c_char_p, [_vp]),
    "sim3opt_pnp_batch_set_options": (C.c_int, [_vp, C.POINTER(PnpBatchOptions)]),
    "sim3opt_pnp_batch_set_problems": (C.c_int, [_vp, C.c_int32, _ip, _dp, _dp, C.c_double, C.c_double, C.c_double]),
    "sim3opt_pnp_batch_dims": (C.c_int, [_vp, _ip, _ip]),
    "sim3opt_pnp_batch_solve": (C.c_int, [_vp]),
    "sim3opt_pnp_batch_get_poses": (C.c_int, [_vp, _dp]),
    "sim3opt_pnp_batch_get_inliers": (C.c_int, [_vp, _up, _ip]),
    "sim3opt_pnp_batch_get_summary": (C.c_int, [_vp, _ip, _ip, _ip, _dp, _dp, _ip]),
    "sim3opt_pnp_batch_debug_hypotheses": (C.c_int, [_vp, C.c_int32, _ip, _ip, _ip, _dp, _ip, _dp]),
    "sim3opt_pnp_batch_debug_score": (C.c_int, [_vp, C.c_int32, _dp, _ip, _dp]),
    "sim3opt_pnp_batch_debug_refine": (C.c_int, [_vp, _dp, _up, _dp, _ip, _dp, _ip]),
    "sim3opt_essential_batch_options_default": (None, [C.POINTER(EssentialBatchOptions)]),
    "sim3opt_essential_batch_create": (_vp, []),
    "sim3opt_essential_batch_destroy": (None, [_vp]),
    "sim3opt_essential_batch_last_error": (C.c_char_p, [_vp]),
    "sim3opt_essential_batch_set_options": (C.c_int, [_vp, C.POINTER(EssentialBatchOptions)]),
    "sim3opt_essential_batch_set_problems": (C.c_int, [_vp, C.c_int32, _ip, _dp, _dp, C.c_double, C.c_double,
                                                       C.c_double]),
    "sim3opt_essential_batch_dims": (C.c_int, [_vp, _ip, _ip, _ip]),
    "sim3opt_essential_batch_solve": (C.c_int, [_vp]),
    "sim3opt_essential_batch_get_poses": (C.c_int, [_vp, _dp]),
    "sim3opt_essential_batch_get_essentials": (C.c_int, [_vp, _dp]),
    "sim3opt_essential_batch_get_inliers": (C.c_int, [_vp, _up, _ip]),
    "sim3opt_essential_batch_get_summary": (C.c_int, [_vp, _ip, _ip, _ip, _dp, _ip, _ip, _ip]),
    "sim3opt_essential_batch_debug_hypotheses": (C.c_int, [_vp, C.c_int32, _ip, _ip, _ip, _dp, _ip, _dp]),
    "sim3opt_essential_batch_debug_score": (C.c_int, [_vp, C.c_int32, _dp, _ip, _dp]),
    "sim3opt_essential_batch_debug_pose": (C.c_int, [_vp, _dp, _up, _dp, _ip, _ip, _up]),
    "sim3opt_homography_batch_options_default": (None, [C.POINTER(HomographyBatchOptions)]),
    "sim3opt_homography_batch_create": (_vp, []),
    "sim3opt_homography_batch_destroy": (None, [_vp]),
    "sim3opt_homography_batch_last_error": (C.c_char_p, [_vp]),
    "sim3opt_homography_batch_set_options": (C.c_int, [_vp, C.POINTER(HomographyBatchOptions)]),
    "sim3opt_homography_batch_set_problems": (C.c_int, [_vp, C.c_int32, _ip, _dp, _dp, C.c_double, C.c_double,
                                                        C.c_double]),
    "sim3opt_homography_batch_dims": (C.c_int, [_vp, _ip, _ip, _ip]),
    "sim3opt_homography_batch_solve": (C.c_int, [_vp]),
    "sim3opt_homography_batch_get_poses": (C.c_int, [_vp, _dp]),
    "sim3opt_homography_batch_get_homographies": (C.c_int, [_vp, _dp, _dp]),
    "sim3opt_homography_batch_get_inliers": (C.c_int, [_vp, _up, _ip]),
    "sim3opt_homography_batch_get_summary": (C.c_int, [_vp, _ip, _ip, _dp, _ip, _dp, _ip, _ip, _ip, _ip, _ip, _dp]),
    "sim3opt_homography_batch_debug_hypotheses": (C.c_int, [_vp, C.c_int32, _ip, _ip, _ip, _dp, _ip, _dp]),
    "sim3opt_homography_batch_debug_score": (C.c_int, [_vp, C.c_int32, _dp, _ip, _dp]),
    "sim3opt_homography_batch_debug_refine": (C.c_int, [_vp, _dp, _up, _dp, _dp]),
    "sim3opt_homography_batch_debug_decompose": (C.c_int, [_vp, _dp, _up, _dp, _ip, _ip, _ip, _ip, _ip, _ip, _dp,
                                                           _dp]),
    "sim3opt_sim3_batch_options_default": (None, [C.POINTER(Sim3BatchOptions)]),
    "sim3opt_sim3_batch_create": (_vp, []),
    "sim3opt_sim3_batch_destroy": (None, [_vp]),
    "sim3opt_sim3_batch_last_error": (C.c_char_p, [_vp]),
    "sim3opt_sim3_batch_set_options": (C.c_int, [_vp, C.POINTER(Sim3BatchOptions)]),
    "sim3opt_sim3_batch_set_problems": (C.c_int, [_vp, C.c_int32, _ip, _dp, _dp, _dp, _dp, C.c_double, C.c_double,
                                                  C.c_double]),
    "sim3opt_sim3_batch_dims": (C.c_int, [_vp, _ip, _ip, _ip]),
    "sim3opt_sim3_batch_solve": (C.c_int, [_vp]),
    "sim3opt_sim3_batch_get_sim3": (C.c_int, [_vp, _dp, _dp]),
    "sim3opt_sim3_batch_get_inliers": (C.c_int, [_vp, _up, _ip]),
    "sim3opt_sim3_batch_get_summary": (C.c_int, [_vp, _ip, _ip, _ip, _dp, _dp, _ip, _dp]),
    "sim3opt_sim3_batch_debug_hypotheses": (C.c_int, [_vp, C.c_int32, _ip, _ip, _ip, _dp, _ip, _dp]),
    "sim3opt_sim3_batch_debug_score": (C.c_int, [_vp, C.c_int32, _dp, _ip, _dp]),
    "sim3opt_sim3_batch_debug_refine": (C.c_int, [_vp, _dp, _up, _dp, _ip, _dp, _ip]),
    "sim3opt_sim3_batch_debug_information": (C.c_int, [_vp, _dp, _up, _dp, _dp, _ip]),
    "sim3opt_match_batch_options_default": (None, [C.POINTER(MatchBatchOptions)]),
    "sim3opt_match_batch_create": (_vp, []),
    "sim3opt_match_batch_destroy": (None, [_vp]),
    "sim3opt_match_batch_last_error": (C.c_char_p, [_vp]),
    "sim3opt_match_batch_set_options": (C.c_int, [_vp, C.POINTER(MatchBatchOptions)]),
    "sim3opt_match_batch_set_frames": (C.c_int, [_vp, C.c_int32, _ip, _ip, _fp, _fp, _fp, _fp, C.c_double, C.c_double,
                                                 C.c_double, C.c_int32, C.c_int32]),
    "sim3opt_match_batch_set_pairs": (C.c_int, [_vp, C.c_int32, _ip]),
    "sim3opt_match_batch_dims": (C.c_int, [_vp, _ip, _ip, _ip, _ip, _ip]),
    "sim3opt_match_batch_solve": (C.c_int, [_vp]),
    "sim3opt_match_batch_get_match_ptr": (C.c_int, [_vp, _ip]),
    "sim3opt_match_batch_get_matches": (C.c_int, [_vp, _ip, _ip, _fp, _dp, _dp, _dp, _dp, _dp]),
    "sim3opt_match_batch_get_summary": (C.c_int, [_vp, _ip, _ip, _ip, _ip, _ip]),
    "sim3opt_match_batch_debug_nn": (C.c_int, [_vp, C.c_int32, _ip, _fp, _ip, _fp]),
    "sim3opt_match_batch_debug_depth": (C.c_int, [_vp, C.c_int32, C.c_int32, _fp, _dp, _ip]),
    "sim3opt_median_depth_ratio": (C.c_int, [C.c_int32, _ip, _dp, _dp, _dp]),
    "sim3opt_place_batch_options_default": (None, [C.POINTER(PlaceBatchOptions)]),
    "sim3opt_place_batch_create": (_vp, []),
    "sim3opt_place_batch_destroy": (None, [_vp]),
    "sim3opt_place_batch_last_error": (C.c_char_p, [_vp]),
    "sim3opt_place_batch_set_options": (C.c_int, [_vp, C.POINTER(PlaceBatchOptions)]),
    "sim3opt_place_batch_set_vocabulary": (C.c_int, [_vp, C.c_int32, _ip, _fp, _dp, _ip]),
    "sim3opt_place_batch_set_frames": (C.c_int, [_vp, C.c_int32, _ip, _fp]),
    "sim3opt_place_batch_dims": (C.c_int, [_vp, _ip, _ip, _ip, _ip, _ip, _ip]),
    "sim3opt_place_batch_solve": (C.c_int, [_vp]),
    "sim3opt_place_batch_get_results": (C.c_int, [_vp, _ip, _ip, _dp, _dp, _ip, _ip]),
    "sim3opt_place_batch_get_pairs": (C.c_int, [_vp, C.c_int32, _ip, _ip]),
    "sim3opt_place_batch_get_bow": (C.c_int, [_vp, _ip, _ip, _dp]),
    "sim3opt_place_batch_debug_words": (C.c_int, [_vp, C.c_int32, _fp, _ip, _dp]),
    "sim3opt_place_batch_debug_scores": (C.c_int, [_vp, C.c_int32, _dp]),
    "sim3opt_place_batch_debug_islands": (C.c_int, [_vp, C.c_int32, _ip, _ip, _dp, _ip, _ip, _dp]),
    "sim3opt_vocabulary_options_default": (None, [C.POINTER(VocabularyOptions)]),
    "sim3opt_vocabulary_create": (_vp, []),
    "sim3opt_vocabulary_destroy": (None, [_vp]),
    "sim3opt_vocabulary_last_error": (C.c_char_p, [_vp]),
    "sim3opt_vocabulary_set_options": (C.c_int, [_vp, C.POINTER(VocabularyOptions)]),
    "sim3opt_vocabulary_set_frames": (C.c_int, [_vp, C.c_int32, _ip, _fp]),
    "sim3opt_vocabulary_train": (C.c_int, [_vp]),
    "sim3opt_vocabulary_dims": (C.c_int, [_vp, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _ip]),
    "sim3opt_vocabulary_get_vocabulary": (C.c_int, [_vp, _ip, _fp, _dp, _ip]),
    "sim3opt_vocabulary_get_assignment": (C.c_int, [_vp, _ip, _ip]),
    "sim3opt_vocabulary_debug_seeding": (C.c_int, [_vp, C.c_int32, _ip, _ip, _ip, _dp, _dp]),
    "sim3opt_vocabulary_debug_lloyd": (C.c_int, [_vp, C.c_int32, C.c_int32, _ip, _ip, _ip, _fp]),
    "sim3opt_vocabulary_save": (C.c_int, [C.c_char_p, C.c_int32, _ip, _fp, _dp, _ip]),
    "sim3opt_vocabulary_load": (C.c_int, [C.c_char_p, _ip, C.POINTER(_ip), C.POINTER(_fp), C.POINTER(_dp), C.POINTER(_ip)]),
    "sim3opt_vocabulary_free": (None, [_vp]),
    "sim3opt_surf_batch_options_default": (None, [C.POINTER(SurfBatchOptions)]),
    "sim3opt_surf_batch_create": (_vp, []),
    "sim3opt_surf_batch_destroy": (None, [_vp]),
    "sim3opt_surf_batch_last_error": (C.c_char_p, [_vp]),
    "sim3opt_surf_batch_set_options": (C.c_int, [_vp, C.POINTER(SurfBatchOptions)]),
    "sim3opt_surf_batch_set_images": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _up]),
    "sim3opt_surf_batch_dims": (C.c_int, [_vp, _ip, _ip, _ip, _ip, _ip]),
    "sim3opt_surf_batch_solve": (C.c_int, [_vp]),
    "sim3opt_surf_batch_get_kp_ptr": (C.c_int, [_vp, _ip]),
    "sim3opt_surf_batch_get_keypoints": (C.c_int, [_vp, _fp, _fp, _fp, _fp, _fp, _ip, _ip]),
    "sim3opt_surf_batch_get_summary": (C.c_int, [_vp, _ip, _ip, _ip, _ip]),
    "sim3opt_surf_batch_debug_integral": (C.c_int, [_vp, C.c_int32, _ip]),
    "sim3opt_surf_batch_debug_responses": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _ip, _ip, _fp, _fp]),
    "sim3opt_surf_batch_debug_candidates": (C.c_int, [_vp, C.c_int32, _ip, _ip, _fp, _fp, _up, _fp]),
    "sim3opt_surf_batch_debug_orientation": (C.c_int, [_vp, C.c_int32, _ip, _fp, _fp, _fp, _fp]),
    "sim3opt_surf_batch_debug_patch": (C.c_int, [_vp, C.c_int32, _fp]),
    "sim3opt_frames_options_default": (None, [C.POINTER(FrameStoreOptions)]),
    "sim3opt_frames_create": (_vp, []),
    "sim3opt_frames_destroy": (None, [_vp]),
    "sim3opt_frames_last_error": (C.c_char_p, [_vp]),
    "sim3opt_frames_set_options": (C.c_int, [_vp, C.POINTER(FrameStoreOptions)]),
    "sim3opt_frames_set": (C.c_int, [_vp, C.c_int32, _ip, _fp, _fp]),
    "sim3opt_frames_get_dims": (C.c_int, [_vp, _ip, _ip, _ip, C.POINTER(C.c_int64), _ip]),
    "sim3opt_frames_get": (C.c_int, [_vp, _ip, _fp, _fp]),
    "sim3opt_frames_debug_compact": (C.c_int, [_vp, C.c_int32, _ip, _ip, _fp, _fp]),
    "sim3opt_surf_batch_solve_into": (C.c_int, [_vp, _vp]),
    "sim3opt_vocabulary_set_frames_from": (C.c_int, [_vp, _vp]),
    "sim3opt_place_batch_set_frames_from": (C.c_int, [_vp, _vp]),
    "sim3opt_match_batch_set_frames_from": (C.c_int, [_vp, _vp, C.c_int32, _ip, _fp, _fp, C.c_double, C.c_double,
                                                      C.c_double, C.c_int32, C.c_int32]),
    "sim3opt_surf_reference_image": (C.c_int, [C.POINTER(SurfBatchOptions), C.c_int32, C.c_int32, C.c_int32, _up, C.c_int32,
                                               _fp, _fp, _fp, _fp, _fp, _ip, _ip, _ip, _ip, C.c_int32, C.c_int32, _fp, _fp,
                                               C.c_int32, _ip, _fp, _fp, _up, _fp]),
    "sim3opt_track_batch_options_default": (None, [C.POINTER(TrackBatchOptions)]),
    "sim3opt_track_batch_create": (_vp, []),
    "sim3opt_track_batch_destroy": (None, [_vp]),
    "sim3opt_track_batch_last_error": (C.c_char_p, [_vp]),
    "sim3opt_track_batch_set_options": (C.c_int, [_vp, C.POINTER(TrackBatchOptions)]),
    "sim3opt_track_batch_set_frames": (C.c_int, [_vp, C.c_int32, _ip, _fp]),
    "sim3opt_track_batch_set_frames_from": (C.c_int, [_vp, _vp]),
    "sim3opt_track_batch_set_matches": (C.c_int, [_vp, C.c_int32, _ip, _ip, _ip, _ip, _up, _dp, _dp]),
    "sim3opt_track_batch_set_cameras": (C.c_int, [_vp, C.c_int32, _dp, C.c_double, C.c_double, C.c_double]),
    "sim3opt_track_batch_solve": (C.c_int, [_vp]),
    "sim3opt_track_batch_dims": (C.c_int, [_vp] + [_ip] * 9),
    "sim3opt_track_batch_get_tracks": (C.c_int, [_vp, _ip, _ip, _ip, _ip, _ip]),
    "sim3opt_track_batch_get_match_track": (C.c_int, [_vp, _ip]),
    "sim3opt_track_batch_get_points": (C.c_int, [_vp, _dp, _ip]),
    "sim3opt_track_batch_get_ba": (C.c_int, [_vp, C.c_int32, _dp, _ip, _ip, _dp]),
    "sim3opt_track_reference": (C.c_int, [C.c_int32, _ip, _fp, C.c_int32, _ip, _ip, _ip, _ip, _up, _dp, _dp, _dp,
                                          C.c_double, C.c_double, C.c_double, C.c_double] + [_ip] * 8 + [_dp, _ip]),
}

_lib = None


def hip_runtime_path():
    """Path of the libamdhip64 this process has mapped (the one libsim3opt.so is bound to), or None."""
    try:
        with open("/proc/self/maps") as f:
            for ln in f:
                if "libamdhip64" in ln:
                    return ln.split()[-1]
    except OSError:
        pass
    return None


MISSING_SYMBOLS = []  # what load(tolerant=True) found missing


def load(tolerant=False):
    """Loads libsim3opt.so and binds every declared symbol (raises if one is missing).  tolerant: for a comparison with
    an older build named by SIM3OPT_LIB, an export it lacks is left unbound and listed in MISSING_SYMBOLS; it holds
    for the process, since the library is loaded once."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not built: run `python -m sim3opt_amd.build` (hipcc, gfx950)")
        # One HIP runtime per process: libsim3opt.so names the system's libamdhip64, a PyTorch-ROCm wheel
        # carries its own.  Whichever is mapped first serves both (same soname) -- but if the library were
        # mapped before torch and torch then initialised its own copy, the library's copy would find the
        # device taken ("no usable HIP device").  So a process that will ALSO use torch (bench.py, the
        # tests, build() + smoke() in one interpreter) must map torch's first: it says so by importing
        # torch before this call, or by SIM3OPT_PRELOAD_TORCH=1.  Otherwise the library binds to the ROCm
        # it was compiled against and this module imports nothing.
        if "torch" not in sys.modules and os.environ.get("SIM3OPT_PRELOAD_TORCH", "0") not in ("", "0"):
            try:
                import torch  # noqa: F401
            except Exception:  # no torch in this interpreter: the system runtime is the only one
                pass
        L = C.CDLL(LIB_PATH)
        if os.environ.get("SIM3OPT_VERBOSE_LOAD"):
            print(f"sim3opt: {LIB_PATH} loaded; HIP runtime mapped: {hip_runtime_path()}", file=sys.stderr)
        for name, (res, args) in SYMBOLS.items():
            if tolerant and not hasattr(L, name):
                MISSING_SYMBOLS.append(name)
                continue
            fn = getattr(L, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, C.c_int32, C.c_int32)
ALLGATHERV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, C.POINTER(C.c_int64), C.c_int32, C.c_int32)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, C.POINTER(C.c_int64), _dp, C.POINTER(C.c_int64), C.c_int32,
                           C.c_int32)


class Sim3OptError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sim3opt error {code}: {msg}")
        self.code = code


def device_memory_in_use():
    """(blocks, bytes) of device memory the library's handles and calls of this process hold right now
    (sim3opt_device_memory_in_use): a call that keeps no device memory leaves both as they were."""
    o = (C.c_int64 * 2)()
    load().sim3opt_device_memory_in_use(o)
    return int(o[0]), int(o[1])


def release_device_cache():
    """Gives the cached device blocks, streams, events and pinned blocks back to the runtime
    (sim3opt_release_device_cache)."""
    load().sim3opt_release_device_cache()


def debug_device_memory(on):
    """Switches the block cache's test mode (sim3opt_debug_device_memory): poisoned blocks with guarded tails.  Switching
    it on resets the report's counters."""
    load().sim3opt_debug_device_memory(int(bool(on)))


def debug_device_memory_report():
    """dict of filled, checked, overwritten (blocks) and first_offset (of the first overwritten tail, or -1) since the
    test mode was last switched on (sim3opt_debug_device_memory_report)."""
    o = (C.c_int64 * 4)()
    load().sim3opt_debug_device_memory_report(o)
    return dict(filled=int(o[0]), checked=int(o[1]), overwritten=int(o[2]), first_offset=int(o[3]))


def debug_device_memory_probe(nbytes, floating, overrun=0):
    """One block of `nbytes` bytes through the cache, `overrun` bytes set behind them, read back whole and freed
    (sim3opt_debug_device_memory_probe): the block's bytes as a uint8 array."""
    out = np.empty(int(nbytes) + int(nbytes) // 4 + 1024, dtype=np.uint8)  # (no block is rounded up further than this)
    size = load().sim3opt_debug_device_memory_probe(int(nbytes), int(bool(floating)), int(overrun),
                                                    out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.shape[0])
    if size < 0 or size > out.shape[0]:
        raise Sim3OptError(int(size), "debug_device_memory_probe")
    return out[:size].copy()


def default_options(**kw):
    o = Options()
    load().sim3opt_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


class Graph:
    """Thin object wrapper over sim3opt_graph* (one per optimiser, like g2o::SparseOptimizer)."""

    def __init__(self, **options):
        self._L = load()
        self._g = self._L.sim3opt_create()
        if not self._g:
            raise MemoryError("sim3opt_create")
        if options:
            self.set_options(**options)

    def close(self):
        if self._g:
            self._L.sim3opt_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            raise Sim3OptError(rc, self._L.sim3opt_last_error(self._g).decode())
        return rc

    # ---- configuration ----
    def set_options(self, **kw):
        o = Options()
        self._chk(self._L.sim3opt_get_options(self._g, C.byref(o)))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            cur = getattr(o, k)
            if hasattr(cur, "__len__"):  # array fields (amg_cycle, amg_passes, amg_over): element by element
                for i, x in enumerate(v):
                    cur[i] = x
            else:
                setattr(o, k, v)
        self._chk(self._L.sim3opt_set_options(self._g, C.byref(o)))

    def options(self):
        o = Options()
        self._chk(self._L.sim3opt_get_options(self._g, C.byref(o)))
        return o

    # ---- graph construction ----
    def add_vertex(self, vid, state, fixed=False):
        s = _f64(state)
        self._chk(self._L.sim3opt_add_vertex(self._g, int(vid), _p(s, _dp), int(bool(fixed))))

    def add_vertices(self, states, fixed=None, ids=None):
        s = _f64(states).reshape(-1, 8)
        f = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.uint8)
        i = None if ids is None else _i32(ids)
        self._chk(self._L.sim3opt_add_vertices(self._g, s.shape[0], _p(i, _ip), _p(s, _dp),
                                               _p(f, _up)))

    def add_edge(self, v0, v1, meas, info=None, kernel=KERNEL_NONE, kernel_delta=0.0):
        m = _f64(meas)
        inf = None if info is None else np.asfortranarray(info, dtype=np.float64).ravel(order="F")
        self._chk(self._L.sim3opt_add_edge(self._g, int(v0), int(v1), _p(m, _dp), _p(inf, _dp),
                                           int(kernel), float(kernel_delta)))

    def add_edges(self, v0, v1, meas, info=None, kernel=KERNEL_NONE, kernel_delta=0.0):
        """kernel / kernel_delta: one kind and delta for every edge, or per-edge arrays of length m."""
        a, b = _i32(v0), _i32(v1)
        m = _f64(meas).reshape(-1, 8)
        inf = None
        if info is not None:  # (m, 7, 7) [k, r, c] -> column-major blocks
            inf = _f64(np.asarray(info).reshape(-1, 7, 7).transpose(0, 2, 1)).reshape(-1, 49)
        per_edge = np.ndim(kernel) > 0 or np.ndim(kernel_delta) > 0
        if per_edge:  # checked before the edges go in, then set on them as set_edge_kernels sets them
            kinds = _i32(np.broadcast_to(kernel, a.shape))
            deltas = _f64(np.broadcast_to(kernel_delta, a.shape))
            bad = (kinds < 0) | (kinds >= len(KERNEL_NAMES)) | (
                (kinds != KERNEL_NONE) & ~(np.isfinite(deltas) & (deltas > 0)))
            if bad.any():
                raise Sim3OptError(ERR_ARG, f"add_edges: bad robust kernel or delta at edge {int(np.argmax(bad))}")
        m0 = self.num_edges
        self._chk(self._L.sim3opt_add_edges(self._g, a.shape[0], _p(a, _ip), _p(b, _ip),
                                            _p(m, _dp), _p(inf, _dp), KERNEL_NONE if per_edge else int(kernel),
                                            0.0 if per_edge else float(kernel_delta)))
        if per_edge:
            self.set_edge_kernels(np.arange(m0, m0 + a.shape[0]), kinds, deltas)

    def set_edge_kernels(self, edges, kinds, deltas):
        """e->setRobustKernel for the edges listed (insertion indices; None = 0..n-1), before or after
        initialize; kinds / deltas: scalars or arrays of the same length.  Bad input changes nothing."""
        if edges is None:
            n = max(np.size(kinds), np.size(deltas))
            e = None
        else:
            e = _i32(np.atleast_1d(edges))
            n = e.shape[0]
        k = _i32(np.broadcast_to(kinds, (n,)))
        d = _f64(np.broadcast_to(deltas, (n,)))
        self._chk(self._L.sim3opt_set_edge_kernels(self._g, n, _p(e, _ip), _p(k, _ip), _p(d, _dp)))

    def edge_kernels(self):
        """(kinds int32 (m,), deltas (m,)) of every edge."""
        m = self.num_edges
        k, d = np.empty(m, np.int32), np.empty(m)
        self._chk(self._L.sim3opt_get_edge_kernels(self._g, _p(k, _ip), _p(d, _dp)))
        return k, d

    @property
    def num_vertices(self):
        return self._L.sim3opt_num_vertices(self._g)

    @property
    def num_edges(self):
        return self._L.sim3opt_num_edges(self._g)

    def get_edge(self, k):
        a, b = C.c_int32(), C.c_int32()
        m = np.empty(8)
        self._chk(self._L.sim3opt_get_edge(self._g, int(k), C.byref(a), C.byref(b), _p(m, _dp)))
        return a.value, b.value, m

    # ---- multi-GPU ----
    def comm_init_rccl(self, rank, world, unique_id):
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        assert uid.shape == (128,)
        self._chk(self._L.sim3opt_comm_init(self._g, int(rank), int(world), _p(uid, _up)))

    def comm_init_callbacks(self, rank, world, allreduce, allgatherv, alltoallv=None):
        """allreduce(np_array, op) and allgatherv(np_array, offsets, rank) operate IN PLACE on
        numpy views of the library's pinned host staging buffer; the optional
        alltoallv(send, send_offsets, recv, recv_offsets, rank) is the neighbour exchange
        (send[send_offsets[p]:send_offsets[p+1]] goes to rank p, recv[...] comes from it)."""
        def _ar(ctx, buf, n, op):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(n,)), int(op))
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1

        def _ag(ctx, buf, offs, rk, world_):
            try:
                o = np.ctypeslib.as_array(offs, shape=(world_ + 1,))
                allgatherv(np.ctypeslib.as_array(buf, shape=(int(o[-1]),)), o, int(rk))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1

        def _aa(ctx, sbuf, soffs, rbuf, roffs, rk, world_):
            try:
                so = np.ctypeslib.as_array(soffs, shape=(world_ + 1,))
                ro = np.ctypeslib.as_array(roffs, shape=(world_ + 1,))
                sv = np.ctypeslib.as_array(sbuf, shape=(max(int(so[-1]), 1),))
                rv = np.ctypeslib.as_array(rbuf, shape=(max(int(ro[-1]), 1),))
                alltoallv(sv, so, rv, ro, int(rk))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1

        self._cb_refs = (ALLREDUCE_FN(_ar), ALLGATHERV_FN(_ag), ALLTOALLV_FN(_aa))  # keep alive
        self._chk(self._L.sim3opt_comm_init_callbacks(
            self._g, int(rank), int(world), C.cast(self._cb_refs[0], C.c_void_p),
            C.cast(self._cb_refs[1], C.c_void_p), None))
        if alltoallv is not None:
            self._chk(self._L.sim3opt_comm_set_alltoallv(self._g, C.cast(self._cb_refs[2], C.c_void_p)))

    def local_rows(self):
        a, b = C.c_int32(), C.c_int32()
        self._chk(self._L.sim3opt_local_rows(self._g, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_devices(self, devices, timeout_s=0.0):
        """One rank per entry of `devices` (1 to 8 HIP ordinals, repeats allowed), run by the library's own worker
        threads: this object stays one graph, called from one thread.  Between construction and initialize();
        timeout_s <= 0: a rank waits 120 s for its peers in a collective before it gives the group up."""
        d = _i32(list(devices))
        self._chk(self._L.sim3opt_set_devices(self._g, int(d.size), _p(d, _ip) if d.size else None, float(timeout_s)))

    def rank_count(self):
        """Ranks this graph drives: len(devices) of set_devices, else 1."""
        return int(self._L.sim3opt_rank_count(self._g))

    def local_rows_of_rank(self, rank):
        a, b = C.c_int32(), C.c_int32()
        self._chk(self._L.sim3opt_local_rows_of_rank(self._g, int(rank), C.byref(a), C.byref(b)))
        return a.value, b.value

    def device_bytes_of_rank(self, rank):
        """device_bytes() of one rank of a set_devices graph."""
        b = (C.c_int64 * 2)()
        self._chk(self._L.sim3opt_device_bytes_of_rank(self._g, int(rank), b))
        return int(b[0]), int(b[1])

    # ---- diagnostic read-outs of the in-process transport (a set_devices graph with more than one rank) ----
    def comm_apply_allreduce(self, rows, op=0, phase=0):
        """One all-reduce (op 0 sum, 1 max) of the ranks' operands: rows (world, n), row r is rank r's, placed on an even
        (phase 0) or odd (phase 1) double of device memory; returns what every rank holds afterwards, (world, n)."""
        a = _f64(rows)
        if a.ndim != 2 or a.shape[0] != self.rank_count():
            raise ValueError("rows must be (rank_count, n)")
        out = np.empty_like(a)
        self._chk(self._L.sim3opt_comm_apply_allreduce(self._g, int(a.shape[1]), int(op), int(phase), _p(a, _dp),
                                                       _p(out, _dp)))
        return out

    def comm_apply_allgatherv(self, offs, rows, phase=0):
        """One in-place all-gather of a vector split at offs (world + 1): rows (world, offs[-1]), row r is rank r's
        whole vector before; returns the vectors afterwards."""
        o = np.ascontiguousarray(offs, dtype=np.int64)
        a = _f64(rows)
        if o.shape != (self.rank_count() + 1,) or a.shape != (self.rank_count(), max(int(o[-1]), 0)):
            raise ValueError("offs must be (rank_count + 1,), rows (rank_count, offs[-1])")
        out = np.empty_like(a)
        self._chk(self._L.sim3opt_comm_apply_allgatherv(self._g, _p(o, C.POINTER(C.c_int64)), int(phase), _p(a, _dp),
                                                        _p(out, _dp)))
        return out

    def comm_apply_exchange(self, soffs, roffs, send, recv, send_phase=0, recv_phase=0):
        """One neighbour exchange: soffs / roffs (world, world + 1) are the ranks' plans, send / recv lists of the
        ranks' send buffers and pre-filled receive buffers; returns the list of the receive buffers afterwards."""
        w = self.rank_count()
        so = np.ascontiguousarray(soffs, dtype=np.int64)
        ro = np.ascontiguousarray(roffs, dtype=np.int64)
        if so.shape != (w, w + 1) or ro.shape != (w, w + 1) or len(send) != w or len(recv) != w:
            raise ValueError("plans must be (rank_count, rank_count + 1), one buffer per rank")
        for r in range(w):
            if len(send[r]) != max(int(so[r, -1]), 0) or len(recv[r]) != max(int(ro[r, -1]), 0):
                raise ValueError("rank %d: a buffer is as long as its plan's last offset" % r)
        s = _f64(np.concatenate([_f64(x) for x in send] + [np.zeros(1)]))  # (never an empty array: a pointer is needed)
        v = _f64(np.concatenate([_f64(x) for x in recv] + [np.zeros(1)])).copy()
        i64 = C.POINTER(C.c_int64)
        self._chk(self._L.sim3opt_comm_apply_exchange(self._g, _p(so, i64), _p(ro, i64), int(send_phase),
                                                      int(recv_phase), _p(s, _dp), _p(v, _dp)))
        cuts = np.cumsum([0] + [len(x) for x in recv])
        return [v[cuts[r]:cuts[r + 1]].copy() for r in range(w)]

    def comm_local_state(self):
        """(capacity of a mailbox in doubles, collectives so far) of the in-process transport."""
        o = (C.c_int64 * 2)()
        self._chk(self._L.sim3opt_comm_local_state(self._g, o))
        return int(o[0]), int(o[1])

    # ---- optimisation ----
    def initialize(self):
        self._chk(self._L.sim3opt_initialize(self._g))

    def optimize(self, max_iters):
        """Returns iterations executed (g2o convention: 0 failure, -1 nothing to do)."""
        it = self._L.sim3opt_optimize(self._g, int(max_iters))
        if it == 0 and max_iters > 0:
            raise Sim3OptError(0, self._L.sim3opt_last_error(self._g).decode())
        return it

    def chi2(self):
        v = C.c_double()
        self._chk(self._L.sim3opt_chi2(self._g, C.byref(v)))
        return v.value

    def get_vertex(self, vid):
        s = np.empty(8)
        self._chk(self._L.sim3opt_get_vertex(self._g, int(vid), _p(s, _dp)))
        return s

    def set_vertex(self, vid, state):
        s = _f64(state)
        self._chk(self._L.sim3opt_set_vertex(self._g, int(vid), _p(s, _dp)))

    def get_vertices(self):
        s = np.empty((self.num_vertices, 8))
        self._chk(self._L.sim3opt_get_vertices(self._g, _p(s, _dp)))
        return s

    def set_vertices(self, states):
        s = _f64(states).reshape(-1, 8)
        assert s.shape[0] == self.num_vertices
        self._chk(self._L.sim3opt_set_vertices(self._g, _p(s, _dp)))

    def stats(self):
        out = []
        for i in range(self._L.sim3opt_num_iterations(self._g)):
            st = IterStats()
            self._chk(self._L.sim3opt_get_stats(self._g, i, C.byref(st)))
            out.append(st)
        return out

    def trust_region_stats(self):
        """Per-iteration TrustRegionStats of the last optimize() -- a dogleg run (options.algorithm = 2)."""
        out = []
        for i in range(self._L.sim3opt_num_iterations(self._g)):
            st = TrustRegionStats()
            self._chk(self._L.sim3opt_get_trust_region_stats(self._g, i, C.byref(st)))
            out.append(st)
        return out

    def kernel_times(self, reset=False):
        kt = KernelTimes()
        self._chk(self._L.sim3opt_get_kernel_times(self._g, C.byref(kt)))
        if reset:
            self._chk(self._L.sim3opt_reset_kernel_times(self._g))
        return kt

    def pcg_schedule_stats(self, reset=False):
        """How the PCG loops were scheduled since initialize / the last reset: dict of iterations `enqueued`, of them
        `past_done` (enqueued after the device had finished the solve), `sync_polls` (looks that drained the queue) and
        `overlapped_polls` (looks waited for with the next chunk queued)."""
        o = (C.c_int64 * 4)()
        self._chk(self._L.sim3opt_pcg_schedule_stats(self._g, o, 1 if reset else 0))
        return dict(zip(("enqueued", "past_done", "sync_polls", "overlapped_polls"), (int(x) for x in o)))

    def comm_times(self):
        """Device time, count and payload of the collectives since initialize / the last reset
        (options.time_kernels): dict of the sim3opt_comm_times fields."""
        ct = CommTimes()
        self._chk(self._L.sim3opt_get_comm_times(self._g, C.byref(ct)))
        return {k: getattr(ct, k) for k, _ in CommTimes._fields_}

    # ---- kernel-level access ----
    def edge_errors(self):
        e = np.empty((self.num_edges, 7))
        self._chk(self._L.sim3opt_edge_errors(self._g, _p(e, _dp)))
        return e

    def edge_chi2(self):
        """(chi2, rho, weight), each (m,): e^T Omega e of every edge (g2o Edge::chi2) and rho / rho' of its
        robust kernel at the current estimates; rho sums to chi2()."""
        m = self.num_edges
        c, r, w = np.empty(m), np.empty(m), np.empty(m)
        self._chk(self._L.sim3opt_edge_chi2(self._g, _p(c, _dp), _p(r, _dp), _p(w, _dp)))
        return c, r, w

    def edge_jacobians(self):
        """Closed-form Jacobians of every edge at the current estimates (needs fix_small_angle_b=1):
        e (m, 7) and J (m, 7, 14), columns 0..6 = de/dd0, 7..13 = de/dd1 (updates S <- exp(d) S)."""
        m = self.num_edges
        e, J = np.empty((m, 7)), np.empty((m, 7, 14))
        self._chk(self._L.sim3opt_edge_jacobians(self._g, _p(e, _dp), _p(J, _dp)))
        return e, J

    def linearize(self):
        self._chk(self._L.sim3opt_linearize(self._g))

    def debug_linearization(self):
        """Diagnostic: linearises (the DUMP instantiation of the linearisation kernel) and returns a dict: J
        (n_active, 15, 7) = the 14 Jacobian columns and e as the Gram phase read them, w (n_active,), active, scratch
        (n_incidences, 35), incptr, inc0, inc1, slot01, slot10, trace, maxdiag.  get_system() afterwards is the
        system of linearize()."""
        na, ni = C.c_int32(), C.c_int32()
        self._chk(self._L.sim3opt_debug_linearization_dims(self._g, C.byref(na), C.byref(ni)))
        na, ni, m = na.value, ni.value, self.num_edges
        nb, _ = self.system_dims()
        d = dict(J=np.empty((na, 15, 7)), w=np.empty(na), active=np.empty(na, dtype=np.int32),
                 scratch=np.empty((ni, 35)), incptr=np.empty(nb + 1, dtype=np.int32))
        for k in ("inc0", "inc1", "slot01", "slot10"):
            d[k] = np.empty(m, dtype=np.int32)
        tr, mx = C.c_double(), C.c_double()
        self._chk(self._L.sim3opt_debug_linearization(
            self._g, _p(d["J"], _dp), _p(d["w"], _dp), _p(d["active"], _ip), _p(d["scratch"], _dp),
            _p(d["incptr"], _ip), _p(d["inc0"], _ip), _p(d["inc1"], _ip), _p(d["slot01"], _ip), _p(d["slot10"], _ip),
            C.byref(tr), C.byref(mx)))
        d["trace"], d["maxdiag"] = tr.value, mx.value
        return d

    def debug_update(self, x, lam=0.0, fail=False, grid=0):
        """Diagnostic: (states, backup, chi2, scale) of an LM trial with the step x (7 per block row) at damping lam;
        the estimates are restored.  fail: with the exact solver's failure token set; grid: workgroups (= partial sums)
        of the chi2 and scale reductions, 0 = a trial's own."""
        nb, _ = self.system_dims()
        xs = _f64(x).reshape(-1)
        assert xs.shape[0] == 7 * nb
        nv = self.num_vertices
        st, bk = np.empty((nv, 8)), np.empty((nv, 8))
        chi, sc = C.c_double(), C.c_double()
        self._chk(self._L.sim3opt_debug_update(self._g, _p(xs, _dp), float(lam), int(bool(fail)), int(grid),
                                               _p(st, _dp), _p(bk, _dp), C.byref(chi), C.byref(sc)))
        return st, bk, chi.value, sc.value

    def debug_dogleg(self, h_gn, ca=0.0, cg=1.0, fail=False, grid=0, j0=0, j1=0, scalars=True, states=True):
        """Diagnostic: the launches of a dogleg iteration after its solve, on a caller's h_gn (7 per block row).  Returns
        (scalars, states, backup): the six scalars b.b, b^T H b, g.g, b.g, (Hb).g, g^T H g (None without `scalars`) and
        the estimates / the backup after k_dogleg_oplus with h_dl = ca b + cg h_gn (None without `states`); the
        estimates are restored.  grid: workgroups of k_dl_dots (0: its own); [j0, j1): the entries its dots run over
        (both 0: all); fail: with the exact solver's failure token set."""
        nb, _ = self.system_dims()
        xs = _f64(h_gn).reshape(-1) if h_gn is not None else None
        assert xs is None or xs.shape[0] == 7 * nb
        nv = self.num_vertices
        sc = np.empty(6) if scalars else None
        st = np.empty((nv, 8)) if states else None
        bk = np.empty((nv, 8)) if states else None
        self._chk(self._L.sim3opt_debug_dogleg(self._g, _p(xs, _dp), float(ca), float(cg), int(bool(fail)), int(grid),
                                               int(j0), int(j1), _p(sc, _dp), _p(st, _dp), _p(bk, _dp)))
        return sc, st, bk

    def column_vector_stride(self):
        """Doubles between the systems' vectors of a column solve: 7 x block rows, rounded up to a multiple of 64."""
        nb, _ = self.system_dims()
        return (7 * nb + 63) // 64 * 64

    def debug_column_vectors(self, kernel, n, out, grid=0, at=None, system=0, a=None, b=None, first=0, count=0, col=0,
                             rows=None):
        """Diagnostic: one vector kernel of the columns of the inverse on the caller's data at vector length n; returns
        the output buffer after the launch, `out` being what it held before (never modified).  kernel "rhs": at (K,)
        unit entries, out (K, vs); "residual": a - b on system `system`, out (vs,); "axpy": y += a, out (vs,) holding y;
        "gather": column col of blocks first .. first + count - 1 of out (n_blocks, 49) from a = y at block rows
        rows[first .. first + count).  vs = column_vector_stride(); grid: workgroups, 0 = a solve's."""
        op = ("rhs", "residual", "axpy", "gather").index(kernel) if isinstance(kernel, str) else int(kernel)
        o = _f64(out).copy() if out is not None else None
        vs = self.column_vector_stride()
        K = 0
        at64 = None
        if at is not None:
            at64 = np.ascontiguousarray(at, dtype=np.int64).reshape(-1)
            K = at64.shape[0]
        if o is not None:
            if op == 0:
                assert o.shape == (K, vs)
            elif op in (1, 2):
                assert o.shape == (vs,)
            elif op == 3:
                assert o.ndim == 2 and o.shape[1] == 49
        av = _f64(a).reshape(-1) if a is not None else None
        bv = _f64(b).reshape(-1) if b is not None else None
        assert av is None or av.shape[0] == n
        assert bv is None or bv.shape[0] == n
        rw = _i32(rows).reshape(-1) if rows is not None else None
        assert rw is None or rw.shape[0] >= first + count
        nblk = o.shape[0] if (o is not None and op == 3) else 0
        self._chk(self._L.sim3opt_debug_column_vectors(
            self._g, op, int(grid), int(n), K, _p(at64, C.POINTER(C.c_int64)), int(system), _p(av, _dp), _p(bv, _dp),
            int(first), int(count), int(col), _p(rw, _ip), int(nblk), _p(o, _dp)))
        return o

    def debug_factor(self, context=0, lam=0.0, vals=None, b=None, solve=True, selinv=False):
        """Diagnostic: the exact block Cholesky of context 0 (the LM's solver) or 1 (the marginals') on the last
        linearisation, or on injected vals (nnzb, 7, 7) [k, r, c] / b (7 nb), read out as a dict in the plan's
        numbering, blocks [s, r, c]: Aperm, bp, L, Dinv, y, fail, bord, brow; with solve xp and x (by block rows of
        the system); with selinv (context 1) Z and singular."""
        nb, nL, nz = C.c_int32(), C.c_int64(), C.c_int64()
        self._chk(self._L.sim3opt_debug_factor_dims(self._g, int(context), C.byref(nb), C.byref(nL), C.byref(nz)))
        nb, nL, nz = nb.value, nL.value, nz.value
        v = bb = None
        if vals is not None:
            v = _f64(np.asarray(vals).reshape(nz, 7, 7).transpose(0, 2, 1)).reshape(-1)
        if b is not None:
            bb = _f64(b).reshape(-1)
            assert bb.shape[0] == 7 * nb
        d = dict(Aperm=np.empty((nL, 49)), bp=np.empty((nb, 7)), L=np.empty((nL, 49)), Dinv=np.empty((nb, 49)),
                 y=np.empty((nb, 7)), xp=np.empty((nb, 7)), x=np.empty((nb, 7)), Z=np.empty((nL if selinv else 0, 49)),
                 bord=np.empty(nL, dtype=np.int32), brow=np.empty(nL, dtype=np.int32))
        fw, sg = C.c_int32(), C.c_int32()
        self._chk(self._L.sim3opt_debug_factor(
            self._g, int(context), float(lam), _p(v, _dp), _p(bb, _dp), int(bool(solve)), int(bool(selinv)),
            _p(d["Aperm"], _dp), _p(d["bp"], _dp), _p(d["L"], _dp), _p(d["Dinv"], _dp), _p(d["y"], _dp),
            _p(d["xp"], _dp), _p(d["x"], _dp), C.byref(fw), _p(d["Z"], _dp) if selinv else None, C.byref(sg),
            _p(d["bord"], _ip), _p(d["brow"], _ip)))
        for k in ("Aperm", "L", "Dinv", "Z"):
            d[k] = d[k].reshape(-1, 7, 7).transpose(0, 2, 1).copy()
        if not solve:
            del d["xp"], d["x"]
        if not selinv:
            del d["Z"]
        else:
            d["singular"] = sg.value
        d["fail"] = fw.value
        return d

    def system_dims(self):
        nb, nnzb = C.c_int32(), C.c_int64()
        self._chk(self._L.sim3opt_system_dims(self._g, C.byref(nb), C.byref(nnzb)))
        return nb.value, nnzb.value

    def get_system(self):
        """(rowptr, colidx, blocks[nnzb, 7, 7] indexed [k, r, c], b)."""
        nb, nnzb = self.system_dims()
        rowptr = np.empty(nb + 1, dtype=np.int32)
        colidx = np.empty(nnzb, dtype=np.int32)
        vals = np.empty((nnzb, 49))
        b = np.empty(7 * nb)
        self._chk(self._L.sim3opt_get_system(self._g, _p(rowptr, _ip), _p(colidx, _ip),
                                             _p(vals, _dp), _p(b, _dp)))
        return rowptr, colidx, vals.reshape(-1, 7, 7).transpose(0, 2, 1).copy(), b

    def dense_system(self):
        """Dense (H, b) assembled from the block-CSR copy (small graphs, tests only)."""
        rowptr, colidx, blocks, b = self.get_system()
        nb = rowptr.shape[0] - 1
        H = np.zeros((7 * nb, 7 * nb))
        for i in range(nb):
            for k in range(rowptr[i], rowptr[i + 1]):
                j = colidx[k]
                H[7 * i:7 * i + 7, 7 * j:7 * j + 7] += blocks[k]
        return H, b

    def solve(self, lam):
        nb, _ = self.system_dims()
        x = np.empty(7 * nb)
        it = C.c_int32()
        rr = C.c_double()
        self._chk(self._L.sim3opt_solve(self._g, float(lam), _p(x, _dp), C.byref(it),
                                        C.byref(rr)))
        return x, it.value, rr.value

    def preconditioner_in_use(self):
        rc = self._L.sim3opt_preconditioner_in_use(self._g)
        if rc < 0:
            self._chk(rc)
        return rc

    def amg_in_use(self):
        """dict(levels, partitioned_levels, cycle): what the automatic multigrid choices resolved to."""
        nl, ns = C.c_int32(), C.c_int32()
        v = np.zeros(4, dtype=np.int32)
        self._chk(self._L.sim3opt_amg_in_use(self._g, C.byref(nl), C.byref(ns), _p(v, _ip)))
        return dict(levels=nl.value, partitioned_levels=ns.value, cycle=[int(x) for x in v])

    def device_bytes(self):
        """(bytes of the block arrays as allocated on this rank, bytes one rank holding the whole graph allocates)."""
        b = (C.c_int64 * 2)()
        self._chk(self._L.sim3opt_device_bytes(self._g, b))
        return int(b[0]), int(b[1])

    def system_pattern(self):
        """(rowptr, colidx) of the block-CSR system; host only."""
        nb, nnzb = C.c_int32(), C.c_int64()
        self._chk(self._L.sim3opt_system_pattern(self._g, C.byref(nb), C.byref(nnzb), None, None))
        rowptr = np.zeros(nb.value + 1, dtype=np.int32)
        colidx = np.zeros(max(nnzb.value, 1), dtype=np.int32)
        self._chk(self._L.sim3opt_system_pattern(self._g, None, None, _p(rowptr, _ip), _p(colidx, _ip)))
        return rowptr, colidx[:nnzb.value]

    def linear_solver_in_use(self):
        rc = self._L.sim3opt_linear_solver_in_use(self._g)
        if rc < 0:
            self._chk(rc)
        return rc

    def direct_plan(self, max_pairs=0):
        """Plan of the exact sparse block Cholesky as a dict of numpy arrays; host only."""
        dims = np.zeros(8, dtype=np.int64)
        dp = dims.ctypes.data_as(C.POINTER(C.c_int64))
        null = [None] * 12
        self._chk(self._L.sim3opt_direct_plan(self._g, int(max_pairs), dp, *null))
        nb, nL, npairs, height, ngroups, nlev, nsrc, nrounds = (int(x) for x in dims[:8])
        arr = dict(perm=nb, colptr=nb + 1, lrow=nL, srcptr=nL + 1, src=nsrc, pairptr=nL + 1,
                   pa=npairs, pb=npairs, gptr=ngroups + 1, lcolp=nlev + 1, rptr=nlev + 1,
                   cells=18 * nrounds)
        out = {k: np.zeros(max(n, 1), dtype=np.int32) for k, n in arr.items()}
        self._chk(self._L.sim3opt_direct_plan(self._g, int(max_pairs), dp,
                                              *[_p(out[k], _ip) for k in arr]))
        out = {k: out[k][:n] for k, n in arr.items()}
        out.update(nb=nb, nL=nL, npairs=npairs, height=height, ngroups=ngroups, nlevels=nlev,
                   nrounds=nrounds)
        return out

    def marginals(self, pairs, lam=0.0):
        """Blocks (a, b) of (H + lam I)^-1 at the current estimates for pairs [(id_a, id_b), ...]: (n, 7, 7)
        indexed [q, r, c], rows = id_a's tangent [omega upsilon sigma], cols = id_b's."""
        pr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        a, b = _i32(pr[:, 0]), _i32(pr[:, 1])
        n = pr.shape[0]
        cov = np.empty((max(n, 1), 49))
        self._chk(self._L.sim3opt_marginals(self._g, float(lam), n, _p(a, _ip), _p(b, _ip), _p(cov, _dp)))
        return cov[:n].reshape(-1, 7, 7).transpose(0, 2, 1).copy()

    def marginal_covariances(self, lam=0.0):
        """Diagonal blocks of (H + lam I)^-1 of every free vertex, insertion order: (nfree, 7, 7)."""
        nb, _ = self.system_dims()
        cov = np.empty((max(nb, 1), 49))
        self._chk(self._L.sim3opt_marginal_covariances(self._g, float(lam), _p(cov, _dp)))
        return cov[:nb].reshape(-1, 7, 7).transpose(0, 2, 1).copy()

    def covariances(self, pairs, lam=0.0):
        """Blocks (a, b) of (H + lam I)^-1 for ANY pairs of free vertices [(id_a, id_b), ...]: (n, 7, 7), laid out
        as marginals() returns them (and the same bits for the pairs marginals() accepts)."""
        pr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        a, b = _i32(pr[:, 0]), _i32(pr[:, 1])
        n = pr.shape[0]
        cov = np.empty((max(n, 1), 49))
        self._chk(self._L.sim3opt_covariances(self._g, float(lam), n, _p(a, _ip), _p(b, _ip), _p(cov, _dp)))
        return cov[:n].reshape(-1, 7, 7).transpose(0, 2, 1).copy()

    def covariance_stats(self):
        """What the last marginals / covariances / gate_edges call did, as a dict."""
        o = (C.c_int64 * 6)()
        self._chk(self._L.sim3opt_covariance_stats(self._g, o))
        keys = ("chunks", "paths", "off_pattern_pairs", "on_pattern_pairs", "workspace_bytes", "selinv")
        return dict(zip(keys, (int(x) for x in o)))

    def covariance_columns_plan(self, pairs):
        """The vertex ids, in the order chosen, whose columns of (H + lam I)^-1 cov_solver = 1 would solve for
        covariances(pairs): a greedy cover of the pairs; host only, may be called before initialize."""
        pr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        a, b = _i32(pr[:, 0]), _i32(pr[:, 1])
        nv = C.c_int32()
        self._chk(self._L.sim3opt_covariance_columns_plan(self._g, pr.shape[0], _p(a, _ip), _p(b, _ip), C.byref(nv), None))
        out = np.zeros(max(nv.value, 1), dtype=np.int32)
        self._chk(self._L.sim3opt_covariance_columns_plan(self._g, pr.shape[0], _p(a, _ip), _p(b, _ip), C.byref(nv),
                                                          _p(out, _ip)))
        return out[:nv.value].copy()

    def covariance_columns_stats(self):
        """What the last covariances / gate_edges call that went by columns of the inverse did, as a dict."""
        c = (C.c_int64 * 5)()
        r = np.zeros(2)
        self._chk(self._L.sim3opt_covariance_columns_stats(self._g, c, _p(r, _dp)))
        out = dict(zip(("vertices", "columns", "pcg_iters", "refinements", "batches"), (int(x) for x in c)))
        out.update(max_rel_residual=float(r[0]), cov_rel_tol=float(r[1]))
        return out

    def gate_edges(self, v0, v1, meas, info=None, lam=0.0, out=None):
        """Chi-square gate of candidate edges that are not added: (e (n, 7), S (n, 7, 7), d2 (n,)) with
        S = J Sigma J^T + info^-1 and d2 = e^T S^-1 e at the current estimates.  out: (e, S49, d2) arrays the
        library writes into (S49: (n, 49) column-major blocks), returned as they are."""
        a, b = _i32(np.atleast_1d(v0)), _i32(np.atleast_1d(v1))
        n = a.shape[0]
        m = _f64(meas).reshape(-1, 8)
        inf = None
        if info is not None:  # (n, 7, 7) [k, r, c] -> column-major blocks
            inf = _f64(np.asarray(info).reshape(-1, 7, 7).transpose(0, 2, 1)).reshape(-1, 49)
        if out is None:
            e, S, d2 = np.empty((max(n, 1), 7)), np.empty((max(n, 1), 49)), np.empty(max(n, 1))
        else:
            e, S, d2 = out
        self._chk(self._L.sim3opt_gate_edges(self._g, float(lam), n, _p(a, _ip), _p(b, _ip), _p(m, _dp),
                                             _p(inf, _dp), _p(e, _dp), _p(S, _dp), _p(d2, _dp)))
        if out is not None:
            return out
        return e[:n].copy(), S[:n].reshape(-1, 7, 7).transpose(0, 2, 1).copy(), d2[:n].copy()

    def marginal_plan(self, max_pairs=0):
        """Plan of the selected inversion (on the factor's plan) as a dict of numpy arrays; host only."""
        dims = np.zeros(6, dtype=np.int64)
        dp = dims.ctypes.data_as(C.POINTER(C.c_int64))
        self._chk(self._L.sim3opt_marginal_plan(self._g, int(max_pairs), dp, *([None] * 9)))
        nb, nL, nprod, height, ngroups, nlev = (int(x) for x in dims)
        arr = dict(perm=nb, colptr=nb + 1, lrow=nL, gptr=ngroups + 1, lcolp=nlev + 1, zptr=nL + 1,
                   za=nprod, zt=nprod, zl=nprod)
        out = {k: np.zeros(max(n, 1), dtype=np.int32) for k, n in arr.items()}
        self._chk(self._L.sim3opt_marginal_plan(self._g, int(max_pairs), dp, *[_p(out[k], _ip) for k in arr]))
        out = {k: out[k][:n] for k, n in arr.items()}
        out.update(nb=nb, nL=nL, nprod=nprod, height=height, ngroups=ngroups, nlevels=nlev)
        return out

    def amg_hierarchy(self):
        """(rows per level, blocks per level, level-1 row of every level-0 block row); host only."""
        nl = C.c_int32()
        rows = np.zeros(16, dtype=np.int32)
        blocks = np.zeros(16, dtype=np.int64)
        nfree = self.num_vertices
        agg = np.full(nfree, -1, dtype=np.int32)
        self._chk(self._L.sim3opt_amg_hierarchy(self._g, 16, C.byref(nl), _p(rows, _ip),
                                                blocks.ctypes.data_as(C.c_void_p), _p(agg, _ip)))
        return rows[:nl.value].copy(), blocks[:nl.value].copy(), agg

    # ---- diagnostic read-outs of the preconditioners (tests/test_gpu_preconditioners.py) ----
    def amg_structure(self):
        """Every level of the hierarchy `amg_hierarchy` describes, host only: a list of dict(nb, nnzb, rowptr, colidx,
        agg), agg = row of the next level for each row (None on the coarsest level)."""
        out = []
        nl = C.c_int32(1)
        level = 0
        while level < nl.value:
            nb, nnzb = C.c_int32(), C.c_int64()
            self._chk(self._L.sim3opt_amg_level_structure(self._g, level, C.byref(nl), C.byref(nb), C.byref(nnzb),
                                                          None, None, None))
            rowptr = np.zeros(nb.value + 1, dtype=np.int32)
            colidx = np.zeros(max(nnzb.value, 1), dtype=np.int32)
            agg = np.full(max(nb.value, 1), -1, dtype=np.int32)
            self._chk(self._L.sim3opt_amg_level_structure(self._g, level, None, None, None, _p(rowptr, _ip),
                                                          _p(colidx, _ip), _p(agg, _ip)))
            out.append(dict(nb=nb.value, nnzb=nnzb.value, rowptr=rowptr, colidx=colidx[:nnzb.value],
                            agg=agg[:nb.value] if level + 1 < nl.value else None))
            level += 1
        return out

    def amg_level_numbers(self, lam, level, nb, nnzb, fp32=True):
        """Numbers of one level after the set-up for `lam` (nb, nnzb: the level's sizes, from amg_structure): dict of
        rowptr, colidx, vals [k, r, c], vals32 (float32, [k, r, c]; None without fp32), Minv [i, r, c], and W, diagH
        [i, r, c] on coarse levels / P [i, r, c] on level 0."""
        rowptr = np.zeros(nb + 1, dtype=np.int32)
        colidx = np.zeros(max(nnzb, 1), dtype=np.int32)
        vals = np.zeros((max(nnzb, 1), 49))
        v32 = np.zeros((max(nnzb, 1), 49), dtype=np.float32) if fp32 else None
        Minv = np.zeros((nb, 49))
        W = np.zeros((nb, 49)) if level > 0 else None
        dH = np.zeros((nb, 49)) if level > 0 else None
        P = np.zeros((nb, 49)) if level == 0 else None
        fp = C.POINTER(C.c_float)
        self._chk(self._L.sim3opt_amg_level_numbers(
            self._g, float(lam), int(level), _p(rowptr, _ip), _p(colidx, _ip), _p(vals, _dp),
            v32.ctypes.data_as(fp) if fp32 else None, _p(W, _dp) if W is not None else None,
            _p(dH, _dp) if dH is not None else None, _p(Minv, _dp), _p(P, _dp) if P is not None else None))
        cm = lambda a: None if a is None else a.reshape(-1, 7, 7).transpose(0, 2, 1).copy()  # column-major blocks
        return dict(rowptr=rowptr, colidx=colidx[:nnzb], vals=cm(vals[:nnzb]), vals32=cm(v32[:nnzb]) if fp32 else None,
                    Minv=Minv.reshape(-1, 7, 7).copy(), W=cm(W), diagH=cm(dH), P=cm(P))

    def amg_coarsest_inverse(self, lam, nb_coarsest):
        """Dense inverse of the coarsest level for `lam`, (7 nb_c, 7 nb_c)."""
        n = 7 * int(nb_coarsest)
        A = np.zeros((n, n))
        self._chk(self._L.sim3opt_amg_coarsest_inverse(self._g, float(lam), _p(A, _dp)))
        return A

    def preconditioner_apply(self, prec, lam, r):
        """z = M^-1 r for prec 0 block-Jacobi / 1 chain segments / 2 multigrid; r: (7 nb,) or (nrhs, 7 nb); one
        set-up per call."""
        r2 = _f64(np.atleast_2d(r))
        z = np.zeros_like(r2)
        self._chk(self._L.sim3opt_preconditioner_apply(self._g, int(prec), float(lam), r2.shape[0], _p(r2, _dp),
                                                       _p(z, _dp)))
        return z.reshape(np.shape(r))

    def spmv_spans(self):
        """The span SpMV's row spans as the device holds them: wrow (4 x workgroups + 1,), wavefront w owns the block
        rows wrow[w] .. wrow[w + 1] - 1."""
        ns = C.c_int32()
        self._chk(self._L.sim3opt_spmv_spans(self._g, C.byref(ns), None))
        wrow = np.zeros(ns.value + 1, dtype=np.int32)
        self._chk(self._L.sim3opt_spmv_spans(self._g, C.byref(ns), _p(wrow, _ip)))
        return wrow

    def spmv_variant(self):
        """(chunk, non_temporal) of the one-system span SpMV in use (SIM3OPT_SPMV)."""
        ch, nt = C.c_int32(), C.c_int32()
        self._chk(self._L.sim3opt_spmv_variant(self._g, C.byref(ch), C.byref(nt)))
        return ch.value, nt.value

    def operator_apply(self, lam, p, rvec=None):
        """(q, p.q, rvec.p) of q = (H + lam I) p by the SpMV launch of a PCG iteration and the sum of its partials; p:
        (7 nb,) with a scalar lam, or (nrhs, 7 nb) with nrhs dampings (nrhs 2 .. 4: the batched launch, multigrid graphs
        only).  rvec.p is None without rvec."""
        p2 = _f64(np.atleast_2d(p))
        k = p2.shape[0]
        lams = _f64(np.broadcast_to(np.asarray(lam, dtype=np.float64), (k,)))
        r2 = None if rvec is None else _f64(np.atleast_2d(rvec))
        assert r2 is None or r2.shape == p2.shape
        q, pq = np.zeros_like(p2), np.zeros(k)
        rp = None if r2 is None else np.zeros(k)
        self._chk(self._L.sim3opt_operator_apply(self._g, k, _p(lams, _dp), _p(p2, _dp), _p(r2, _dp), _p(q, _dp),
                                                 _p(pq, _dp), _p(rp, _dp)))
        if np.ndim(p) == 1:
            return q[0], float(pq[0]), None if rp is None else float(rp[0])
        return q, pq, rp

    def partition_plan(self, world, locality=True):
        """(vertex of every block row, row_begin, boundary rows per rank, cut edges); host only."""
        nfree = C.c_int32()
        nblk = C.c_int64()
        self._chk(self._L.sim3opt_system_pattern(self._g, C.byref(nfree), C.byref(nblk), None, None))
        v = np.empty(nfree.value, dtype=np.int32)
        rb = np.empty(world + 1, dtype=np.int32)
        bnd = np.empty(world, dtype=np.int32)
        cut = C.c_int64()
        self._chk(self._L.sim3opt_partition_plan(self._g, int(world), int(bool(locality)), _p(v, _ip), _p(rb, _ip),
                                                 _p(bnd, _ip), C.byref(cut)))
        return v, rb, bnd, cut.value

    def halo_plan(self, world, rank):
        """(send_rows, send_seg, recv_rows, recv_seg) of `rank` on level 0 of the `world`-rank partition; host only."""
        ns, nr = C.c_int32(), C.c_int32()
        self._chk(self._L.sim3opt_halo_plan(self._g, int(world), int(rank), C.byref(ns), C.byref(nr), None, None,
                                            None, None))
        sr, rr = np.zeros(max(ns.value, 1), np.int32), np.zeros(max(nr.value, 1), np.int32)
        ss, rs = np.zeros(world + 1, np.int32), np.zeros(world + 1, np.int32)
        self._chk(self._L.sim3opt_halo_plan(self._g, int(world), int(rank), None, None, _p(sr, _ip), _p(ss, _ip),
                                            _p(rr, _ip), _p(rs, _ip)))
        return sr[:ns.value], ss, rr[:nr.value], rs

    def bench_spmv(self, reps=20):
        ms = C.c_double()
        self._chk(self._L.sim3opt_bench_spmv(self._g, int(reps), C.byref(ms)))
        return ms.value

    def bench_stream(self, mode, reps=20):
        ms = C.c_double()
        self._chk(self._L.sim3opt_bench_stream(self._g, int(mode), int(reps), C.byref(ms)))
        return ms.value

    # ---- reference-format I/O ----
    def load_kitti_direct(self, directory, use_one_constraint=True):
        self._chk(self._L.sim3opt_load_kitti_direct(self._g, os.fsencode(directory),
                                                    int(bool(use_one_constraint))))

    def load_kitti_gt_loops(self, directory):
        """Ground-truth poses + line 1 of every loop record: all residuals ~ 0 (a convention pin)."""
        self._chk(self._L.sim3opt_load_kitti_gt_loops(self._g, os.fsencode(directory)))

    def stepwise_scale_init(self):
        """Stage 1 of the stepwise pipeline; returns the sigma_min/sigma_max estimate."""
        r = C.c_double()
        self._chk(self._L.sim3opt_stepwise_scale_init(self._g, C.byref(r)))
        return r.value

    def write_g2o(self, path):
        self._chk(self._L.sim3opt_write_g2o(self._g, os.fsencode(path)))

    def write_poses(self, path, image_ids=None):
        ids = None if image_ids is None else _i32(image_ids)
        self._chk(self._L.sim3opt_write_poses(self._g, os.fsencode(path), _p(ids, _ip)))


def robustify(kind, delta, e2):
    """sim3opt_robustify: (rho(e2), rho'(e2)) of a robust kernel, on the host."""
    out = np.empty(2)
    rc = load().sim3opt_robustify(int(kind), float(delta), float(e2), _p(out, _dp))
    if rc != OK:
        raise Sim3OptError(rc, "robustify: unknown kind, delta not finite and > 0, or e2 < 0")
    return float(out[0]), float(out[1])


def edge_jacobian_host(meas, s0, s1, **opts):
    """sim3opt_sim3_edge_jacobian: e = log(meas s0 s1^-1) (7,) and its closed-form Jacobian J (7, 14), computed on
    the host by the code the device runs.  opts are Options fields; fix_small_angle_b defaults to 1 here."""
    opts.setdefault("fix_small_angle_b", 1)
    o = default_options(**opts)
    m, a, b = _f64(meas), _f64(s0), _f64(s1)
    assert m.shape == a.shape == b.shape == (8,)
    e, J = np.empty(7), np.empty((7, 14))
    rc = load().sim3opt_sim3_edge_jacobian(_p(m, _dp), _p(a, _dp), _p(b, _dp), C.byref(o), _p(e, _dp), _p(J, _dp))
    if rc != OK:
        raise Sim3OptError(rc, "sim3_edge_jacobian: bad state (non-finite, scale <= 0) or fix_small_angle_b != 1")
    return e, J


def dogleg_rule(scalars, delta):
    """sim3opt_dogleg_rule: the dogleg's step rule on the host, the function optimize() calls per trial.  scalars = (b.b,
    b^T H b, g.g, b.g, (Hb).g, g^T H g) for g = h_gn; returns a dict of alpha, norm_sd, norm_gn, ca, cg, norm_dl,
    linear_gain and step (1 steepest descent, 2 Gauss-Newton, 3 dogleg) for h_dl = ca b + cg h_gn."""
    s = _f64(scalars).reshape(-1)
    assert s.shape == (6,)
    m, t, st = np.empty(3), np.empty(4), C.c_int32()
    rc = load().sim3opt_dogleg_rule(_p(s, _dp), float(delta), _p(m, _dp), _p(t, _dp), C.byref(st))
    if rc != OK:
        raise Sim3OptError(rc, "dogleg_rule: null argument")
    return dict(alpha=float(m[0]), norm_sd=float(m[1]), norm_gn=float(m[2]), ca=float(t[0]), cg=float(t[1]),
                norm_dl=float(t[2]), linear_gain=float(t[3]), step=int(st.value))


def read_keyframe_bin(path):
    """dict(kf_id, Rw2c 3x3, twinc, point_ids, points_w (n,3), obs_uv (n,2))  -- LoadComboKeyFrame."""
    Lb = load()
    kf, n = C.c_int32(), C.c_int32()
    R, t = np.empty(9), np.empty(3)
    rc = Lb.sim3opt_read_keyframe_bin(os.fsencode(path), C.byref(kf), _p(R, _dp), _p(t, _dp),
                                      C.byref(n), None, None, None, 0)
    if rc != OK:
        raise Sim3OptError(rc, "read_keyframe_bin")
    ids = np.empty(max(n.value, 1), dtype=np.uint32)
    pts = np.empty((max(n.value, 1), 3))
    uv = np.empty((max(n.value, 1), 2))
    rc = Lb.sim3opt_read_keyframe_bin(os.fsencode(path), C.byref(kf), _p(R, _dp), _p(t, _dp),
                                      C.byref(n), ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      _p(pts, _dp), _p(uv, _dp), n.value)
    if rc != OK:
        raise Sim3OptError(rc, "read_keyframe_bin")
    k = n.value
    return dict(kf_id=kf.value, Rw2c=R.reshape(3, 3), twinc=t, point_ids=ids[:k], points_w=pts[:k],
                obs_uv=uv[:k])


def reanchor_points(old_Rt, new_states, points, obs_frame, obs_point, device=-1):
    """figureKITTIBA's point re-anchoring on the GPU; returns the corrected (n_points, 3) array."""
    rt = _f64(old_Rt).reshape(-1, 12)
    st = _f64(new_states).reshape(-1, 8)
    pts = _f64(points).reshape(-1, 3).copy()
    of, op = _i32(obs_frame), _i32(obs_point)
    rc = load().sim3opt_reanchor_points(rt.shape[0], _p(rt, _dp), _p(st, _dp), pts.shape[0],
                                        _p(pts, _dp), of.shape[0], _p(of, _ip), _p(op, _ip),
                                        int(device))
    if rc != OK:
        raise Sim3OptError(rc, "reanchor_points")
    return pts


def write_bal(path, Rw2c, tw2c, f_k1_k2, points, obs_cam, obs_point, obs_uv):
    """SaveBALFile (drawPTAMPoints.cpp:218-283): cameras (R_w2c row-major, t_w2c), points, observations."""
    R = _f64(Rw2c).reshape(-1, 9)
    t = _f64(tw2c).reshape(-1, 3)
    fk = _f64(f_k1_k2).reshape(3)
    pts = _f64(points).reshape(-1, 3)
    oc, op = _i32(obs_cam), _i32(obs_point)
    uv = _f64(obs_uv).reshape(-1, 2)
    rc = load().sim3opt_write_bal(os.fsencode(path), R.shape[0], _p(R, _dp), _p(t, _dp), _p(fk, _dp),
                                  pts.shape[0], _p(pts, _dp), oc.shape[0], _p(oc, _ip), _p(op, _ip),
                                  _p(uv, _dp))
    if rc != OK:
        raise Sim3OptError(rc, "write_bal")


# KITTI calibration the reference hard-codes for ba_demo (bal_example.cpp:90-91, kitti_surf.cpp:52-57)
KITTI_FOCAL, KITTI_CX, KITTI_CY = 718.856, 607.1928, 185.2157


class _Handle:
    """What BundleAdjuster, TwoViewBatch, PnpBatch, EssentialBatch, HomographyBatch, Sim3Batch, MatchBatch, PlaceBatch, VocabularyTrainer, SurfBatch, FrameStore and TrackBatch share: the C handle sim3opt_<_prefix>_* in self._b with
    its creation and destruction, the options (a ctypes Structure, _Options) and the checks of return codes."""
    _prefix = _Options = None

    def __init__(self, **options):
        self._L = load()
        self._b = self._fn("create")()
        if not self._b:
            raise MemoryError(f"sim3opt_{self._prefix}_create")
        self._opt = self._Options()
        self._fn("options_default")(C.byref(self._opt))
        if options:
            self.set_options(**options)

    def _fn(self, name):
        return getattr(self._L, f"sim3opt_{self._prefix}_{name}")

    def close(self):
        if self._b:
            self._fn("destroy")(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != OK:
            raise Sim3OptError(rc, f"{what}: {self._fn('last_error')(self._b).decode()}")

    def _count(self, n, what):
        """What optimize() / solve() return: the count the library gives, or its error raised."""
        if n < 0:
            self._chk(n, what)
        return n

    def set_options(self, **kw):
        """The defaults with `kw` over them."""
        o = self._Options()
        self._fn("options_default")(C.byref(o))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        self._chk(self._fn("set_options")(self._b, C.byref(o)), f"{self._prefix}_set_options")
        self._opt = o

    def options(self):
        return {k: getattr(self._opt, k) for k, _ in self._Options._fields_}


class BundleAdjuster(_Handle):
    """sim3opt_ba*: the reference's ba_demo (bal_example.cpp:44-243) -- SE(3) cameras + points, Huber,
    LM over the Schur complement -- on the GPU.  Mirrors the demo's flow: read a BAL file (or hand the
    arrays over), optimize(maxIterations), write the camera poses."""
    _prefix, _Options = "ba", BaOptions

    def set_problem(self, cams, points, obs_cam, obs_point, obs_uv, focal=KITTI_FOCAL, cx=KITTI_CX,
                    cy=KITTI_CY):
        cq, pts = _f64(cams).reshape(-1, 7), _f64(points).reshape(-1, 3)
        oc, op, uv = _i32(obs_cam), _i32(obs_point), _f64(obs_uv).reshape(-1, 2)
        if not (oc.shape[0] == op.shape[0] == uv.shape[0]):
            raise ValueError("observation arrays differ in length")
        self._chk(self._L.sim3opt_ba_set_problem(self._b, cq.shape[0], _p(cq, _dp), pts.shape[0],
                                                 _p(pts, _dp), oc.shape[0], _p(oc, _ip), _p(op, _ip),
                                                 _p(uv, _dp), focal, cx, cy), "ba_set_problem")

    def set_fixed_cameras(self, mask):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.shape[0] != self.dims()[0]:
            raise ValueError("one flag per camera")
        self._chk(self._L.sim3opt_ba_set_fixed_cameras(self._b, _p(m, _up)), "ba_set_fixed_cameras")

    def read_bal(self, path, focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY):
        self._chk(self._L.sim3opt_ba_read_bal(self._b, os.fsencode(path), focal, cx, cy), "ba_read_bal")

    def dims(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.sim3opt_ba_dims(self._b, C.byref(a), C.byref(b), C.byref(c)), "ba_dims")
        return a.value, b.value, c.value

    def chi2(self):
        v = C.c_double()
        self._chk(self._L.sim3opt_ba_chi2(self._b, C.byref(v)), "ba_chi2")
        return v.value

    def optimize(self, max_iters=5):
        """LM iterations performed (0 = failure, as g2o); raises when the library reports an error."""
        n = self._L.sim3opt_ba_optimize(self._b, int(max_iters))
        if n <= 0:
            msg = self._L.sim3opt_ba_last_error(self._b).decode()
            if msg:
                raise Sim3OptError(n, f"ba_optimize: {msg}")
        return n

    def cameras(self):
        nc = self.dims()[0]
        out = np.empty((nc, 7))
        self._chk(self._L.sim3opt_ba_get_cameras(self._b, _p(out, _dp)), "ba_get_cameras")
        return out

    def points(self):
        n = self.dims()[1]
        out = np.empty((n, 3))
        self._chk(self._L.sim3opt_ba_get_points(self._b, _p(out, _dp)), "ba_get_points")
        return out

    def stats(self):
        out = []
        for i in range(self._L.sim3opt_ba_num_iterations(self._b)):
            st = IterStats()
            self._chk(self._L.sim3opt_ba_get_stats(self._b, i, C.byref(st)), "ba_get_stats")
            out.append({k: getattr(st, k) for k, _ in IterStats._fields_})
        return out

    def write_poses(self, path):
        self._chk(self._L.sim3opt_ba_write_poses(self._b, os.fsencode(path)), "ba_write_poses")

    # ---- covariances (sim3opt_ba_covariances): Sigma = (H + lam I)^-1 at the current estimates, fixed cameras removed;
    # an optimize() after a call computes bit for bit what it computes without it ----
    def covariances(self, cam_pairs=None, points=None, point_cams=None, lam=0.0):
        """Blocks of the covariance in one linearisation, factorisation and selected inversion: cam_pairs (n, 2) ->
        (n, 6, 6) blocks [omega, upsilon] x [omega, upsilon] (a camera with itself, or two cameras on the pattern of the
        factor: any two that share a point); points (n,) -> (n, 3, 3); point_cams (n, 2) rows (point, camera) ->
        (n, 3, 6).  A fixed camera gives exact zeros.  Returns (cc, pp, pc), None for a request not made.  lam >= 0 is
        added to every diagonal entry; a singular system (no fixed camera, a point seen once, ...) raises ERR_STATE."""
        def pairs(a):
            a = _i32(a).reshape(-1, 2)
            return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
        ca = cb = pt = qp = qc = cc = pp = pc = None
        ncc = npp = npc = 0
        if cam_pairs is not None:
            ca, cb = pairs(cam_pairs)
            ncc, cc = ca.shape[0], np.empty((ca.shape[0], 36))
        if points is not None:
            pt = _i32(points).reshape(-1)
            npp, pp = pt.shape[0], np.empty((pt.shape[0], 9))
        if point_cams is not None:
            qp, qc = pairs(point_cams)
            npc, pc = qp.shape[0], np.empty((qp.shape[0], 18))
        self._chk(self._L.sim3opt_ba_covariances(self._b, float(lam), ncc, _p(ca, _ip), _p(cb, _ip), _p(cc, _dp), npp,
                                                 _p(pt, _ip), _p(pp, _dp), npc, _p(qp, _ip), _p(qc, _ip), _p(pc, _dp)),
                  "ba_covariances")
        # column-major blocks: [q, r, c] is the transpose of the raw [q, c, r]
        t = lambda a, r, c: None if a is None else np.ascontiguousarray(a.reshape(-1, c, r).transpose(0, 2, 1))
        return t(cc, 6, 6), t(pp, 3, 3), t(pc, 3, 6)

    def camera_covariances(self, lam=0.0):
        """(n_cams, 6, 6): every camera's own block (zeros for a fixed camera)."""
        c = np.arange(self.dims()[0])
        return self.covariances(cam_pairs=np.stack([c, c], axis=1), lam=lam)[0]

    def point_covariances(self, lam=0.0):
        """(n_points, 3, 3): every point's own block."""
        return self.covariances(points=np.arange(self.dims()[1]), lam=lam)[1]

    def covariance_stats(self):
        """Of the last covariances(): dict of columns, blocks, factor_products, selinv_products, point_pair_terms, selinv."""
        o = (C.c_int64 * 6)()
        self._chk(self._L.sim3opt_ba_covariance_stats(self._b, o), "ba_covariance_stats")
        keys = ("columns", "blocks", "factor_products", "selinv_products", "point_pair_terms", "selinv")
        return dict(zip(keys, (int(x) for x in o)))

    def covariance_plan(self):
        """The pattern of the covariances' factor: dict of nb, nL, ngroups, perm (nb), colptr (nb + 1), lrow (nL)."""
        nb, ng, nl = C.c_int32(), C.c_int32(), C.c_int64()
        f = self._L.sim3opt_ba_covariance_plan
        self._chk(f(self._b, C.byref(nb), C.byref(nl), C.byref(ng), None, None, None), "ba_covariance_plan")
        perm, colptr = np.empty(nb.value, dtype=np.int32), np.empty(nb.value + 1, dtype=np.int32)
        lrow = np.empty(nl.value, dtype=np.int32)
        self._chk(f(self._b, C.byref(nb), C.byref(nl), C.byref(ng), _p(perm, _ip), _p(colptr, _ip), _p(lrow, _ip)),
                  "ba_covariance_plan")
        return dict(nb=nb.value, nL=nl.value, ngroups=ng.value, perm=perm, colptr=colptr, lrow=lrow)

    # ---- diagnostic read-outs (sim3opt_ba_debug_*): nothing in the solver uses them, and an optimize() after one of
    # them computes bit for bit what it computes without it ----
    def debug_pattern(self):
        """(rptr, bcol) of the reduced camera system's block-CSR pattern, the diagonal block first in every row."""
        n = C.c_int32()
        self._chk(self._L.sim3opt_ba_debug_pattern(self._b, C.byref(n), None, None), "ba_debug_pattern")
        rptr, bcol = np.empty(self.dims()[0] + 1, dtype=np.int32), np.empty(n.value, dtype=np.int32)
        self._chk(self._L.sim3opt_ba_debug_pattern(self._b, C.byref(n), _p(rptr, _ip), _p(bcol, _ip)),
                  "ba_debug_pattern")
        return rptr, bcol

    def debug_linearization(self):
        """lin (n_obs, 20) = [A (2x6), B (2x3), es (2)] of the current estimate, as k_ba_obs writes it."""
        lin = np.empty((self.dims()[2], 20))
        self._chk(self._L.sim3opt_ba_debug_linearization(self._b, _p(lin, _dp)), "ba_debug_linearization")
        return lin

    def debug_reduced(self, lam):
        """The reduced system of an LM trial with damping lam: dict of S (nblk, 7, 7) [k, r, c], g, b_c (nc, 7),
        Hpp_inv (np, 3, 3), b_p (np, 3), Z (no, 6, 3), point_maxdiag (np,), cam_maxdiag (nc, 7), maxdiag, and the
        pattern rptr, bcol."""
        nc, npt, no = self.dims()
        rptr, bcol = self.debug_pattern()
        nblk = bcol.shape[0]
        S, g, bc = np.empty((nblk, 49)), np.empty((nc, 7)), np.empty((nc, 7))
        Hi, bp, Z = np.empty((npt, 3, 3)), np.empty((npt, 3)), np.empty((no, 6, 3))
        pd, cd, md = np.empty(npt), np.empty((nc, 7)), C.c_double()
        self._chk(self._L.sim3opt_ba_debug_reduced(self._b, float(lam), _p(S, _dp), _p(g, _dp), _p(bc, _dp),
                                                   _p(Hi, _dp), _p(bp, _dp), _p(Z, _dp), _p(pd, _dp), _p(cd, _dp),
                                                   C.byref(md)), "ba_debug_reduced")
        # stored column-major (entry (r, c) at r + 7 c): [k, r, c] is the transpose of the raw [k, c, r]
        return dict(S=np.ascontiguousarray(S.reshape(nblk, 7, 7).transpose(0, 2, 1)), g=g, b_c=bc, Hpp_inv=Hi, b_p=bp,
                    Z=Z, point_maxdiag=pd, cam_maxdiag=cd, maxdiag=md.value, rptr=rptr, bcol=bcol)

    def debug_step(self, lam, solver=1, pcg_max_iters=0, pcg_rel_tol=1e-12):
        """The step of an LM trial with damping lam: solver 1 the exact block Cholesky, 0 k_ba_pcg with the given cap
        (the iterate x_k) and tolerance.  dict of dx_c (nc, 7), dx_p (np, 3), iters, rel, fail."""
        nc, npt, _ = self.dims()
        xc, xp = np.empty((nc, 7)), np.empty((npt, 3))
        it, fail, rel = C.c_int32(), C.c_int32(), C.c_double()
        self._chk(self._L.sim3opt_ba_debug_step(self._b, float(lam), int(solver), int(pcg_max_iters),
                                                float(pcg_rel_tol), _p(xc, _dp), _p(xp, _dp), C.byref(it),
                                                C.byref(rel), C.byref(fail)), "ba_debug_step")
        return dict(dx_c=xc, dx_p=xp, iters=it.value, rel=rel.value, fail=fail.value)

    def debug_update(self, dx_c, dx_p, lam=0.0, fail=False):
        """What an LM trial makes of the step dx_c (nc, 7), dx_p (np, 3): dict of cams (nc, 7), points (np, 3), chi2
        of that estimate and scale = x . (lam x + b).  The estimate is restored afterwards."""
        nc, npt, _ = self.dims()
        xc, xp = _f64(dx_c).reshape(-1), _f64(dx_p).reshape(-1)
        if xc.shape[0] != 7 * nc or xp.shape[0] != 3 * npt:
            raise ValueError("dx_c holds 7 numbers per camera, dx_p 3 per point")
        cams, pts = np.empty((nc, 7)), np.empty((npt, 3))
        chi, sc = C.c_double(), C.c_double()
        self._chk(self._L.sim3opt_ba_debug_update(self._b, _p(xc, _dp), _p(xp, _dp), float(lam), int(bool(fail)),
                                                  _p(cams, _dp), _p(pts, _dp), C.byref(chi), C.byref(sc)),
                  "ba_debug_update")
        return dict(cams=cams, points=pts, chi2=chi.value, scale=sc.value)


class TwoViewBatch(_Handle):
    """sim3opt_ba_batch*: the loop detector's two-view refinement (BAOptimize, kittiDetector.h:845-954) of a whole
    batch of loop candidates in one kernel launch -- camera 0 fixed, camera 1 and the points refined, Huber, LM with
    the detector's settings (lambda_0 = 50, 5 trials, 10 iterations).  Problem k owns the points
    point_ptr[k]:point_ptr[k+1] of the flat arrays."""
    _prefix, _Options = "ba_batch", BaBatchOptions

    def set_problems(self, point_ptr, cam0, cam1, points, uv0, uv1, focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY):
        ptr = _i32(point_ptr).reshape(-1)
        c0, c1 = _f64(cam0).reshape(-1, 7), _f64(cam1).reshape(-1, 7)
        pts, a, b = _f64(points).reshape(-1, 3), _f64(uv0).reshape(-1, 2), _f64(uv1).reshape(-1, 2)
        n = ptr.shape[0] - 1
        if n >= 1 and not (c0.shape[0] == c1.shape[0] == n):
            raise ValueError("one camera pair per problem")
        if n >= 1 and not (pts.shape[0] == a.shape[0] == b.shape[0] and pts.shape[0] >= ptr.max()):
            raise ValueError("point and observation arrays shorter than point_ptr says")
        self._chk(self._L.sim3opt_ba_batch_set_problems(self._b, n, _p(ptr, _ip), _p(c0, _dp), _p(c1, _dp),
                                                        _p(pts, _dp), _p(a, _dp), _p(b, _dp), focal, cx, cy),
                  "ba_batch_set_problems")

    def dims(self):
        """(problems, points of all problems)"""
        a, b = C.c_int32(), C.c_int32()
        self._chk(self._L.sim3opt_ba_batch_dims(self._b, C.byref(a), C.byref(b)), "ba_batch_dims")
        return a.value, b.value

    def optimize(self):
        """Problems optimised (one launch); raises when the library reports an error."""
        return self._count(self._L.sim3opt_ba_batch_optimize(self._b), "ba_batch_optimize")

    def cameras(self):
        """(cam0 as given, cam1), n x 7 each"""
        n = self.dims()[0]
        c0, c1 = np.empty((n, 7)), np.empty((n, 7))
        self._chk(self._L.sim3opt_ba_batch_get_cameras(self._b, _p(c0, _dp), _p(c1, _dp)), "ba_batch_get_cameras")
        return c0, c1

    def points(self):
        out = np.empty((self.dims()[1], 3))
        self._chk(self._L.sim3opt_ba_batch_get_points(self._b, _p(out, _dp)), "ba_batch_get_points")
        return out

    def num_iterations(self):
        return np.array([self._L.sim3opt_ba_batch_num_iterations(self._b, k) for k in range(self.dims()[0])],
                        dtype=np.int32)

    def stats(self, problem):
        out = []
        for i in range(self._L.sim3opt_ba_batch_num_iterations(self._b, int(problem))):
            st = IterStats()
            self._chk(self._L.sim3opt_ba_batch_get_stats(self._b, int(problem), i, C.byref(st)), "ba_batch_get_stats")
            out.append({k: getattr(st, k) for k in ("chi2_before", "chi2_after", "lambda_", "rho", "trials")})
        return out

    def lambda_init(self):
        out = np.empty(self.dims()[0])
        self._chk(self._L.sim3opt_ba_batch_get_lambda_init(self._b, _p(out, _dp)), "ba_batch_get_lambda_init")
        return out

    def chi2(self):
        """dict: active_before, active_after (n), edge_chi2 (total x 2), n_outlier_edges (n)"""
        n, t = self.dims()
        ab, aa, ec, no = np.empty(n), np.empty(n), np.empty((t, 2)), np.empty(n, dtype=np.int32)
        self._chk(self._L.sim3opt_ba_batch_get_chi2(self._b, _p(ab, _dp), _p(aa, _dp), _p(ec, _dp), _p(no, _ip)),
                  "ba_batch_get_chi2")
        return dict(active_before=ab, active_after=aa, edge_chi2=ec, n_outlier_edges=no)

    # ---- diagnostic read-out (sim3opt_ba_batch_debug_trial): nothing in the solver uses it, and an optimize() after
    # it computes bit for bit what it computes without it ----
    # name -> (first row, rows) of the per-point scratch; name -> (first, count) of a problem's row
    TRIAL_POINT_ROWS = dict(H_pp=(0, 6), b_p=(6, 3), A1=(9, 12), B1=(21, 6), es1=(27, 2), Hpp_inv=(29, 6), Z=(35, 18),
                            trial_points=(53, 3))
    TRIAL_PROBLEM_ROWS = dict(AtA=(0, 21), b_c=(21, 6), chi2=(27, 1), active_chi2=(28, 1), maxdiag=(29, 1),
                              ZY=(30, 21), Zb=(51, 6), S=(57, 21), g=(78, 6), dx_c=(84, 6), fail=(90, 1), cam=(91, 7),
                              chi2_new=(98, 1), scale=(99, 1))

    def debug_trial(self, lam, dx_c=None):
        """One LM trial of every problem at the current estimate, damping lam (one per problem, or one for all); with
        dx_c (n x 6) the back-substitution and the trial estimate use that camera step.  dict, per point: H_pp (t, 6:
        xx xy xz yy yz zz, undamped), b_p (t, 3), A1 (t, 2, 6), B1 (t, 2, 3), es1 (t, 2), Hpp_inv (t, 6), Z (t, 6, 3),
        trial_points (t, 3); per problem: AtA, ZY = -sum Z Y^T, S (n, 21: upper triangles row by row), b_c, Zb =
        -sum Z b_p, g, dx_c (n, 6), chi2, active_chi2, maxdiag, chi2_new, scale (n), fail (n, bool), cam (n, 7)."""
        n, t = self.dims()
        lam = np.ascontiguousarray(np.broadcast_to(_f64(lam).reshape(-1), (n,)) if np.size(lam) == 1 else
                                   _f64(lam).reshape(-1))
        if lam.shape[0] != n:
            raise ValueError("one lambda per problem")
        step = None
        if dx_c is not None:
            step = _f64(dx_c).reshape(-1)
            if step.shape[0] != 6 * n:
                raise ValueError("dx_c holds 6 numbers per problem")
        rows, prob = np.empty((56, max(t, 1))), np.empty((max(n, 1), 100))
        self._chk(self._L.sim3opt_ba_batch_debug_trial(self._b, _p(lam, _dp), _p(step, _dp), _p(rows, _dp),
                                                       _p(prob, _dp)), "ba_batch_debug_trial")
        shape = dict(A1=(t, 2, 6), B1=(t, 2, 3), Z=(t, 6, 3))
        out = {k: np.ascontiguousarray(rows[a:a + c].T).reshape(shape.get(k, (t, c)))
               for k, (a, c) in self.TRIAL_POINT_ROWS.items()}
        for k, (a, c) in self.TRIAL_PROBLEM_ROWS.items():
            out[k] = prob[:, a].copy() if c == 1 else prob[:, a:a + c].copy()
        out["fail"] = out["fail"] != 0
        return out


class _RansacBatch(_Handle):
    """What PnpBatch, EssentialBatch, HomographyBatch and Sim3Batch share (csrc/ransac_frame.hpp): a batch of problems, each owning the rows
    point_ptr[k]:point_ptr[k+1] of two flat arrays; one launch makes `iterations` hypotheses per problem from samples
    of _sample points, scores every one and keeps the best model (of shape _model, under the key _key)."""
    _sample = _model = _key = None
    _dims_extra = ()  # what the stage's dims takes after the two counts

    def _set_problems(self, point_ptr, a, b, focal, cx, cy, what):
        ptr = _i32(point_ptr).reshape(-1)
        n = ptr.shape[0] - 1
        if n >= 1 and not (a.shape[0] == b.shape[0] and a.shape[0] >= ptr.max()):
            raise ValueError(f"{what} arrays shorter than point_ptr says")
        self._chk(self._fn("set_problems")(self._b, n, _p(ptr, _ip), _p(a, _dp), _p(b, _dp), focal, cx, cy),
                  f"{self._prefix}_set_problems")

    def dims(self):
        """(problems, points of all problems)"""
        a, b = C.c_int32(), C.c_int32()
        self._chk(self._fn("dims")(self._b, C.byref(a), C.byref(b), *self._dims_extra), f"{self._prefix}_dims")
        return a.value, b.value

    def solve(self):
        """Problems with status 0 (one launch); raises when the library reports an error."""
        return self._count(self._fn("solve")(self._b), f"{self._prefix}_solve")

    def inliers(self):
        """(mask (total,) uint8, n_inliers (n,))"""
        n, t = self.dims()
        m, c = np.empty(t, dtype=np.uint8), np.empty(n, dtype=np.int32)
        self._chk(self._fn("get_inliers")(self._b, _p(m, _up), _p(c, _ip)), f"{self._prefix}_get_inliers")
        return m, c

    def debug_hypotheses(self, problem):
        """What the last solve computed for `problem`: dict of sample (H, _sample), n_solutions, valid, count (H,), the
        models (H, *_model) under _key, cost (H,)."""
        H = self._opt.iterations
        i = lambda *s: np.empty(s, dtype=np.int32)
        sm, ns, va, mo, co, cs = i(H, self._sample), i(H), i(H), np.empty((H,) + self._model), i(H), np.empty(H)
        self._chk(self._fn("debug_hypotheses")(self._b, int(problem), _p(sm, _ip), _p(ns, _ip), _p(va, _ip),
                                               _p(mo, _dp), _p(co, _ip), _p(cs, _dp)),
                  f"{self._prefix}_debug_hypotheses")
        return {"sample": sm, "n_solutions": ns, "valid": va, self._key: mo, "count": co, "cost": cs}

    def debug_score(self, models):
        """models (n, P, *_model) through the kernel's scoring: (count (n, P) int32, cost (n, P))"""
        n = self.dims()[0]
        q = _f64(models).reshape(n, -1, int(np.prod(self._model)))
        P = q.shape[1]
        co, cs = np.empty((n, P), dtype=np.int32), np.empty((n, P))
        self._chk(self._fn("debug_score")(self._b, P, _p(q, _dp), _p(co, _ip), _p(cs, _dp)),
                  f"{self._prefix}_debug_score")
        return co, cs


class _PoseRansacBatch(_RansacBatch):
    """... whose result is a rigid pose (PnpBatch, EssentialBatch, HomographyBatch; Sim3Batch's is a similarity)"""

    def poses(self):
        """(n, 7) [qx qy qz qw tx ty tz]"""
        out = np.empty((self.dims()[0], 7))
        self._chk(self._fn("get_poses")(self._b, _p(out, _dp)), f"{self._prefix}_get_poses")
        return out


PNP_OK, PNP_FEW_POINTS, PNP_NO_HYPOTHESIS, PNP_FEW_INLIERS = 0, 1, 2, 3


class PnpBatch(_PoseRansacBatch):
    """sim3opt_pnp_batch*: the loop detector's start pose (cv::solvePnPRansac, kittiDetector.h:1300-1301) of a whole
    batch of loop candidates in one kernel launch -- P3P hypotheses from a reproducible sampler, every one scored,
    an LM refit over the best one's inliers.  Problem k owns the points point_ptr[k]:point_ptr[k+1] of the flat
    arrays; poses() is the cam1 TwoViewBatch.set_problems takes."""
    _prefix, _Options = "pnp_batch", PnpBatchOptions
    _sample, _model, _key = 4, (7,), "pose"  # (poses() is cam1)

    def set_problems(self, point_ptr, points, uv1, focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY):
        self._set_problems(point_ptr, _f64(points).reshape(-1, 3), _f64(uv1).reshape(-1, 2), focal, cx, cy,
                           "point and observation")

    def summary(self):
        """dict of (n,) arrays: status, best_hypothesis, n_inliers_hypothesis, cost_hypothesis, rms_px,
        refine_iterations"""
        n = self.dims()[0]
        i = lambda: np.empty(n, dtype=np.int32)
        st, bh, nh, ch, rm, ri = i(), i(), i(), np.empty(n), np.empty(n), i()
        self._chk(self._L.sim3opt_pnp_batch_get_summary(self._b, _p(st, _ip), _p(bh, _ip), _p(nh, _ip), _p(ch, _dp),
                                                        _p(rm, _dp), _p(ri, _ip)), "pnp_batch_get_summary")
        return dict(status=st, best_hypothesis=bh, n_inliers_hypothesis=nh, cost_hypothesis=ch, rms_px=rm,
                    refine_iterations=ri)

    def debug_refine(self, poses, mask):
        """The kernel's refit from poses (n, 7) on mask (total,): dict of pose (n, 7), iterations (n,), chi2 (n, 2:
        before, after), trials (n, refine_iters)."""
        n, t = self.dims()
        q = _f64(poses).reshape(-1)
        m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        if q.shape[0] != 7 * n or m.shape[0] != t:
            raise ValueError("poses holds 7 numbers per problem, mask one entry per point")
        po, it, ch = np.empty((n, 7)), np.empty(n, dtype=np.int32), np.empty((n, 2))
        tr = np.zeros((n, self._opt.refine_iters), dtype=np.int32)
        self._chk(self._L.sim3opt_pnp_batch_debug_refine(self._b, _p(q, _dp), _p(m, _up), _p(po, _dp), _p(it, _ip),
                                                         _p(ch, _dp), _p(tr, _ip)), "pnp_batch_debug_refine")
        return dict(pose=po, iterations=it, chi2=ch, trials=tr)


def median_depth_ratio(point_ptr, depth0, depth1):
    """sim3opt_median_depth_ratio: per problem, the element at index floor(0.5 n) of the sorted depth1 over that of the
    sorted depth0 (kittiDetector.h:1305-1311).  Host only."""
    ptr = _i32(point_ptr).reshape(-1)
    a, b = _f64(depth0).reshape(-1), _f64(depth1).reshape(-1)
    n = ptr.shape[0] - 1
    if n >= 1 and not (a.shape[0] == b.shape[0] and a.shape[0] >= ptr.max()):
        raise ValueError("depth arrays shorter than point_ptr says")
    out = np.empty(max(n, 0))
    rc = load().sim3opt_median_depth_ratio(n, _p(ptr, _ip), _p(a, _dp), _p(b, _dp), _p(out, _dp))
    if rc != OK:
        raise Sim3OptError(rc, "median_depth_ratio")
    return out


ESSENTIAL_OK, ESSENTIAL_FEW_POINTS, ESSENTIAL_NO_HYPOTHESIS, ESSENTIAL_NO_POSE = 0, 1, 2, 3


class EssentialBatch(_PoseRansacBatch):
    """sim3opt_essential_batch*: the loop detector's essential matrix and relative pose (ExtractCameras,
    kittiDetector.h:279-293: cv::findEssentialMat + cv::recoverPose) of a whole batch of loop candidates in one kernel
    launch -- five-point hypotheses from a reproducible sampler, every one scored by its Sampson inliers, the best
    one's four pose candidates voted on by its inliers.  Problem k owns the correspondences
    point_ptr[k]:point_ptr[k+1] of uv0 / uv1: exactly MatchBatch's match_ptr, uv0, uv1."""
    _prefix, _Options = "essential_batch", EssentialBatchOptions
    # (poses() is Rc12c2, tc1inc2 (X1 = R X0 + t) with |t| = 1; inliers() are those of the best hypothesis that voted
    # for the winning candidate)
    _sample, _model, _key, _dims_extra = 6, (3, 3), "E", (None,)

    def set_problems(self, point_ptr, uv0, uv1, focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY):
        self._set_problems(point_ptr, _f64(uv0).reshape(-1, 2), _f64(uv1).reshape(-1, 2), focal, cx, cy, "observation")

    def tiles(self):
        """(points staged in LDS at most, hypotheses of a chunk): the sizes at which the kernel takes another path"""
        t = np.zeros(2, dtype=np.int32)
        self._chk(self._L.sim3opt_essential_batch_dims(self._b, None, None, _p(t, _ip)), "essential_batch_dims")
        return int(t[0]), int(t[1])

    def essentials(self):
        """(n, 3, 3), Frobenius norm 1: x1^T E x0 = 0 in normalised coordinates"""
        out = np.empty((self.dims()[0], 3, 3))
        self._chk(self._L.sim3opt_essential_batch_get_essentials(self._b, _p(out, _dp)),
                  "essential_batch_get_essentials")
        return out

    def summary(self):
        """dict of (n,) arrays: status, best_hypothesis, n_inliers_hypothesis, cost_hypothesis, winner, votes_winner,
        and votes (n, 4)"""
        n = self.dims()[0]
        i = lambda *s: np.empty((n,) + s, dtype=np.int32)
        st, bh, nh, ch, wi, vw, vo = i(), i(), i(), np.empty(n), i(), i(), i(4)
        self._chk(self._L.sim3opt_essential_batch_get_summary(self._b, _p(st, _ip), _p(bh, _ip), _p(nh, _ip),
                                                              _p(ch, _dp), _p(wi, _ip), _p(vw, _ip), _p(vo, _ip)),
                  "essential_batch_get_summary")
        return dict(status=st, best_hypothesis=bh, n_inliers_hypothesis=nh, cost_hypothesis=ch, winner=wi,
                    votes_winner=vw, votes=vo)

    def debug_pose(self, essentials, mask):
        """The kernel's pose step on essentials (n, 3, 3) and mask (total,): dict of candidates (n, 4, 7), votes
        (n, 4), winner (n,), mask (total,) narrowed to the winner's voters."""
        n, t = self.dims()
        e = _f64(essentials).reshape(-1)
        m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        if e.shape[0] != 9 * n or m.shape[0] != t:
            raise ValueError("essentials holds 9 numbers per problem, mask one entry per point")
        ca, vo, wi = np.empty((n, 4, 7)), np.empty((n, 4), dtype=np.int32), np.empty(n, dtype=np.int32)
        mo = np.empty(t, dtype=np.uint8)
        self._chk(self._L.sim3opt_essential_batch_debug_pose(self._b, _p(e, _dp), _p(m, _up), _p(ca, _dp), _p(vo, _ip),
                                                             _p(wi, _ip), _p(mo, _up)), "essential_batch_debug_pose")
        return dict(candidates=ca, votes=vo, winner=wi, mask=mo)


HOMOGRAPHY_OK, HOMOGRAPHY_FEW_POINTS, HOMOGRAPHY_NO_HYPOTHESIS, HOMOGRAPHY_NO_INLIERS, HOMOGRAPHY_DEGENERATE = 0, 1, 2, 3, 4
HOMOGRAPHY_MAX_ROUNDS = 8


class HomographyBatch(_PoseRansacBatch):
    """sim3opt_homography_batch*: the loop detector's planar relative pose (HomographyInit::Compute,
    kittiDetector.h:1387-1443; HomographyInit.cc) of a whole batch of loop candidates in one kernel launch -- four-point
    homographies from a reproducible sampler scored by MLESAC, the best one refined on its inliers by Tukey-reweighted
    rounds, decomposed into eight (R, t, n, d) and chosen by the visibility tests and the Sampson tie-break.  Problem k
    owns the correspondences point_ptr[k]:point_ptr[k+1] of uv0 / uv1: exactly MatchBatch's match_ptr, uv0, uv1."""
    _prefix, _Options = "homography_batch", HomographyBatchOptions
    # (poses() is se3SecondFromFirst (X1 = R X0 + t), t not normalised; inliers() are mvHomographyInliers)
    _sample, _model, _key, _dims_extra = 4, (3, 3), "H", (None,)

    def set_problems(self, point_ptr, uv0, uv1, focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY):
        self._set_problems(point_ptr, _f64(uv0).reshape(-1, 2), _f64(uv1).reshape(-1, 2), focal, cx, cy, "observation")

    def tiles(self):
        """(points staged in LDS at most, hypotheses of a chunk): the sizes at which the kernel takes another path"""
        t = np.zeros(2, dtype=np.int32)
        self._chk(self._L.sim3opt_homography_batch_dims(self._b, None, None, _p(t, _ip)), "homography_batch_dims")
        return int(t[0]), int(t[1])

    def homographies(self):
        """(mlesac (n, 3, 3) of Frobenius norm 1, refined (n, 3, 3)): second ~ H first in camera-plane coordinates"""
        n = self.dims()[0]
        a, b = np.empty((n, 3, 3)), np.empty((n, 3, 3))
        self._chk(self._L.sim3opt_homography_batch_get_homographies(self._b, _p(a, _dp), _p(b, _dp)),
                  "homography_batch_get_homographies")
        return a, b

    def summary(self):
        """dict of (n,) arrays: status, best_hypothesis, cost_hypothesis, n_inliers, choice, ambiguous, and sigma2
        (n, refine_rounds), counts_first (n, 8), kept (n, 4), counts_second (n, 4), sampson (n, 2)"""
        n = self.dims()[0]
        i = lambda *s: np.empty((n,) + s, dtype=np.int32)
        st, bh, ch, ni, sg = i(), i(), np.empty(n), i(), np.empty((n, HOMOGRAPHY_MAX_ROUNDS))
        c1, ke, c2, cho, am, sa = i(8), i(4), i(4), i(), i(), np.empty((n, 2))
        self._chk(self._L.sim3opt_homography_batch_get_summary(
            self._b, _p(st, _ip), _p(bh, _ip), _p(ch, _dp), _p(ni, _ip), _p(sg, _dp), _p(c1, _ip), _p(ke, _ip),
            _p(c2, _ip), _p(cho, _ip), _p(am, _ip), _p(sa, _dp)), "homography_batch_get_summary")
        return dict(status=st, best_hypothesis=bh, cost_hypothesis=ch, n_inliers=ni,
                    sigma2=sg[:, :self._opt.refine_rounds].copy(), counts_first=c1, kept=ke, counts_second=c2,
                    choice=cho, ambiguous=am, sampson=sa)

    def _h_and_mask(self, homographies, mask):
        n, t = self.dims()
        h = _f64(homographies).reshape(-1)
        m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        if h.shape[0] != 9 * n or m.shape[0] != t:
            raise ValueError("homographies holds 9 numbers per problem, mask one entry per point")
        return n, h, m

    def debug_refine(self, homographies, mask):
        """The kernel's refinement rounds from homographies (n, 3, 3) on mask (total,): dict of sigma2
        (n, refine_rounds) and H (n, refine_rounds, 3, 3) after every round."""
        n, h, m = self._h_and_mask(homographies, mask)
        r = self._opt.refine_rounds
        sg, hr = np.zeros((n, r)), np.zeros((n, r, 3, 3))
        self._chk(self._L.sim3opt_homography_batch_debug_refine(self._b, _p(h, _dp), _p(m, _up), _p(sg, _dp),
                                                                _p(hr, _dp)), "homography_batch_debug_refine")
        return dict(sigma2=sg, H=hr)

    def debug_decompose(self, homographies, mask):
        """The kernel's decomposition and choice of homographies (n, 3, 3) on mask (total,): dict of R (n, 8, 3, 3),
        t, normal (n, 8, 3), d (n, 8), status, choice, ambiguous (n,), counts_first (n, 8), kept, counts_second (n, 4),
        sampson (n, 2), pose (n, 7)."""
        n, h, m = self._h_and_mask(homographies, mask)
        i = lambda *s: np.empty((n,) + s, dtype=np.int32)
        de, st, c1, ke, c2, cho, am = np.empty((n, 8, 16)), i(), i(8), i(4), i(4), i(), i()
        sa, po = np.empty((n, 2)), np.empty((n, 7))
        self._chk(self._L.sim3opt_homography_batch_debug_decompose(
            self._b, _p(h, _dp), _p(m, _up), _p(de, _dp), _p(st, _ip), _p(c1, _ip), _p(ke, _ip), _p(c2, _ip),
            _p(cho, _ip), _p(am, _ip), _p(sa, _dp), _p(po, _dp)), "homography_batch_debug_decompose")
        return dict(R=de[:, :, :9].reshape(n, 8, 3, 3).copy(), t=de[:, :, 9:12].copy(), normal=de[:, :, 12:15].copy(),
                    d=de[:, :, 15].copy(), status=st, counts_first=c1, kept=ke, counts_second=c2, choice=cho,
                    ambiguous=am, sampson=sa, pose=po)


SIM3_OK, SIM3_FEW_POINTS, SIM3_NO_HYPOTHESIS, SIM3_FEW_INLIERS, SIM3_NOT_POSITIVE = 0, 1, 2, 3, 4


class Sim3Batch(_RansacBatch):
    """sim3opt_sim3_batch*: the Sim(3) measurement of a whole batch of loop candidates with its information matrix in
    one kernel launch -- Horn's closed form on three 3-D -- 3-D matches from a reproducible sampler, every hypothesis
    scored on the reprojection errors in both images, an LM refinement of the best one on its inliers, Omega over the
    final inliers.  Problem k owns the matches point_ptr[k]:point_ptr[k+1]: exactly MatchBatch's match_ptr, uv0, uv1,
    depth0, depth1.  sim3() and information() are the meas and info of Graph.add_edges / Graph.gate_edges."""
    _prefix, _Options = "sim3_batch", Sim3BatchOptions
    _sample, _model, _key, _dims_extra = 3, (8,), "sim3", (None,)

    def set_problems(self, point_ptr, uv0, uv1, depth0, depth1, focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY):
        ptr = _i32(point_ptr).reshape(-1)
        a, b = _f64(uv0).reshape(-1, 2), _f64(uv1).reshape(-1, 2)
        d0, d1 = _f64(depth0).reshape(-1), _f64(depth1).reshape(-1)
        n = ptr.shape[0] - 1
        if n >= 1 and not (a.shape[0] == b.shape[0] == d0.shape[0] == d1.shape[0] and a.shape[0] >= ptr.max()):
            raise ValueError("observation and depth arrays shorter than point_ptr says")
        self._chk(self._L.sim3opt_sim3_batch_set_problems(self._b, n, _p(ptr, _ip), _p(a, _dp), _p(b, _dp), _p(d0, _dp),
                                                          _p(d1, _dp), focal, cx, cy), "sim3_batch_set_problems")

    def tiles(self):
        """(matches staged in LDS at most, hypotheses of a chunk): the sizes at which the kernel takes another path"""
        t = np.zeros(2, dtype=np.int32)
        self._chk(self._L.sim3opt_sim3_batch_dims(self._b, None, None, _p(t, _ip)), "sim3_batch_dims")
        return int(t[0]), int(t[1])

    def sim3(self):
        """(n, 8) [qx qy qz qw tx ty tz s]: X1 ~ s R X0 + t"""
        out = np.empty((self.dims()[0], 8))
        self._chk(self._L.sim3opt_sim3_batch_get_sim3(self._b, _p(out, _dp), None), "sim3_batch_get_sim3")
        return out

    def information(self):
        """(n, 7, 7) indexed [k, r, c], tangent order [omega upsilon sigma]: what add_edges / gate_edges take as info"""
        out = np.empty((self.dims()[0], 49))
        self._chk(self._L.sim3opt_sim3_batch_get_sim3(self._b, None, _p(out, _dp)), "sim3_batch_get_sim3")
        return out.reshape(-1, 7, 7).transpose(0, 2, 1).copy()

    def summary(self):
        """dict of (n,) arrays: status, best_hypothesis, n_inliers_hypothesis, cost_hypothesis, rms_px,
        refine_iterations, and chi2 (n, 2: before, after the refinement)"""
        n = self.dims()[0]
        i = lambda: np.empty(n, dtype=np.int32)
        st, bh, nh, ch, rm, ri, c2 = i(), i(), i(), np.empty(n), np.empty(n), i(), np.empty((n, 2))
        self._chk(self._L.sim3opt_sim3_batch_get_summary(self._b, _p(st, _ip), _p(bh, _ip), _p(nh, _ip), _p(ch, _dp),
                                                         _p(rm, _dp), _p(ri, _ip), _p(c2, _dp)),
                  "sim3_batch_get_summary")
        return dict(status=st, best_hypothesis=bh, n_inliers_hypothesis=nh, cost_hypothesis=ch, rms_px=rm,
                    refine_iterations=ri, chi2=c2)

    def _sims_and_mask(self, sims, mask):
        n, t = self.dims()
        q = _f64(sims).reshape(-1)
        m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        if q.shape[0] != 8 * n or m.shape[0] != t:
            raise ValueError("sims holds 8 numbers per problem, mask one entry per match")
        return n, t, q, m

    def debug_refine(self, sims, mask):
        """The kernel's refinement from sims (n, 8) on mask (total,): dict of sim3 (n, 8), iterations (n,), chi2
        (n, 2: before, after), trials (n, refine_iters)."""
        n, t, q, m = self._sims_and_mask(sims, mask)
        po, it, ch = np.empty((n, 8)), np.empty(n, dtype=np.int32), np.empty((n, 2))
        tr = np.zeros((n, self._opt.refine_iters), dtype=np.int32)
        self._chk(self._L.sim3opt_sim3_batch_debug_refine(self._b, _p(q, _dp), _p(m, _up), _p(po, _dp), _p(it, _ip),
                                                          _p(ch, _dp), _p(tr, _ip)), "sim3_batch_debug_refine")
        return dict(sim3=po, iterations=it, chi2=ch, trials=tr)

    def debug_information(self, sims, mask):
        """Omega and the Huber weights at sims (n, 8) on mask (total,), no LM: dict of information (n, 7, 7) [k, r, c],
        weights (total, 2: image 1, image 0), positive_definite (n,)."""
        n, t, q, m = self._sims_and_mask(sims, mask)
        om, w, pd = np.empty((n, 49)), np.empty((t, 2)), np.empty(n, dtype=np.int32)
        self._chk(self._L.sim3opt_sim3_batch_debug_information(self._b, _p(q, _dp), _p(m, _up), _p(om, _dp), _p(w, _dp),
                                                               _p(pd, _ip)), "sim3_batch_debug_information")
        return dict(information=om.reshape(-1, 7, 7).transpose(0, 2, 1).copy(), weights=w, positive_definite=pd)


MATCH_OK, MATCH_NO_KEYPOINTS, MATCH_NO_MAP = 0, 1, 2
KITTI_WIDTH, KITTI_HEIGHT = 1241, 376  # (KITTI-00's images)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _store_handle(store):
    """The C handle of a FrameStore (None passes through: the library refuses a NULL store)."""
    return None if store is None else store._b


class FrameStore(_Handle):
    """sim3opt_frames*: kp_ptr / kp / desc of a sequence on one device, held once.  SurfBatch.solve_into fills it on the
    device (set() does from host arrays); VocabularyTrainer, PlaceBatch and MatchBatch read it in place through their
    set_frames_from.  What it holds is an immutable snapshot: a consumer that took it keeps it through a refill or
    the store's close()."""
    _prefix, _Options = "frames", FrameStoreOptions
    TILES = ("compact_tile", "row_lanes")

    def set(self, kp_ptr, kp, desc):
        kpp, k, d = _i32(kp_ptr).reshape(-1), _f32(kp).reshape(-1, 2), _f32(desc).reshape(-1, 64)
        n = kpp.shape[0] - 1
        if n >= 1 and not (k.shape[0] == d.shape[0] and k.shape[0] >= kpp.max()):
            raise ValueError("keypoint arrays shorter than kp_ptr says")
        if d.shape[0] == 0:  # (the C-ABI refuses a NULL array; nothing of them is read)
            k, d = np.zeros((1, 2), dtype=np.float32), np.zeros((1, 64), dtype=np.float32)
        self._chk(self._L.sim3opt_frames_set(self._b, n, _p(kpp, _ip), _p(k, _fp), _p(d, _fp)), "frames_set")

    def dims(self):
        """dict: n_frames, total_keypoints, device (-1 before a fill), desc_bytes and the compaction's tile sizes
        (TILES)"""
        v = [C.c_int32() for _ in range(3)]
        nb, t = C.c_int64(), (C.c_int32 * 2)()
        self._chk(self._L.sim3opt_frames_get_dims(self._b, *(C.byref(x) for x in v), C.byref(nb), t), "frames_get_dims")
        out = dict(zip(("n_frames", "total_keypoints", "device"), (x.value for x in v)), desc_bytes=nb.value)
        out.update(zip(self.TILES, t))
        return out

    def kp_ptr(self):
        """The host mirror of kp_ptr (nothing is read from the device)"""
        p = np.empty(self.dims()["n_frames"] + 1, dtype=np.int32)
        self._chk(self._L.sim3opt_frames_get(self._b, _p(p, _ip), None, None), "frames_get")
        return p

    def get(self):
        """(kp_ptr (n_frames + 1,), kp (N, 2), desc (N, 64)) read back from the device"""
        d = self.dims()
        p = np.empty(d["n_frames"] + 1, dtype=np.int32)
        k, e = np.empty((d["total_keypoints"], 2), dtype=np.float32), np.empty((d["total_keypoints"], 64), dtype=np.float32)
        self._chk(self._L.sim3opt_frames_get(self._b, _p(p, _ip), _p(k, _fp), _p(e, _fp)), "frames_get")
        return p, k, e

    def debug_compact(self, cand_ptr, state, slot_kp, slot_desc):
        """The ordered compaction on caller-supplied slot arrays: the store is filled with the slots of state 2."""
        cp, st = _i32(cand_ptr).reshape(-1), _i32(state).reshape(-1)
        k, d = _f32(slot_kp).reshape(-1, 2), _f32(slot_desc).reshape(-1, 64)
        n = cp.shape[0] - 1
        if n >= 1 and not (st.shape[0] == k.shape[0] == d.shape[0] and st.shape[0] >= cp.max()):
            raise ValueError("slot arrays shorter than cand_ptr says")
        if st.shape[0] == 0:
            st = np.zeros(1, dtype=np.int32)
            k, d = np.zeros((1, 2), dtype=np.float32), np.zeros((1, 64), dtype=np.float32)
        self._chk(self._L.sim3opt_frames_debug_compact(self._b, n, _p(cp, _ip), _p(st, _ip), _p(k, _fp), _p(d, _fp)),
                  "frames_debug_compact")


def _opt_array(a, conv, n, what):
    """None, or `a` as a contiguous array of n entries"""
    if a is None:
        return None
    a = conv(a).reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"{what} holds one entry per match")
    return a


def _match_arrays(pairs, match_ptr, query_idx, train_idx, mask, depth0, depth1):
    """The arrays sim3opt_track_batch_set_matches and sim3opt_track_reference take, checked for their lengths."""
    pr, mp = _i32(pairs).reshape(-1, 2), _i32(match_ptr).reshape(-1)
    q, t = _i32(query_idx).reshape(-1), _i32(train_idx).reshape(-1)
    if mp.shape[0] != pr.shape[0] + 1:
        raise ValueError("match_ptr holds one entry per pair and one more")
    M = q.shape[0]
    if t.shape[0] != M or (mp.shape[0] >= 2 and M < mp.max()):
        raise ValueError("match arrays shorter than match_ptr says")
    mk = _opt_array(mask, lambda a: np.ascontiguousarray(a, dtype=np.uint8), M, "mask")
    d0, d1 = _opt_array(depth0, _f64, M, "depth0"), _opt_array(depth1, _f64, M, "depth1")
    if M == 0:  # (the C-ABI refuses a NULL array; nothing of them is read)
        q = t = np.zeros(1, dtype=np.int32)
    return pr, mp, q, t, mk, d0, d1


def _po(a, ptr_type):
    return None if a is None else _p(a, ptr_type)


class TrackBatch(_Handle):
    """sim3opt_track_batch*: the kept matches of all loop pairs fused into multi-view tracks, one 3-D point per track in
    the corrected world and the rows BundleAdjuster.set_problem takes behind the map's (SaveAsSfMInit's connection loop,
    kitti_surf.cpp:349-391, as connected components).  set_matches takes what MatchBatch.match_ptr() / matches() return
    and a RANSAC stage's inlier mask; set_cameras what Graph.get_vertices() returns.  include/sim3opt.h says what is
    pinned on the reference's loopTracks.txt (the connection) and what has no counterpart there (the point, the gates,
    the rows)."""
    _prefix, _Options = "track_batch", TrackBatchOptions
    TILES = ("workgroup", "scan_tile", "lane_max", "wave_max")
    DIMS = ("n_frames", "n_pairs", "total_matches", "n_tracks", "n_observations", "n_kept_tracks", "n_kept_observations",
            "rounds")

    def set_frames(self, kp_ptr, kp):
        kpp, k = _i32(kp_ptr).reshape(-1), _f32(kp).reshape(-1, 2)
        n = kpp.shape[0] - 1
        if n >= 1 and k.shape[0] < kpp.max():
            raise ValueError("keypoint array shorter than kp_ptr says")
        if k.shape[0] == 0:  # (the C-ABI refuses a NULL array; nothing of it is read)
            k = np.zeros((1, 2), dtype=np.float32)
        self._chk(self._L.sim3opt_track_batch_set_frames(self._b, n, _p(kpp, _ip), _p(k, _fp)), "track_batch_set_frames")

    def set_frames_from(self, store):
        """set_frames with kp_ptr / kp read in place from a FrameStore's current snapshot"""
        self._chk(self._L.sim3opt_track_batch_set_frames_from(self._b, _store_handle(store)), "track_batch_set_frames_from")

    def set_matches(self, pairs, match_ptr, query_idx, train_idx, mask=None, depth0=None, depth1=None):
        pr, mp, q, t, mk, d0, d1 = _match_arrays(pairs, match_ptr, query_idx, train_idx, mask, depth0, depth1)
        self._chk(self._L.sim3opt_track_batch_set_matches(self._b, pr.shape[0], _p(pr, _ip), _p(mp, _ip), _p(q, _ip),
                                                          _p(t, _ip), _po(mk, _up), _po(d0, _dp), _po(d1, _dp)),
                  "track_batch_set_matches")

    def set_cameras(self, states, focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY):
        st = _f64(states).reshape(-1, 8)
        self._chk(self._L.sim3opt_track_batch_set_cameras(self._b, st.shape[0], _p(st, _dp), focal, cx, cy),
                  "track_batch_set_cameras")

    def dims(self):
        """dict: DIMS (rounds: the hook-and-jump rounds of the last solve) and the kernels' switch sizes (TILES)"""
        v = [C.c_int32() for _ in self.DIMS]
        t = (C.c_int32 * 4)()
        self._chk(self._L.sim3opt_track_batch_dims(self._b, *(C.byref(x) for x in v), t), "track_batch_dims")
        out = dict(zip(self.DIMS, (x.value for x in v)))
        out.update(zip(self.TILES, t))
        return out

    def solve(self):
        """Tracks with status 0; raises when the library reports an error."""
        return self._count(self._L.sim3opt_track_batch_solve(self._b), "track_batch_solve")

    def tracks(self):
        """dict: track_ptr (T + 1,), obs_frame, obs_keypoint (n_observations,), status, first_match (T,) and
        match_track (total_matches,), -1 where masked"""
        d = self.dims()
        T, n = d["n_tracks"], d["n_observations"]
        ptr, st, fm = np.empty(T + 1, dtype=np.int32), np.empty(T, dtype=np.int32), np.empty(T, dtype=np.int32)
        of, ok, mt = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(d["total_matches"], dtype=np.int32)
        self._chk(self._L.sim3opt_track_batch_get_tracks(self._b, _p(ptr, _ip), _p(of, _ip), _p(ok, _ip), _p(st, _ip),
                                                         _p(fm, _ip)), "track_batch_get_tracks")
        self._chk(self._L.sim3opt_track_batch_get_match_track(self._b, _p(mt, _ip)), "track_batch_get_match_track")
        return dict(track_ptr=ptr, obs_frame=of, obs_keypoint=ok, status=st, first_match=fm, match_track=mt)

    def points(self):
        """(points (T, 3), n_depths (T,))"""
        T = self.dims()["n_tracks"]
        pts, nd = np.empty((T, 3)), np.empty(T, dtype=np.int32)
        self._chk(self._L.sim3opt_track_batch_get_points(self._b, _p(pts, _dp), _p(nd, _ip)), "track_batch_get_points")
        return pts, nd

    def ba_rows(self, point_base=0):
        """dict: points (K, 3), obs_cam, obs_point (= point_base + rank), obs_uv (n, 2) of the status-0 tracks, the rows
        BundleAdjuster.set_problem takes once concatenated behind a map of point_base points"""
        d = self.dims()
        K, n = d["n_kept_tracks"], d["n_kept_observations"]
        pts, uv = np.empty((K, 3)), np.empty((n, 2))
        oc, op = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        self._chk(self._L.sim3opt_track_batch_get_ba(self._b, int(point_base), _p(pts, _dp), _p(oc, _ip), _p(op, _ip),
                                                     _p(uv, _dp)), "track_batch_get_ba")
        return dict(points=pts, obs_cam=oc, obs_point=op, obs_uv=uv)

    @staticmethod
    def reference(kp_ptr, kp, pairs, match_ptr, query_idx, train_idx, states, mask=None, depth0=None, depth1=None,
                  focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY, max_reproj_px=0.0):
        """sim3opt_track_reference, the serial restatement on the host (no device): the dict tracks() returns with
        points and n_depths added"""
        L = load()
        kpp, k, st = _i32(kp_ptr).reshape(-1), _f32(kp).reshape(-1, 2), _f64(states).reshape(-1, 8)
        if k.shape[0] == 0:
            k = np.zeros((1, 2), dtype=np.float32)
        if st.shape[0] != kpp.shape[0] - 1 or k.shape[0] < kpp.max():
            raise ValueError("one state per frame, one pixel pair per keypoint")
        pr, mp, q, t, mk, d0, d1 = _match_arrays(pairs, match_ptr, query_idx, train_idx, mask, depth0, depth1)
        M = int(mp[-1]) if mp.shape[0] else 0
        nt, no = C.c_int32(), C.c_int32()
        ptr, stt, fm, nd = (np.zeros(M + 1, dtype=np.int32) for _ in range(4))
        of, ok = np.zeros(2 * M + 1, dtype=np.int32), np.zeros(2 * M + 1, dtype=np.int32)
        mt, pts = np.zeros(M + 1, dtype=np.int32), np.zeros((M + 1, 3))
        rc = L.sim3opt_track_reference(kpp.shape[0] - 1, _p(kpp, _ip), _p(k, _fp), pr.shape[0], _p(pr, _ip), _p(mp, _ip),
                                       _p(q, _ip), _p(t, _ip), _po(mk, _up), _po(d0, _dp), _po(d1, _dp), _p(st, _dp),
                                       focal, cx, cy, max_reproj_px, C.byref(nt), C.byref(no), _p(ptr, _ip), _p(of, _ip),
                                       _p(ok, _ip), _p(stt, _ip), _p(fm, _ip), _p(mt, _ip), _p(pts, _dp), _p(nd, _ip))
        if rc != OK:
            raise Sim3OptError(rc, "track_reference: refused")
        T, n = nt.value, no.value
        return dict(track_ptr=ptr[:T + 1].copy(), obs_frame=of[:n].copy(), obs_keypoint=ok[:n].copy(),
                    status=stt[:T].copy(), first_match=fm[:T].copy(), match_track=mt[:M].copy(), points=pts[:T].copy(),
                    n_depths=nd[:T].copy())


class MatchBatch(_Handle):
    """sim3opt_match_batch*: descriptor matching with the reference's filters (kittiDetector.h:1085-1160) and the
    map-depth lookup (:1229-1279) of a whole batch of loop candidates.  Frames are handed over once, pairs name them;
    match_ptr() / matches() are the point_ptr, points, uv0 / uv1 and depths PnpBatch, TwoViewBatch and
    median_depth_ratio take."""
    _prefix, _Options = "match_batch", MatchBatchOptions
    _n_kp = _pairs = None  # set_frames / set_pairs: what debug_nn sizes its arrays by

    def set_frames(self, kp_ptr, obs_ptr, kp, desc, obs_uv, obs_depth, focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY,
                   image_width=KITTI_WIDTH, image_height=KITTI_HEIGHT):
        kpp, obp = _i32(kp_ptr).reshape(-1), _i32(obs_ptr).reshape(-1)
        k, d = _f32(kp).reshape(-1, 2), _f32(desc).reshape(-1, 64)
        ou, od = _f32(obs_uv).reshape(-1, 2), _f32(obs_depth).reshape(-1)
        n = kpp.shape[0] - 1
        if obp.shape[0] != n + 1:
            raise ValueError("kp_ptr and obs_ptr hold one entry per frame and one more")
        if n >= 1 and not (k.shape[0] == d.shape[0] and k.shape[0] >= kpp.max() and ou.shape[0] == od.shape[0]
                           and ou.shape[0] >= obp.max()):
            raise ValueError("keypoint or observation arrays shorter than their pointer arrays say")
        self._chk(self._L.sim3opt_match_batch_set_frames(self._b, n, _p(kpp, _ip), _p(obp, _ip), _p(k, _fp), _p(d, _fp),
                                                         _p(ou, _fp), _p(od, _fp), focal, cx, cy, int(image_width),
                                                         int(image_height)), "match_batch_set_frames")
        self._n_kp, self._pairs = np.diff(kpp), None  # (what debug_nn sizes its arrays by; the pairs went with the frames)

    def set_frames_from(self, store, obs_ptr, obs_uv, obs_depth, focal=KITTI_FOCAL, cx=KITTI_CX, cy=KITTI_CY,
                        image_width=KITTI_WIDTH, image_height=KITTI_HEIGHT):
        """set_frames with kp_ptr / kp / desc read in place from a FrameStore's current snapshot"""
        obp = _i32(obs_ptr).reshape(-1)
        ou, od = _f32(obs_uv).reshape(-1, 2), _f32(obs_depth).reshape(-1)
        if obp.shape[0] >= 2 and not (ou.shape[0] == od.shape[0] and ou.shape[0] >= obp.max()):
            raise ValueError("observation arrays shorter than obs_ptr says")
        if ou.shape[0] == 0:  # (the C-ABI refuses a NULL array; nothing of them is read)
            ou, od = np.zeros((1, 2), dtype=np.float32), np.zeros(1, dtype=np.float32)
        self._chk(self._L.sim3opt_match_batch_set_frames_from(
            self._b, _store_handle(store), obp.shape[0] - 1, _p(obp, _ip), _p(ou, _fp), _p(od, _fp), focal, cx, cy,
            int(image_width), int(image_height)), "match_batch_set_frames_from")
        self._n_kp, self._pairs = np.diff(store.kp_ptr()), None

    def set_pairs(self, pairs):
        p = _i32(pairs).reshape(-1, 2)
        self._chk(self._L.sim3opt_match_batch_set_pairs(self._b, p.shape[0], _p(p, _ip)), "match_batch_set_pairs")
        self._pairs = p.copy()

    def dims(self):
        """dict: n_frames, n_pairs, total_keypoints, total_observations and the kernels' tile sizes wavefront,
        query_tile, train_tile, obs_chunk"""
        v = [C.c_int32() for _ in range(4)]
        t = (C.c_int32 * 4)()
        self._chk(self._L.sim3opt_match_batch_dims(self._b, *(C.byref(x) for x in v), t), "match_batch_dims")
        return dict(n_frames=v[0].value, n_pairs=v[1].value, total_keypoints=v[2].value,
                    total_observations=v[3].value, wavefront=t[0], query_tile=t[1], train_tile=t[2], obs_chunk=t[3])

    def solve(self):
        """Pairs with status 0; raises when the library reports an error."""
        return self._count(self._L.sim3opt_match_batch_solve(self._b), "match_batch_solve")

    def match_ptr(self):
        out = np.empty(self.dims()["n_pairs"] + 1, dtype=np.int32)
        self._chk(self._L.sim3opt_match_batch_get_match_ptr(self._b, _p(out, _ip)), "match_batch_get_match_ptr")
        return out

    def matches(self):
        """dict of per-match arrays: query_idx, train_idx (int32), distance (float32), uv0, uv1 (M, 2), depth0,
        depth1 (M,), points0 (M, 3)"""
        M = int(self.match_ptr()[-1])
        q, t = np.empty(M, dtype=np.int32), np.empty(M, dtype=np.int32)
        d = np.empty(M, dtype=np.float32)
        u0, u1, z0, z1, pt = np.empty((M, 2)), np.empty((M, 2)), np.empty(M), np.empty(M), np.empty((M, 3))
        self._chk(self._L.sim3opt_match_batch_get_matches(self._b, _p(q, _ip), _p(t, _ip), _p(d, _fp), _p(u0, _dp),
                                                          _p(u1, _dp), _p(z0, _dp), _p(z1, _dp), _p(pt, _dp)),
                  "match_batch_get_matches")
        return dict(query_idx=q, train_idx=t, distance=d, uv0=u0, uv1=u1, depth0=z0, depth1=z1, points0=pt)

    def summary(self):
        """dict of (n_pairs,) arrays: status, n_nearest, n_after_ratio, n_after_filters, n_after_unique"""
        n = self.dims()["n_pairs"]
        a = [np.empty(n, dtype=np.int32) for _ in range(5)]
        self._chk(self._L.sim3opt_match_batch_get_summary(self._b, *(_p(x, _ip) for x in a)), "match_batch_get_summary")
        return dict(zip(("status", "n_nearest", "n_after_ratio", "n_after_filters", "n_after_unique"), a))

    def debug_nn(self, pair):
        """What k_match_nn wrote for every query of `pair` (the keypoints of its frame0): dict of best_idx, best_d2,
        second_idx, second_d2."""
        if self._pairs is None or not 0 <= int(pair) < self._pairs.shape[0]:
            n_query = 0  # (the library says what is wrong: no pairs, no solve, no such pair)
        else:
            n_query = int(self._n_kp[self._pairs[int(pair), 0]])
        bi, si = np.empty(n_query, dtype=np.int32), np.empty(n_query, dtype=np.int32)
        bd, sd = np.empty(n_query, dtype=np.float32), np.empty(n_query, dtype=np.float32)
        self._chk(self._L.sim3opt_match_batch_debug_nn(self._b, int(pair), _p(bi, _ip), _p(bd, _fp), _p(si, _ip),
                                                       _p(sd, _fp)), "match_batch_debug_nn")
        return dict(best_idx=bi, best_d2=bd, second_idx=si, second_d2=sd)

    def debug_depth(self, frame, uv):
        """Pixels uv (n, 2) through the kernel's K-nearest code on `frame`'s observations: (depth (n,), neighbours
        (n, knn_k) int32, -1 padded)."""
        q = _f32(uv).reshape(-1, 2)
        n = q.shape[0]
        z, nb = np.empty(n), np.empty((n, self._opt.knn_k), dtype=np.int32)
        self._chk(self._L.sim3opt_match_batch_debug_depth(self._b, n, int(frame), _p(q, _fp), _p(z, _dp), _p(nb, _ip)),
                  "match_batch_debug_depth")
        return z, nb


class PlaceBatch(_Handle):
    """sim3opt_place_batch*: bag-of-words place recognition over a whole sequence of keyframes (detector.detectLoop,
    kittiDetector.h:1663).  It takes the kp_ptr / desc MatchBatch.set_frames takes; pairs() is what
    MatchBatch.set_pairs takes.  PARITY UNPINNED: include/sim3opt.h says what is the reference's and what is recalled
    from upstream."""
    _prefix, _Options = "place_batch", PlaceBatchOptions
    TILES = ("wavefront", "workgroup", "bow_chunk", "score_lds", "score_frames", "lds_nodes")

    def set_vocabulary(self, parent, centre, weight, word_id):
        p, c = _i32(parent).reshape(-1), _f32(centre).reshape(-1, 64)
        w, i = _f64(weight).reshape(-1), _i32(word_id).reshape(-1)
        if not p.shape[0] == c.shape[0] == w.shape[0] == i.shape[0]:
            raise ValueError("parent, centre, weight and word_id hold one entry per node")
        self._chk(self._L.sim3opt_place_batch_set_vocabulary(self._b, p.shape[0], _p(p, _ip), _p(c, _fp), _p(w, _dp),
                                                             _p(i, _ip)), "place_batch_set_vocabulary")

    def set_frames(self, kp_ptr, desc):
        kpp, d = _i32(kp_ptr).reshape(-1), _f32(desc).reshape(-1, 64)
        n = kpp.shape[0] - 1
        if n >= 1 and d.shape[0] < kpp.max():
            raise ValueError("descriptor array shorter than kp_ptr says")
        if d.shape[0] == 0:
            d = np.zeros((1, 64), dtype=np.float32)  # (the C-ABI refuses a NULL array; nothing of it is read)
        self._chk(self._L.sim3opt_place_batch_set_frames(self._b, n, _p(kpp, _ip), _p(d, _fp)), "place_batch_set_frames")

    def set_frames_from(self, store):
        """set_frames with kp_ptr / desc read in place from a FrameStore's current snapshot"""
        self._chk(self._L.sim3opt_place_batch_set_frames_from(self._b, _store_handle(store)), "place_batch_set_frames_from")

    def dims(self):
        """dict: n_nodes, n_words, depth, n_frames, total_descriptors and the kernels' tile sizes (TILES)"""
        v = [C.c_int32() for _ in range(5)]
        t = (C.c_int32 * 6)()
        self._chk(self._L.sim3opt_place_batch_dims(self._b, *(C.byref(x) for x in v), t), "place_batch_dims")
        out = dict(zip(("n_nodes", "n_words", "depth", "n_frames", "total_descriptors"), (x.value for x in v)))
        out.update(zip(self.TILES, t))
        return out

    def solve(self):
        """The number of candidates; raises when the library reports an error."""
        return self._count(self._L.sim3opt_place_batch_solve(self._b), "place_batch_solve")

    def results(self):
        """dict of per-frame arrays: status, match, score, ns_factor, n_consistent, island (n, 2)"""
        n = self.dims()["n_frames"]
        st, ma, nc = (np.empty(n, dtype=np.int32) for _ in range(3))
        sc, ns, isl = np.empty(n), np.empty(n), np.empty((n, 2), dtype=np.int32)
        self._chk(self._L.sim3opt_place_batch_get_results(self._b, _p(st, _ip), _p(ma, _ip), _p(sc, _dp), _p(ns, _dp),
                                                          _p(nc, _ip), _p(isl, _ip)), "place_batch_get_results")
        return dict(status=st, match=ma, score=sc, ns_factor=ns, n_consistent=nc, island=isl)

    def pairs(self):
        """(n_pairs, 2) int32: (query, match) of the candidates in ascending query"""
        n = C.c_int32()
        self._chk(self._L.sim3opt_place_batch_get_pairs(self._b, 0, C.byref(n), None), "place_batch_get_pairs")
        out = np.empty((n.value, 2), dtype=np.int32)
        self._chk(self._L.sim3opt_place_batch_get_pairs(self._b, n.value, C.byref(n), _p(out, _ip)),
                  "place_batch_get_pairs")
        return out

    def bow(self):
        """(bow_ptr (n + 1,), word, value): the ragged bag-of-words vectors, by ascending word id within a frame"""
        ptr = np.empty(self.dims()["n_frames"] + 1, dtype=np.int32)
        self._chk(self._L.sim3opt_place_batch_get_bow(self._b, _p(ptr, _ip), None, None), "place_batch_get_bow")
        w, v = np.empty(int(ptr[-1]), dtype=np.int32), np.empty(int(ptr[-1]))
        self._chk(self._L.sim3opt_place_batch_get_bow(self._b, None, _p(w, _ip), _p(v, _dp)), "place_batch_get_bow")
        return ptr, w, v

    def debug_words(self, desc):
        """Descriptors (n, 64) through the descent code of k_place_words: (word (n,), path_d2 (n, depth), -1 padded)."""
        d = _f32(desc).reshape(-1, 64)
        n = d.shape[0]
        w, path = np.empty(n, dtype=np.int32), np.empty((n, self.dims()["depth"]))
        self._chk(self._L.sim3opt_place_batch_debug_words(self._b, n, _p(d, _fp), _p(w, _ip), _p(path, _dp)),
                  "place_batch_debug_words")
        return w, path

    def debug_scores(self, query):
        """s(v_query, v_j) for every frame j of the last solve"""
        row = np.empty(self.dims()["n_frames"])
        self._chk(self._L.sim3opt_place_batch_debug_scores(self._b, int(query), _p(row, _dp)), "place_batch_debug_scores")
        return row

    def debug_islands(self, query):
        """dict: kept_j, kept_score (ascending j); island (n_islands, 4: first, last, best_entry, results),
        island_score"""
        R = 1024  # max_db_results' upper limit: room whatever the last solve ran with
        nk, ni = C.c_int32(), C.c_int32()
        kj, ks = np.empty(R, dtype=np.int32), np.empty(R)
        isl, iss = np.empty((R, 4), dtype=np.int32), np.empty(R)
        self._chk(self._L.sim3opt_place_batch_debug_islands(self._b, int(query), C.byref(nk), _p(kj, _ip), _p(ks, _dp),
                                                            C.byref(ni), _p(isl, _ip), _p(iss, _dp)),
                  "place_batch_debug_islands")
        return dict(kept_j=kj[:nk.value].copy(), kept_score=ks[:nk.value].copy(), island=isl[:ni.value].copy(),
                    island_score=iss[:ni.value].copy())


class VocabularyTrainer(_Handle):
    """sim3opt_vocabulary*: the vocabulary tree PlaceBatch descends, trained on the descriptors of a sequence by
    hierarchical k-means (DBoW2's create over FSurf64).  It takes the kp_ptr / desc PlaceBatch.set_frames takes;
    vocabulary() is what PlaceBatch.set_vocabulary(*...) takes.  PARITY UNPINNED: include/sim3opt.h says what is the
    reference's and what is recalled from upstream."""
    _prefix, _Options = "vocabulary", VocabularyOptions
    TILES = ("chunk", "mean_chunk")

    def set_frames(self, kp_ptr, desc):
        kpp, d = _i32(kp_ptr).reshape(-1), _f32(desc).reshape(-1, 64)
        n = kpp.shape[0] - 1
        if n >= 1 and d.shape[0] < kpp.max():
            raise ValueError("descriptor array shorter than kp_ptr says")
        if d.shape[0] == 0:
            d = np.zeros((1, 64), dtype=np.float32)  # (the C-ABI refuses a NULL array; nothing of it is read)
        self._chk(self._L.sim3opt_vocabulary_set_frames(self._b, n, _p(kpp, _ip), _p(d, _fp)), "vocabulary_set_frames")

    def set_frames_from(self, store):
        """set_frames with kp_ptr / desc read in place from a FrameStore's current snapshot"""
        self._chk(self._L.sim3opt_vocabulary_set_frames_from(self._b, _store_handle(store)), "vocabulary_set_frames_from")

    def train(self):
        """The number of nodes; raises when the library reports an error."""
        return self._count(self._L.sim3opt_vocabulary_train(self._b), "vocabulary_train")

    def dims(self):
        """dict: n_nodes, n_words, depth, n_unconverged, n_frames, total_descriptors, passes (per level, 8) and the
        kernels' tile sizes (TILES)"""
        v = [C.c_int32() for _ in range(6)]
        ps, t = (C.c_int32 * 8)(), (C.c_int32 * 2)()
        self._chk(self._L.sim3opt_vocabulary_dims(self._b, *(C.byref(x) for x in v), ps, t), "vocabulary_dims")
        out = dict(zip(("n_nodes", "n_words", "depth", "n_unconverged", "n_frames", "total_descriptors"),
                       (x.value for x in v)))
        out["passes"] = list(ps)
        out.update(zip(self.TILES, t))
        return out

    def vocabulary(self):
        """(parent, centre (n, 64), weight, word_id): the arguments of PlaceBatch.set_vocabulary"""
        n = self.dims()["n_nodes"]
        p, w = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        c, g = np.empty((n, 64), dtype=np.float32), np.empty(n)
        self._chk(self._L.sim3opt_vocabulary_get_vocabulary(self._b, _p(p, _ip), _p(c, _fp), _p(g, _dp), _p(w, _ip)),
                  "vocabulary_get_vocabulary")
        return p, c, g, w

    def assignment(self, descent=False):
        """Per training descriptor the leaf node it ended in by clustering; with descent=True also the leaf node the
        descent rule reaches on the finished tree (what the weights were counted from)."""
        d = self.dims()["total_descriptors"]
        a, b = np.empty(d, dtype=np.int32), np.empty(d, dtype=np.int32)
        self._chk(self._L.sim3opt_vocabulary_get_assignment(self._b, _p(a, _ip), _p(b, _ip)), "vocabulary_get_assignment")
        return (a, b) if descent else a

    def debug_seeding(self, node):
        """dict: members (the chosen descriptors), W and r (one per round run)"""
        nc, nr = C.c_int32(), C.c_int32()
        m, W, r = np.empty(64, dtype=np.int32), np.empty(64), np.empty(64)
        self._chk(self._L.sim3opt_vocabulary_debug_seeding(self._b, int(node), C.byref(nc), _p(m, _ip), C.byref(nr),
                                                           _p(W, _dp), _p(r, _dp)), "vocabulary_debug_seeding")
        return dict(members=m[:nc.value].copy(), W=W[:nr.value].copy(), r=r[:nr.value].copy())

    def debug_lloyd(self, level, n_pass, k=None):
        """dict: first_node, cluster (per descriptor) and centre (n_level_nodes, k, 64) after n_pass passes of `level`;
        k: the branching the last training ran with (the options' by default)"""
        k = self._opt.k if k is None else k
        f, n = C.c_int32(), C.c_int32()
        self._chk(self._L.sim3opt_vocabulary_debug_lloyd(self._b, int(level), int(n_pass), C.byref(f), C.byref(n), None,
                                                         None), "vocabulary_debug_lloyd")
        cl = np.empty(self.dims()["total_descriptors"], dtype=np.int32)
        ce = np.empty((n.value, k, 64), dtype=np.float32)
        self._chk(self._L.sim3opt_vocabulary_debug_lloyd(self._b, int(level), int(n_pass), C.byref(f), C.byref(n),
                                                         _p(cl, _ip), _p(ce, _fp)), "vocabulary_debug_lloyd")
        return dict(first_node=f.value, cluster=cl, centre=ce)


SURF_OK, SURF_NO_KEYPOINTS = 0, 1


class SurfBatch(_Handle):
    """sim3opt_surf_batch*: SURF-64 keypoints and descriptors of a batch of grey images of one size
    (SurfExtractor::operator(), kitti_surf.cpp:501-523), the head of the chain: kp_ptr(), and kp / desc of keypoints(),
    are what MatchBatch.set_frames, PlaceBatch.set_frames and VocabularyTrainer.set_frames take.  PARITY UNPINNED:
    include/sim3opt.h holds the definition and says what is the call site's and what is recalled from upstream."""
    _prefix, _Options = "surf_batch", SurfBatchOptions
    TILES = ("detect_tile", "rank_tile", "keypoint_lanes")
    FIELDS = ("kp", "desc", "size", "angle", "response", "octave", "laplacian")

    def set_images(self, images):
        """images: uint8, n x h x w (or h x w for one)"""
        a = np.ascontiguousarray(images, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("images: n x h x w")
        n, h, w = a.shape
        if a.size == 0:
            a = np.zeros(1, dtype=np.uint8)  # (the C-ABI refuses a NULL array; it refuses the size first)
        self._chk(self._L.sim3opt_surf_batch_set_images(self._b, n, w, h, w, _p(a, _up)), "surf_batch_set_images")

    def dims(self):
        """dict: n_images, width, height, total_keypoints and the kernels' tile sizes (TILES)"""
        v = [C.c_int32() for _ in range(4)]
        t = (C.c_int32 * 3)()
        self._chk(self._L.sim3opt_surf_batch_dims(self._b, *(C.byref(x) for x in v), t), "surf_batch_dims")
        out = dict(zip(("n_images", "width", "height", "total_keypoints"), (x.value for x in v)))
        out.update(zip(self.TILES, t))
        return out

    def solve(self):
        """The number of images with keypoints; raises when the library reports an error."""
        return self._count(self._L.sim3opt_surf_batch_solve(self._b), "surf_batch_solve")

    def solve_into(self, store):
        """solve(), with kp and desc left on the device in `store` (a FrameStore): keypoints() then gives the small
        fields only (desc=False) and the descriptors are store.get()'s."""
        return self._count(self._L.sim3opt_surf_batch_solve_into(self._b, _store_handle(store)), "surf_batch_solve_into")

    def kp_ptr(self):
        p = np.empty(self.dims()["n_images"] + 1, dtype=np.int32)
        self._chk(self._L.sim3opt_surf_batch_get_kp_ptr(self._b, _p(p, _ip)), "surf_batch_get_kp_ptr")
        return p

    @staticmethod
    def _arrays(n):
        return dict(kp=np.empty((n, 2), dtype=np.float32), desc=np.empty((n, 64), dtype=np.float32),
                    size=np.empty(n, dtype=np.float32), angle=np.empty(n, dtype=np.float32),
                    response=np.empty(n, dtype=np.float32), octave=np.empty(n, dtype=np.int32),
                    laplacian=np.empty(n, dtype=np.int32))

    def keypoints(self, desc=True):
        """dict of FIELDS over all keypoints; image f owns [kp_ptr()[f], kp_ptr()[f + 1]).  desc=False: without the
        descriptors (after solve_into they are the store's, and asking for them here is refused)."""
        o = self._arrays(self.dims()["total_keypoints"])
        if not desc:
            del o["desc"]
        self._chk(self._L.sim3opt_surf_batch_get_keypoints(
            self._b, *(_p(o[f], _fp) if f in o else None for f in self.FIELDS[:5]), _p(o["octave"], _ip),
            _p(o["laplacian"], _ip)), "surf_batch_get_keypoints")
        return o

    def summary(self):
        """dict of per-image arrays: status, n_candidates, n_interpolated, n_dropped"""
        n = self.dims()["n_images"]
        names = ("status", "n_candidates", "n_interpolated", "n_dropped")
        o = {k: np.empty(n, dtype=np.int32) for k in names}
        self._chk(self._L.sim3opt_surf_batch_get_summary(self._b, *(_p(o[k], _ip) for k in names)), "surf_batch_get_summary")
        return o

    def debug_integral(self, image):
        d = self.dims()
        S = np.empty((d["height"] + 1, d["width"] + 1), dtype=np.int32)
        self._chk(self._L.sim3opt_surf_batch_debug_integral(self._b, int(image), _p(S, _ip)), "surf_batch_debug_integral")
        return S

    def debug_responses(self, image, octave, layer):
        """(det, trace) of a layer, rows x cols each"""
        r, c = C.c_int32(), C.c_int32()
        a = (self._b, int(image), int(octave), int(layer), C.byref(r), C.byref(c))
        self._chk(self._L.sim3opt_surf_batch_debug_responses(*a, None, None), "surf_batch_debug_responses")
        det, tr = (np.empty((r.value, c.value), dtype=np.float32) for _ in range(2))
        if det.size:
            self._chk(self._L.sim3opt_surf_batch_debug_responses(*a, _p(det, _fp), _p(tr, _fp)), "surf_batch_debug_responses")
        return det, tr

    @staticmethod
    def _cand_arrays(n):
        n = max(n, 1)
        return dict(layer=np.empty(n, dtype=np.int32), pos0=np.empty((n, 3), dtype=np.float32),
                    response=np.empty(n, dtype=np.float32), kept=np.empty(n, dtype=np.uint8),
                    pos1=np.empty((n, 3), dtype=np.float32))

    def debug_candidates(self, image):
        """dict: octave, layer, pos0 (x, y, size before the interpolation), response, kept, pos1; scan order"""
        n = C.c_int32()
        a = (self._b, int(image), C.byref(n))
        self._chk(self._L.sim3opt_surf_batch_debug_candidates(*a, None, None, None, None, None), "surf_batch_debug_candidates")
        o = self._cand_arrays(n.value)
        if n.value:
            self._chk(self._L.sim3opt_surf_batch_debug_candidates(*a, _p(o["layer"], _ip), _p(o["pos0"], _fp),
                                                                  _p(o["response"], _fp), _p(o["kept"], _up),
                                                                  _p(o["pos1"], _fp)), "surf_batch_debug_candidates")
        return self._cand_out(o, n.value)

    @staticmethod
    def _cand_out(o, n):
        o = {k: v[:n].copy() for k, v in o.items()}
        o["octave"], o["layer"] = o["layer"] // 8, o["layer"] % 8
        return o

    def debug_orientation(self, keypoint):
        """dict: valid, vx, vy, angle (113 each) and window (72)"""
        o = dict(valid=np.empty(113, dtype=np.int32), vx=np.empty(113, dtype=np.float32), vy=np.empty(113, dtype=np.float32),
                 angle=np.empty(113, dtype=np.float32), window=np.empty(72, dtype=np.float32))
        self._chk(self._L.sim3opt_surf_batch_debug_orientation(self._b, int(keypoint), _p(o["valid"], _ip), _p(o["vx"], _fp),
                                                               _p(o["vy"], _fp), _p(o["angle"], _fp), _p(o["window"], _fp)),
                  "surf_batch_debug_orientation")
        return o

    def debug_patch(self, keypoint):
        p = np.empty((21, 21), dtype=np.float32)
        self._chk(self._L.sim3opt_surf_batch_debug_patch(self._b, int(keypoint), _p(p, _fp)), "surf_batch_debug_patch")
        return p

    @classmethod
    def reference_image(cls, img, responses=None, **options):
        """A test aid: the header's definition restated serially on the host (no device) for one image.  dict of
        FIELDS, counts (candidates, interpolated, dropped), S, candidates (as debug_candidates) and, with
        responses=(octave, layer), det and trace of that layer."""
        L = load()
        o = SurfBatchOptions()
        L.sim3opt_surf_batch_options_default(C.byref(o))
        for k, v in options.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        a = np.ascontiguousarray(img, dtype=np.uint8)
        if a.ndim != 2 or a.size == 0:
            raise ValueError("img: h x w")
        h, w = a.shape
        S = np.empty((h + 1, w + 1), dtype=np.int32)
        ro, rl = responses if responses is not None else (0, 0)
        det, tr = (np.empty((h >> ro, w >> ro), dtype=np.float32) for _ in range(2))
        counts = np.zeros(3, dtype=np.int32)
        cap, ccap = 4096, 4096
        while True:
            k, c = cls._arrays(cap), cls._cand_arrays(ccap)
            n = L.sim3opt_surf_reference_image(
                C.byref(o), w, h, w, _p(a, _up), cap, *(_p(k[f], _fp) for f in cls.FIELDS[:5]), _p(k["octave"], _ip),
                _p(k["laplacian"], _ip), _p(counts, _ip), _p(S, _ip), ro, rl,
                _p(det, _fp) if responses is not None and det.size else None,
                _p(tr, _fp) if responses is not None and det.size else None, ccap, _p(c["layer"], _ip), _p(c["pos0"], _fp),
                _p(c["response"], _fp), _p(c["kept"], _up), _p(c["pos1"], _fp))
            if n < 0:
                raise Sim3OptError(n, "surf_reference_image")
            if n <= cap and counts[0] <= ccap:
                break
            cap, ccap = max(cap, n), max(ccap, int(counts[0]))
        out = {f: v[:n].copy() for f, v in k.items()}
        out.update(counts=counts, S=S, candidates=cls._cand_out(c, int(counts[0])))
        if responses is not None:
            out.update(det=det, trace=tr)
        return out


def vocabulary_save(path, parent, centre, weight, word_id):
    """Writes a tree (the four arrays of PlaceBatch.set_vocabulary) into this library's own binary format."""
    p, c = _i32(parent).reshape(-1), _f32(centre).reshape(-1, 64)
    w, i = _f64(weight).reshape(-1), _i32(word_id).reshape(-1)
    if not p.shape[0] == c.shape[0] == w.shape[0] == i.shape[0]:
        raise ValueError("parent, centre, weight and word_id hold one entry per node")
    rc = load().sim3opt_vocabulary_save(os.fsencode(path), p.shape[0], _p(p, _ip), _p(c, _fp), _p(w, _dp), _p(i, _ip))
    if rc != OK:
        raise Sim3OptError(rc, "vocabulary_save")


def vocabulary_load(path):
    """(parent, centre (n, 64), weight, word_id) of a file vocabulary_save wrote"""
    L = load()
    n = C.c_int32()
    p, c, w, i = _ip(), _fp(), _dp(), _ip()
    rc = L.sim3opt_vocabulary_load(os.fsencode(path), C.byref(n), C.byref(p), C.byref(c), C.byref(w), C.byref(i))
    if rc != OK:
        raise Sim3OptError(rc, "vocabulary_load")
    try:
        N = n.value
        return (np.ctypeslib.as_array(p, (N,)).copy(), np.ctypeslib.as_array(c, (N, 64)).copy(),
                np.ctypeslib.as_array(w, (N,)).copy(), np.ctypeslib.as_array(i, (N,)).copy())
    finally:
        for q in (p, c, w, i):
            L.sim3opt_vocabulary_free(C.cast(q, C.c_void_p))


def align_trajectory(query_xyz, train_xyz, with_scale=True):
    """(S 4x4, rmse, max_dev) of the Umeyama alignment query -> train (kitti_surf.cpp:1091-1161)."""
    q, t = _f64(query_xyz).reshape(-1, 3), _f64(train_xyz).reshape(-1, 3)
    S = np.empty(16)
    rm, mx = C.c_double(), C.c_double()
    rc = load().sim3opt_align_trajectory(q.shape[0], _p(q, _dp), _p(t, _dp), int(with_scale),
                                         _p(S, _dp), C.byref(rm), C.byref(mx))
    if rc != OK:
        raise Sim3OptError(rc, "align_trajectory")
    return S.reshape(4, 4), rm.value, mx.value


def partition_rows_equal(n_block_rows, world):
    out = np.empty(world + 1, dtype=np.int32)
    rc = load().sim3opt_partition_rows_equal(int(n_block_rows), int(world), _p(out, _ip))
    if rc != OK:
        raise Sim3OptError(rc, "partition_rows_equal")
    return out


def partition_rows(rowptr, world):
    rp = _i32(rowptr)
    out = np.empty(world + 1, dtype=np.int32)
    rc = load().sim3opt_partition_rows(rp.shape[0] - 1, _p(rp, _ip), int(world), _p(out, _ip))
    if rc != OK:
        raise Sim3OptError(rc, "partition_rows")
    return out
