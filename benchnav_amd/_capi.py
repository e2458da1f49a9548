"""ctypes binding of include/benchnav_mppi.h (the C-ABI drop-in boundary).

No CPU fallback: importing works anywhere (so host logic is testable), but
`load()` raises if libbenchnav_mppi.so is missing and cannot be built, and
`bn_mppi_create` fails without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

# ---- enums (include/benchnav_mppi.h) ---------------------------------------------
BN_OK = 0
BN_ERR_INVALID, BN_ERR_HIP, BN_ERR_NO_DEVICE, BN_ERR_STATE = -1, -2, -3, -4
BN_NOISE_PHILOX, BN_NOISE_HOST_KT2, BN_NOISE_DEVICE_KT2, BN_NOISE_DEVICE_T2K = 0, 1, 2, 3
BN_MEM_HOST, BN_MEM_DEVICE = 0, 1
(BN_BUF_STATES, BN_BUF_WEIGHTS, BN_BUF_COSTS, BN_BUF_CONTROLS, BN_BUF_USTAR, BN_BUF_XSTAR,
 BN_BUF_MEAN, BN_BUF_MAP, BN_BUF_GOAL, BN_BUF_USTAR_XSTAR) = range(10)
BN_FLAG_STORE_CONTROLS, BN_FLAG_SHARED_MAP, BN_FLAG_NO_LDS_WINDOW, BN_FLAG_PROFILE, BN_FLAG_PRIVATE_STREAM = 1, 2, 4, 8, 16
BN_FLAG_NO_PIPELINE = 32
BN_FLAG_SAMPLED_SLIP = 64
BN_FLAG_WAVE_KERNEL = 128
BN_FLAG_ROLE_KERNEL = 256
BN_FLAG_LEAN = 512
BN_FLAG_LAT_KERNEL = 1024
BN_FLAG_NO_OVERLAP = 2048
BN_FLAG_REFERENCE_ORDER = 4096
BN_FLAG_HOST_PACED = 8192
BN_FLAG_UNORDERED_OUTPUTS = 16384
BN_BUF_STATES_ALT, BN_BUF_CONTROLS_ALT = 10, 11
BN_RISK_EXPECTED, BN_RISK_VAR, BN_RISK_CVAR = 0, 1, 2
BN_RISK_MAX_SETTINGS = 16
BN_EVAL_MAX_CLASSES, BN_EVAL_MAX_BINS, BN_EVAL_MAX_GROUPS, BN_EVAL_SLAB_CELLS, BN_EVAL_SLIP_SUMS, BN_EVAL_RISK_COUNTS = 64, 64, 512, 4096, 8, 5
(BN_TASK_TILE, BN_TASK_STATS, BN_TASK_MAX_SIDE, BN_TASK_MAX_CELLS, BN_TASK_MAX_MAPS, BN_TASK_MAX_PAIRS,
 BN_TASK_MAX_ATTEMPTS) = 32, 8, 4096, 1 << 24, 4096, 65536, 4096
BN_TASK_ERR_TILE, BN_TASK_ERR_UNITE, BN_TASK_ERR_FLATTEN = 1, 2, 4
BN_OUTCOME_GOAL, BN_OUTCOME_TIME_LIMIT, BN_OUTCOME_STOPPED, BN_OUTCOME_INVALID = 0, 1, 2, 3   # bn_episode_outcome
BN_AD_OK, BN_AD_OUT_OF_BOUNDS, BN_AD_GOAL_COLLISION, BN_AD_FIELD_ERROR = 0, 1, 2, 3   # bn_astar_dwa_status
BN_RRT_FLAG_GLOBAL_NODES, BN_RRT_FLAG_ONE_WAVE, BN_RRT_FLAG_FOUR_WAVES = 1, 2, 4
(BN_RRT_BUF_NODES, BN_RRT_BUF_EDGES, BN_RRT_BUF_COSTS, BN_RRT_BUF_COUNTS, BN_RRT_BUF_SAMPLES, BN_RRT_BUF_SAMPLE_FLAGS,
 BN_RRT_BUF_PATHS, BN_RRT_BUF_RESULTS) = range(8)
(BN_CLRRT_BUF_NODES, BN_CLRRT_BUF_EDGES, BN_CLRRT_BUF_COSTS, BN_CLRRT_BUF_COUNTS, BN_CLRRT_BUF_SEQ_LENGTHS, BN_CLRRT_BUF_CONTROLLERS,
 BN_CLRRT_BUF_ACTION_SEQS, BN_CLRRT_BUF_STATE_SEQS, BN_CLRRT_BUF_SAMPLES, BN_CLRRT_BUF_SAMPLE_FLAGS, BN_CLRRT_BUF_NEAREST,
 BN_CLRRT_BUF_FEASIBLE, BN_CLRRT_BUF_PATH_ACTIONS, BN_CLRRT_BUF_PATH_STATES, BN_CLRRT_BUF_RESULTS, BN_CLRRT_BUF_STEER_ACTIONS,
 BN_CLRRT_BUF_STEER_STATES, BN_CLRRT_BUF_STEER_PATHS, BN_CLRRT_BUF_STEER_TARGETS, BN_CLRRT_BUF_STEER_RESULTS, BN_CLRRT_BUF_STEER_COSTS,
 BN_CLRRT_BUF_STEER_CONTROLLERS, BN_CLRRT_BUF_MT_STATE, BN_CLRRT_BUF_MT_POS) = range(24)
(BN_CL_RUNNING, BN_CL_GOAL, BN_CL_TIME_LIMIT, BN_CL_NO_PLAN, BN_CL_NO_SEQUENCE, BN_CL_PLAN_EXHAUSTED, BN_CL_PATH_OVERFLOW,
 BN_CL_OUT_OF_BOUNDS) = range(8)                                                       # bn_clrrt_loop_status
BN_CL_EVENT_STEP, BN_CL_EVENT_REPLAN, BN_CL_EVENT_FROZEN = 0, 1, 2                     # bn_clrrt_loop_event
ABI_VERSION = 7


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device_id", C.c_int32), ("horizon", C.c_int32),
        ("num_samples", C.c_int32), ("num_instances", C.c_int32), ("grid_size", C.c_int32),
        ("resolution", C.c_float), ("x_limits", C.c_float * 2), ("y_limits", C.c_float * 2),
        ("sigma", C.c_float * 2), ("inv_var", C.c_float * 2), ("lambda_", C.c_float),
        ("u_min", C.c_float * 2), ("u_max", C.c_float * 2), ("dt", C.c_float),
        ("stuck_threshold", C.c_float), ("seed", C.c_uint64), ("flags", C.c_uint32),
        ("stream", C.c_void_p),
    ]


class PlanInfo(C.Structure):
    """bn_mppi_plan_info: what bn_mppi_create would decide (bn_mppi_debug_plan)."""
    _fields_ = ([("struct_size", C.c_uint32), ("n_cus", C.c_int32)]
                + [(n, C.c_int32) for n in ("nblk", "Kp", "pow2", "reach", "WN", "lds_park", "ref_order", "wrap_near", "regen_steps",
                                            "park_steps", "xs", "map_stride", "slip_on")]
                + [("inv_lambda", C.c_float)]
                + [(n, C.c_int32) for n in ("n_maps", "slow_path", "want_wave", "pipelined", "wave_kernel", "lat_kernel", "role_overlap",
                                            "ticket_det", "ticket_overlap", "ticket_mode", "may_overlap", "n_streams", "has_X", "has_U",
                                            "has_granules", "has_alt", "has_ticket_buffers", "has_slip_std")]
                + [("snap_cap", C.c_uint64), ("resident_wgs", C.c_uint64), ("buffer_bytes", C.c_uint64 * 12)])


class LaunchRecord(C.Structure):
    """bn_mppi_launch_record: one launch of the solve path as it was decided (bn_mppi_debug_launch_log)."""
    _fields_ = ([(n, C.c_int32) for n in ("call", "entry", "family", "eps_mode", "stream", "have_prev", "mean_from_part", "self_tail", "overlap",
                                          "cur_slot", "prev_slot", "wave_kernel", "lat_kernel", "aux_prio", "tail_merged", "closed_loop", "env_on",
                                          "ep_index", "state_inline", "host_paced", "x_buf", "u_buf", "flag_part", "flag_tail", "gran", "gran_prev",
                                          "mean_snap", "state_snap", "err", "err_dev", "out_copy_self", "env_z", "part_gathered")]
                + [(n, C.c_uint64) for n in ("solve", "tail_solve", "wait_part", "wait_tail", "wait_part_self", "wait_tail_self")])


class RRTConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device_id", C.c_int32), ("num_instances", C.c_int32), ("max_iterations", C.c_int32),
        ("path_cap", C.c_int32), ("flags", C.c_uint32), ("x_limits", C.c_double * 2), ("y_limits", C.c_double * 2),
        ("delta_distance", C.c_double), ("goal_sample_rate", C.c_double), ("goal_threshold", C.c_double), ("seed", C.c_uint64),
    ]


class CLRRTConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device_id", C.c_int32), ("num_instances", C.c_int32), ("max_iterations", C.c_int32),
        ("max_seqs", C.c_int32), ("path_cap", C.c_int32), ("grid_size", C.c_int32), ("reserved", C.c_int32), ("resolution", C.c_double),
        ("x_limits", C.c_double * 2), ("y_limits", C.c_double * 2), ("delta_distance", C.c_double), ("goal_sample_rate", C.c_double),
        ("goal_threshold", C.c_double), ("delta_t", C.c_double), ("transit_dt", C.c_double), ("u_min", C.c_double * 2),
        ("u_max", C.c_double * 2), ("seed", C.c_uint64),
    ]


# every symbol include/benchnav_mppi.h declares: name -> (restype, argtypes)
_FP = C.POINTER(C.c_float)
_H = C.c_void_p
SYMBOLS = {
    "bn_mppi_config_init": (None, [C.POINTER(Config)]),
    "bn_mppi_create": (C.c_int, [C.POINTER(Config), C.POINTER(_H)]),
    "bn_mppi_destroy": (None, [_H]),
    "bn_mppi_set_map": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_int]),
    "bn_mppi_set_slip_std": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_int]),
    "bn_mppi_get_slip_noise": (C.c_int, [_H, C.c_int32, C.c_uint64, _FP, _FP, _FP]),
    "bn_mppi_set_slip_noise": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_mppi_set_goal": (C.c_int, [_H, C.c_int32, _FP]),
    "bn_mppi_set_mean": (C.c_int, [_H, C.c_int32, _FP]),
    "bn_mppi_get_mean": (C.c_int, [_H, C.c_int32, _FP]),
    "bn_mppi_solve": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_int, _FP, _FP]),
    "bn_mppi_solve_async": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "bn_mppi_forward_async": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bn_mppi_forward_state_async": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bn_mppi_solve_n_async": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int32, C.c_int64]),
    "bn_mppi_set_rollout_offset": (C.c_int, [_H, C.c_int64]),
    "bn_mppi_shard_rollout_async": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "bn_mppi_shard_partials": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bn_mppi_shard_finish_async": (C.c_int, [_H, C.c_void_p, C.c_int32]),
    "bn_dist_unique_id": (C.c_int, [C.c_void_p]),
    "bn_mppi_shard_comm_prepare": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "bn_mppi_shard_comm_init": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32]),
    "bn_mppi_shard_solve_async": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "bn_mppi_env_attach": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_uint64]),
    "bn_mppi_env_set_freeze": (C.c_int, [_H, C.c_int32]),
    "bn_mppi_env_step": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "bn_mppi_env_collision_check": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_uint64, C.c_void_p]),
    "bn_mppi_episode_async": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_void_p]),
    "bn_mppi_episode_log": (C.c_int, [_H, _FP, _FP, _FP, C.POINTER(C.c_int32)]),
    "bn_mppi_dwa_solve": (C.c_int, [_H, _FP, _FP, C.c_int32, _FP, _FP, _FP, _FP, _FP, _FP, C.POINTER(C.c_int32)]),
    "bn_mppi_dwa_forward_async": (C.c_int, [_H, C.c_void_p, C.c_void_p, _FP, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]),
    "bn_mppi_dwa_candidates": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "bn_mppi_dwa_buffers": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "bn_mppi_sync": (C.c_int, [_H]),
    "bn_mppi_recovery_count": (C.c_uint64, [_H]),
    "bn_mppi_overlap_mode": (C.c_int32, [_H]),
    "bn_mppi_debug_cadence": (C.c_int, [_H, C.c_int32, C.c_double]),
    "bn_mppi_first_action": (C.c_int, [_H, C.c_int32, _FP]),
    "bn_mppi_debug_expire_wait": (C.c_int, [_H]),
    "bn_mppi_flush": (C.c_int, [_H]),
    "bn_mppi_debug_host_paced": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "bn_mppi_debug_plan": (C.c_int, [C.POINTER(Config), C.c_int32, C.POINTER(PlanInfo)]),
    "bn_mppi_debug_launch_log": (C.c_int, [_H, C.POINTER(LaunchRecord), C.c_int32]),
    "bn_mppi_get_weights": (C.c_int, [_H, C.c_int32, _FP]),
    "bn_mppi_get_costs": (C.c_int, [_H, C.c_int32, _FP]),
    "bn_mppi_get_states": (C.c_int, [_H, C.c_int32, _FP]),
    "bn_mppi_get_controls": (C.c_int, [_H, C.c_int32, _FP]),
    "bn_mppi_get_philox_noise": (C.c_int, [_H, C.c_int32, C.c_uint64, _FP]),
    "bn_mppi_get_top_samples": (C.c_int, [_H, C.c_int32, C.c_int32, _FP, _FP]),
    "bn_mppi_reroll_async": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "bn_mppi_device_buffer": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "bn_mppi_solve_count": (C.c_uint64, [_H]),
    "bn_mppi_arithmetic": (C.c_int32, [_H]),
    "bn_mppi_launches_per_solve": (C.c_int32, [_H]),
    "bn_mppi_launches_per_forward": (C.c_int32, [_H]),
    "bn_mppi_host_paced": (C.c_int32, [_H]),
    "bn_mppi_order_outputs": (C.c_int, [_H]),
    "bn_mppi_states_buffer_index": (C.c_int32, [_H]),
    "bn_mppi_fast_quotient": (C.c_int32, [_H]),
    "bn_mppi_row_pitch": (C.c_int32, [_H]),
    "bn_mppi_kernel_ms": (C.c_int, [_H, _FP, _FP, C.POINTER(C.c_int32)]),
    "bn_mppi_algorithmic_bytes": (C.c_int64, [_H, C.c_int]),
    "bn_mppi_algorithmic_bytes_window": (C.c_int64, [_H, C.c_int]),
    "bn_risk_map_infer": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_int, C.c_float,
                                    C.c_int32, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_int]),
    "bn_risk_last_error": (C.c_char_p, []),
    "bn_risk_maps_infer": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int), _FP, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_episode_score": (C.c_int, [C.c_int32] + [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_float, C.c_double] + [C.c_void_p] * 8),
    "bn_score_last_error": (C.c_char_p, []),
    "bn_eval_confusion_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "bn_eval_slip_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "bn_eval_slip_async": (C.c_int, [C.c_int32] + [C.c_void_p] * 8 + [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double] + [C.c_void_p] * 5
                           + [C.c_size_t]),
    "bn_eval_risk_async": (C.c_int, [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "bn_eval_last_error": (C.c_char_p, []),
    "bn_task_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bn_task_mask_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_float, C.c_void_p]),
    "bn_task_label_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t]),
    "bn_task_sample_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64,
                                       C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "bn_task_last_error": (C.c_char_p, []),
    "bn_mppi_episode_buffers": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32)]),
    "bn_astar_dwa_episode_buffers": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bn_astar_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_H)]),
    "bn_astar_destroy": (None, [_H]),
    "bn_astar_set_map": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_double]),
    "bn_astar_set_goal": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32]),
    "bn_astar_solve_async": (C.c_int, [_H, C.c_void_p]),
    "bn_astar_sync": (C.c_int, [_H]),
    "bn_astar_kernel_ms": (C.c_int, [_H, _FP]),
    "bn_astar_path": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "bn_astar_buffers": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "bn_astar_jump_build_async": (C.c_int, [_H, C.c_void_p]),
    "bn_astar_jump_ms": (C.c_int, [_H, _FP]),
    "bn_astar_paths_async": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_astar_jump_buffers": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]),
    "bn_astar_last_error": (C.c_char_p, []),
    "bn_astar_dwa_episode_async": (C.c_int, [_H, _H, C.c_int32, C.c_void_p, C.c_int, C.c_void_p, _FP, C.c_float, C.c_int32,
                                             C.c_int32, C.c_float, C.c_void_p]),
    "bn_astar_dwa_episode_log": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_astar_dwa_reset": (C.c_int, [_H]),
    "bn_astar_dwa_set_root": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32]),
    "bn_astar_dwa_set_walk": (C.c_int, [_H, C.c_int32]),
    "bn_terrain_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(_H)]),
    "bn_terrain_destroy": (None, [_H]),
    "bn_terrain_set_geometry": (C.c_int, [_H, C.c_double, C.c_double, C.c_double, C.c_int32]),
    "bn_terrain_set_draws": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    "bn_terrain_set_draw_params": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32,
                                             C.c_double, C.c_double]),
    "bn_terrain_draw_async": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "bn_terrain_draw_layout": (C.c_int, [_H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bn_terrain_read_draws": (C.c_int, [_H] + [C.c_void_p] * 9),
    "bn_terrain_set_slip": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int32]),
    "bn_terrain_generate_async": (C.c_int, [_H, C.c_void_p]),
    "bn_terrain_sync": (C.c_int, [_H]),
    "bn_terrain_buffers": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "bn_terrain_copy_out": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_terrain_spectrum": (C.c_int, [_H, C.c_int32, C.c_void_p]),
    "bn_terrain_set_coloring": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_int32]),
    "bn_terrain_colorize": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_void_p]),
    "bn_terrain_color_buffers": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "bn_terrain_class_counts": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "bn_terrain_last_error": (C.c_char_p, []),
    "bn_rrt_config_init": (None, [C.POINTER(RRTConfig)]),
    "bn_rrt_create": (C.c_int, [C.POINTER(RRTConfig), C.POINTER(_H)]),
    "bn_rrt_destroy": (None, [_H]),
    "bn_rrt_plan_async": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_rrt_grow_from_samples_async": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "bn_rrt_sync": (C.c_int, [_H]),
    "bn_rrt_device_buffer": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "bn_rrt_node_storage": (C.c_int32, [_H]),
    "bn_rrt_last_error": (C.c_char_p, []),
    "bn_clrrt_config_init": (None, [C.POINTER(CLRRTConfig)]),
    "bn_clrrt_create": (C.c_int, [C.POINTER(CLRRTConfig), C.POINTER(_H)]),
    "bn_clrrt_destroy": (None, [_H]),
    "bn_clrrt_set_map": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_double]),
    "bn_clrrt_set_instance_maps": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_double]),
    "bn_clrrt_plan_async": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_clrrt_grow_from_samples_async": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "bn_clrrt_steer_async": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_clrrt_sync": (C.c_int, [_H]),
    "bn_clrrt_device_buffer": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "bn_clrrt_path_cap": (C.c_int32, [_H]),
    "bn_clrrt_last_error": (C.c_char_p, []),
    "bn_clrrt_loop_reset": (C.c_int, [_H, _H, C.c_void_p, C.c_void_p, C.c_double, C.c_double]),
    "bn_clrrt_loop_run": (C.c_int, [_H, _H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, _FP]),
    "bn_clrrt_loop_log": (C.c_int, [_H] + [C.c_void_p] * 10),
    "bn_clrrt_loop_episode_buffers": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bn_clrrt_loop_rover_buffers": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "bn_clrrt_loop_set_plans": (C.c_int, [_H, _H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "bn_gp_max_points": (C.c_int32, []),
    "bn_gp_create": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double,
                               C.POINTER(_H)]),
    "bn_gp_destroy": (None, [_H]),
    "bn_gp_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32]),
    "bn_gp_predict_async": (C.c_int, [C.c_int32, C.c_void_p, C.POINTER(_H), C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "bn_gp_last_error": (C.c_char_p, []),
    "bn_gp_fit_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "bn_gp_fit_create": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(_H)]),
    "bn_gp_fit_destroy": (None, [_H]),
    "bn_gp_fit_set_raw": (C.c_int, [_H, C.c_void_p]),
    "bn_gp_fit_set_hyperparameters": (C.c_int, [_H, C.c_double, C.c_double, C.c_double, C.c_double]),
    "bn_gp_fit_evaluate_async": (C.c_int, [_H, C.c_void_p]),
    "bn_gp_fit_run_async": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double]),
    "bn_gp_fit_read": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bn_gp_fit_hyperparameters": (C.c_int, [_H, C.c_void_p]),
    "bn_gp_fit_history": (C.c_int32, [_H, C.c_void_p, C.c_int32]),
    "bn_gp_fit_finish": (C.c_int, [_H, C.c_void_p, C.POINTER(_H)]),
    "bn_gp_fit_last_error": (C.c_char_p, []),
    "bn_unet_param_count": (C.c_int64, [C.c_int32]),
    "bn_unet_create": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(_H)]),
    "bn_unet_destroy": (None, [_H]),
    "bn_unet_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bn_unet_forward_async": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t]),
    "bn_unet_feature_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bn_unet_conv2d_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bn_unet_conv2d_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_size_t]),
    "bn_unet_maxpool_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "bn_unet_last_error": (C.c_char_p, []),
    "bn_segtrain_param_count": (C.c_int64, [C.c_int32]),
    "bn_segtrain_create": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(_H)]),
    "bn_segtrain_destroy": (None, [_H]),
    "bn_segtrain_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bn_segtrain_grad_async": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "bn_segtrain_step_async": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                         C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t]),
    "bn_segtrain_read": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_int64]),
    "bn_segtrain_steps": (C.c_int64, [_H]),
    "bn_segtrain_conv2d_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 8),
    "bn_segtrain_conv2d_backward_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                    C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "bn_segtrain_batchnorm_forward_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_segtrain_batchnorm_backward_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                       C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bn_segtrain_maxpool_backward_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "bn_segtrain_cross_entropy_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_size_t]),
    "bn_segtrain_adam_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double,
                                         C.c_double, C.c_double, C.c_double, C.c_double]),
    "bn_segtrain_last_error": (C.c_char_p, []),
    "bn_dataset_sample_slips_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_uint64,
                                                C.c_uint32, C.c_void_p]),
    "bn_dataset_gather_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "bn_dataset_gather_async": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t]),
    "bn_dataset_last_error": (C.c_char_p, []),
    "bn_device_math_eval": (C.c_int,[C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "bn_device_rng_eval": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "bn_last_error": (C.c_char_p, []),
    "bn_mppi_abi_version": (C.c_int, []),
}

_lib = None


class BenchnavError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"benchnav_mppi error {code}: {msg}")
        self.code = code


def lib_path() -> str:
    return _build.LIB_PATH


def _preload_hip_runtime():
    """Make sure ONE HIP/HSA runtime serves both this library and torch.

    torch wheels bundle their own libamdhip64.so (soname libamdhip64.so.7) and load it by
    file name; our library needs `libamdhip64.so.7`.  If ours pulled in /opt/rocm's copy
    first, a later `import torch` would load a second runtime, which then sees no GPU.
    Loading torch's copy first satisfies both by soname.  Without torch installed the
    system ROCm runtime is used.
    """
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def _open_checked(path):
    """dlopen + bind every symbol of SYMBOLS.  Returns (lib, None) or (lib, what does not match)."""
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            return lib, f"symbol {name} missing: the header and the library disagree"
        fn.restype = res
        fn.argtypes = args
    if lib.bn_mppi_abi_version() != ABI_VERSION:
        return lib, f"ABI version {lib.bn_mppi_abi_version()} != binding {ABI_VERSION}"
    return lib, None


def load(build_if_missing: bool = True):
    """dlopen the in-tree library (building it with hipcc first if it is absent)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    _preload_hip_runtime()
    # A missing library is built.  A library older than its sources is rebuilt only on request (BENCHNAV_REBUILD_IF_STALE=1):
    # file times do not survive every way a tree gets copied to a GPU box, and a spurious 60 s rebuild in every test
    # process would be worse than the stale-binary risk.  A library that does not MATCH this binding -- another ABI version,
    # or a symbol of include/benchnav_mppi.h missing -- is rebuilt once, whatever its file time says.
    stale = os.environ.get("BENCHNAV_REBUILD_IF_STALE") == "1" and _build.is_stale()
    if not os.path.exists(path) or stale:
        if not build_if_missing:
            raise RuntimeError(f"{path} is missing; run `python -m benchnav_amd.build`")
        _build.build_library()
    lib, why = _open_checked(path)
    if why and build_if_missing:
        import _ctypes
        _ctypes.dlclose(lib._handle)     # or the next dlopen of this path returns the old image
        del lib
        _build.build_library(force=True)
        lib, why = _open_checked(path)
    if why:
        raise RuntimeError(f"{path} does not match this binding ({why}); run `python -m benchnav_amd.build`")
    _lib = lib
    return lib


def check(code: int):
    if code != BN_OK:
        raise BenchnavError(code, load().bn_last_error().decode("utf-8", "replace"))
