"""ctypes binding of the C ABI in include/mplx.h (csrc/libmplx.so).

There is no fallback: if the shared library is missing or cannot be loaded the
import of the engine fails with an explicit error, and every compute call
needs a gfx950 device (mplx_create fails without one).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPLX_LIB") or os.path.join(HERE, "csrc", "libmplx.so")  # MPLX_LIB: a diagnostic build

OK = 0
ERR_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_STATE = -1, -2, -3, -4

# every symbol include/mplx.h declares, in declaration order
SYMBOLS = [
    "mplx_create", "mplx_destroy", "mplx_last_error", "mplx_abi_version",
    "mplx_set_map", "mplx_edit_map", "mplx_map_upload_bytes", "mplx_read_cells", "mplx_set_potential", "mplx_set_region", "mplx_set_params", "mplx_set_controls",
    "mplx_update_potential_map", "mplx_set_search_region_path",
    "mplx_expand_device", "mplx_expand", "mplx_expand_lists_device", "mplx_expand_lists", "mplx_lists_zero_fill", "mplx_expand_lists_device_z", "mplx_get_succ",
    "mplx_set_goal", "mplx_post_lists_device", "mplx_post_packed_device",
    "mplx_pack_lists_device", "mplx_comm_unique_id", "mplx_comm_init", "mplx_comm_destroy", "mplx_comm_broadcast_map",
    "mplx_comm_allgather_lists", "mplx_comm_schedule",
    "mplx_check_edges",
    "mplx_device_alloc", "mplx_device_free", "mplx_memcpy_h2d", "mplx_memcpy_d2h", "mplx_memset",
    "mplx_synchronize", "mplx_timer_begin", "mplx_timer_end",
    "mplx_planner_create", "mplx_planner_destroy", "mplx_planner_attach_ctx", "mplx_planner_set_provider",
    "mplx_planner_set_map", "mplx_planner_edit_map", "mplx_planner_set_controls", "mplx_planner_configure", "mplx_planner_plan",
    "mplx_planner_trajectory", "mplx_planner_trajectory_end", "mplx_planner_closed_set", "mplx_planner_open_set", "mplx_planner_last_error", "mplx_planner_timing", "mplx_planner_set_prior_trajectory", "mplx_planner_set_prior_trajectory_potential", "mplx_planner_use_device_heuristic", "mplx_planner_set_lpastar", "mplx_planner_reset", "mplx_planner_linked_nodes", "mplx_planner_update_blocked_nodes", "mplx_planner_update_cleared_nodes", "mplx_planner_sub_state_space", "mplx_planner_set_edge_provider",
    "mplx_selftest_math", "mplx_selftest_forward_state", "mplx_set_lists_route", "mplx_last_lists_route", "mplx_last_lists_zero_rows", "mplx_last_grid_kernel", "mplx_last_identity_form", "mplx_debug_store_model", "mplx_yaw_pin_stats", "mplx_service", "mplx_device_info",
]

# the symbols include/mplx_map_util.h declares (MapUtil's dilate / freeUnknown / freeAll / clouds on the device map),
# exported by the same library; kept apart from SYMBOLS, which is exactly mplx.h + mplx_debug.h
MAP_UTIL_SYMBOLS = ["mplx_map_dilate", "mplx_map_free", "mplx_map_cloud"]
CELL_OCCUPIED, CELL_FREE, CELL_UNKNOWN = 0, 1, 2
# ... and the ones include/mplx_rollout.h declares (batched rollouts), kept apart in the same way
ROLLOUT_SYMBOLS = ["mplx_rollout_device", "mplx_rollout"]
ROLLOUT_BAD_ACTION, ROLLOUT_HEADING_BAND = 4, 0x80
# ... and the ones include/mplx_ray.h declares (MapUtil::rayTrace, the ray trace of is_goal)
RAY_SYMBOLS = ["mplx_ray_trace_device", "mplx_ray_trace", "mplx_goal_sight_device"]
RAY_LEFT_MAP, RAY_HIT, RAY_BAD, RAY_TRUNCATED = 1, 2, 4, 8
FLAG_GOAL_BLOCKED = 8
# ... and the ones include/mplx_traj.h declares (Trajectory: info, samples, traverse_trajectory)
TRAJ_SYMBOLS = ["mplx_traj_info_device", "mplx_traj_info", "mplx_traj_sample_device", "mplx_traj_sample",
                "mplx_traj_traverse_device", "mplx_traj_traverse"]
TRAJ_EMPTY, TRAJ_BAD_ACTION, TRAJ_BAD = 1, 2, 4
TRAJ_COMMAND, TRAJ_WAYPOINT = 0, 1
# ... and the ones include/mplx_table.h declares (the persistent node table: relax, frontier, path)
TABLE_SYMBOLS = ["mplx_table_create", "mplx_table_destroy", "mplx_table_clear", "mplx_table_view_of", "mplx_table_stats",
                 "mplx_table_seed", "mplx_table_relax_device", "mplx_table_find_device", "mplx_table_find", "mplx_table_path",
                 "mplx_table_set_time_keys", "mplx_time_key"]
TABLE_NODES_FULL, TABLE_PROBE_FULL, TABLE_FRONTIER_FULL = 1, 2, 4
# ... and the ones include/mplx_open.h declares (the open set of a table: push, select)
OPEN_SYMBOLS = ["mplx_open_create", "mplx_open_destroy", "mplx_open_clear", "mplx_open_view_of", "mplx_open_push_device",
                "mplx_open_select_device"]
OPEN_IS_OPEN, OPEN_IS_GOAL, OPEN_SEEN = 1, 2, 4
OPEN_SELECTED, OPEN_FOUND, OPEN_EMPTY = 0, 1, 2
# ... and the ones include/mplx_multi.h declares (Q queries in one table and one open set)
MULTI_SYMBOLS = ["mplx_table_create_multi", "mplx_table_query_of", "mplx_table_seed_multi", "mplx_table_find_multi_device",
                 "mplx_table_find_multi", "mplx_open_set_goals", "mplx_open_select_multi_device"]
# ... and the ones include/mplx_best.h declares (the k best open nodes per query)
BEST_SYMBOLS = ["mplx_open_select_best_device", "mplx_open_select_best_multi_device"]
# ... and the one include/mplx_anytime.h declares (re-key an open set, the lower bound of its open nodes)
ANYTIME_SYMBOLS = ["mplx_open_rekey_device"]
# ... and the ones include/mplx_replan.h declares (re-root and repair a table after a map edit)
REPLAN_SYMBOLS = ["mplx_table_rebase_device", "mplx_table_rebase_multi_device", "mplx_open_push_closed_device"]
# ... and the ones include/mplx_prior.h declares (prior-trajectory guidance of an open set)
PRIOR_SYMBOLS = ["mplx_open_set_priors_device", "mplx_open_clear_priors", "mplx_open_prior_view_of", "mplx_planner_prior_table"]
# ... and the ones include/mplx_solve.h declares (the batched trajectory solver and Trajectory on what it returns)
SOLVE_SYMBOLS = ["mplx_poly_create", "mplx_poly_destroy", "mplx_solve_device", "mplx_solve", "mplx_poly_info_device",
                 "mplx_poly_info", "mplx_poly_sample_device", "mplx_poly_sample", "mplx_poly_traverse_device",
                 "mplx_poly_traverse"]
SOLVE_EMPTY, SOLVE_BAD_TIME, SOLVE_SINGULAR = 1, 2, 8
USE_POS, USE_VEL, USE_ACC = 1, 2, 4
# ... and the ones include/mplx_limits.h declares (caller-given segments in a poly, and the dynamic limits of a set)
LIMITS_SYMBOLS = ["mplx_poly_load_device", "mplx_poly_load", "mplx_poly_limits_device", "mplx_poly_limits",
                  "mplx_shortcut_device", "mplx_shortcut"]
SHORTCUT_BAD_CHAIN = 16
LIMITS_REFERENCE, LIMITS_ALL_ROOTS = 0, 1
EXCEED_VEL, EXCEED_ACC, EXCEED_JRK = 1, 2, 4
# ... and the ones include/mplx_scale.h declares (time scaling of the set a poly holds: Lambda, scale, scale_down)
SCALE_SYMBOLS = ["mplx_poly_set_lambda_device", "mplx_poly_set_lambda", "mplx_poly_scale_device", "mplx_poly_scale",
                 "mplx_poly_scale_down_device", "mplx_poly_scale_down", "mplx_poly_tau_device", "mplx_poly_tau",
                 "mplx_poly_clear_lambda"]
SCALE_REFERENCE, SCALE_ROBUST = 0, 1
LAMBDA_BAD_POINTS, LAMBDA_NOT_POSITIVE = 32, 64
LAMBDA_MAX_SEGS, LAMBDA_NEWTON = 8, 3
# ... and the ones include/mplx_conflict.h declares (conflicts between the trajectories of one set on a common clock)
CONFLICT_SYMBOLS = ["mplx_poly_conflicts_device", "mplx_poly_conflicts", "mplx_traj_conflicts_device", "mplx_traj_conflicts"]
CONFLICT_PARK, CONFLICT_GONE = 0, 1
CONFLICT_BAD_INPUT = 128
# ... and the ones include/mplx_reserve.h declares (a reservation table and the check of successor lists against it)
RESERVE_SYMBOLS = ["mplx_reserve_create", "mplx_reserve_destroy", "mplx_reserve_fill_poly_device", "mplx_reserve_fill_poly",
                   "mplx_reserve_fill_traj_device", "mplx_reserve_fill_traj", "mplx_reserve_shape", "mplx_reserve_positions",
                   "mplx_reserve_set_queries", "mplx_reserve_check_device", "mplx_reserve_park_device"]
RESERVE_MAX_BYTES = 1 << 30
# ... and the ones include/mplx_reserve_poly.h declares (a solved set against a reservation table, the timed shortcut)
RESERVE_POLY_SYMBOLS = ["mplx_reserve_check_poly_device", "mplx_reserve_check_poly", "mplx_shortcut_timed_device",
                        "mplx_shortcut_timed"]
# ... and the one include/mplx_wait.h declares (the zero control's entry appended to the lists of an expansion)
WAIT_SYMBOLS = ["mplx_lists_add_wait_device"]
# ... and the one include/mplx_replan_timed.h declares (the rebase of a table with time keys, waits and reservations)
REPLAN_TIMED_SYMBOLS = ["mplx_table_rebase_timed_device"]
# ... and the ones include/mplx_field.h declares (goal distance fields and the push of an open set that reads one)
FIELD_SYMBOLS = ["mplx_field_create", "mplx_field_destroy", "mplx_field_build", "mplx_field_shape", "mplx_field_view_of",
                 "mplx_field_download", "mplx_field_is_stale", "mplx_field_passes", "mplx_open_set_field", "mplx_open_clear_field"]
FIELD_MAX_BYTES = 1 << 30
# ... and the ones include/mplx_heur.h declares (the dynamics-aware heuristic: batches of states, the push of an open set)
HEUR_SYMBOLS = ["mplx_heur_eval", "mplx_heur_eval_device", "mplx_open_set_heur", "mplx_planner_set_heur_dynamics"]
HEUR_DEFAULT, HEUR_REFERENCE, HEUR_ROBUST = 0, 1, 2
# ... and the ones include/mplx_body.h declares (an ellipsoid body against a point cloud: lists and trajectory sets)
BODY_SYMBOLS = ["mplx_body_create", "mplx_body_destroy", "mplx_body_set_shape", "mplx_body_fill", "mplx_body_fill_device",
                "mplx_body_fill_map", "mplx_body_shape", "mplx_body_cells", "mplx_body_check_device",
                "mplx_body_check_poly_device", "mplx_body_check_poly"]
BODY_MAX_BYTES = 1 << 30
BODY_BAD_ATTITUDE = 0x7fffffff
HEUR_BISECT = 56


def heur_mode(mode):
    """None / "default" / "reference" / "robust" (or the constant itself) -> MPLX_HEUR_*; anything else is passed on as
    an int for the library to refuse."""
    names = {None: HEUR_DEFAULT, False: HEUR_DEFAULT, "default": HEUR_DEFAULT, "reference": HEUR_REFERENCE, "robust": HEUR_ROBUST}
    if isinstance(mode, str) or mode is None:
        if mode not in names:
            raise ValueError("heuristic mode %r: None, 'default', 'reference' or 'robust'" % (mode,))
        return names[mode]
    return int(mode)

ROUTE_AUTO, ROUTE_DENSE, ROUTE_TILE, ROUTE_GRID = 0, 1, 2, 3


class Params(C.Structure):
    _fields_ = [
        ("control", C.c_int32), ("reserved", C.c_int32),
        ("dt", C.c_double), ("w", C.c_double), ("wyaw", C.c_double),
        ("v_max", C.c_double), ("a_max", C.c_double), ("j_max", C.c_double), ("yaw_max", C.c_double),
        ("potential_weight", C.c_double), ("gradient_weight", C.c_double),
    ]


class Succ(C.Structure):
    _fields_ = [
        ("status", C.c_void_p), ("cost", C.c_void_p), ("hash", C.c_void_p),
        ("state", C.c_void_p), ("state_stride", C.c_int64), ("iters", C.c_void_p),
    ]


class SuccLists(C.Structure):
    _fields_ = [
        ("count", C.c_void_p), ("action", C.c_void_p), ("cost", C.c_void_p), ("hash", C.c_void_p),
        ("state", C.c_void_p), ("state_stride", C.c_int64), ("iters", C.c_void_p), ("node_stride", C.c_int64),
        ("heur", C.c_void_p), ("flags", C.c_void_p),  # ABI v8: written by the expansion launch (mplx_set_goal)
    ]


class RolloutOut(C.Structure):
    _fields_ = [
        ("status", C.c_void_p), ("steps", C.c_void_p), ("cost", C.c_void_p), ("prefix_cost", C.c_void_p),
        ("end_state", C.c_void_p), ("end_stride", C.c_int64),
        ("end_hash", C.c_void_p), ("end_heur", C.c_void_p), ("end_flags", C.c_void_p),
    ]


class RayOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("n_cells", C.c_void_p), ("first_hit", C.c_void_p), ("cells", C.c_void_p),
                ("cell_cap", C.c_int32)]


class TrajSet(C.Structure):
    _fields_ = [("starts", C.c_void_p), ("n_starts", C.c_int64), ("start_stride", C.c_int64), ("actions", C.c_void_p),
                ("n_traj", C.c_int64), ("horizon", C.c_int32), ("action_stride", C.c_int64)]


class TrajInfoOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("n_segs", C.c_void_p), ("total_time", C.c_void_p), ("effort", C.c_void_p),
                ("effort_stride", C.c_int64), ("seg_state", C.c_void_p), ("seg_stride", C.c_int64)]


class TrajTimes(C.Structure):
    _fields_ = [("form", C.c_int32), ("n_uniform", C.c_int32), ("times", C.c_void_p), ("n_times", C.c_int64),
                ("time_stride", C.c_int64)]


class TrajSampleOut(C.Structure):
    _fields_ = [("out", C.c_void_p), ("row_stride", C.c_int64), ("sample_stride", C.c_int64), ("status", C.c_void_p)]


class TrajTraverseOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("cost", C.c_void_p), ("n_samples", C.c_void_p), ("n_cells", C.c_void_p),
                ("stop_sample", C.c_void_p)]


class SolveIn(C.Structure):
    _fields_ = [("waypoints", C.c_void_p), ("n_prob", C.c_int64), ("w_max", C.c_int32), ("wp_stride", C.c_int64),
                ("n_wp", C.c_void_p), ("dts", C.c_void_p), ("dt_stride", C.c_int64), ("v", C.c_double),
                ("v_arr", C.c_void_p), ("control", C.c_int32), ("yaw_control", C.c_int32), ("wp_flags", C.c_void_p),
                ("flag_stride", C.c_int64)]


class SolveOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("n_segs", C.c_void_p), ("total_time", C.c_void_p), ("coeff", C.c_void_p),
                ("coeff_stride", C.c_int64), ("dts_out", C.c_void_p), ("dts_out_stride", C.c_int64),
                ("yaw_coeff", C.c_void_p), ("yaw_stride", C.c_int64), ("taus", C.c_void_p), ("taus_stride", C.c_int64)]


class PolyLoadIn(C.Structure):
    _fields_ = [("n_prob", C.c_int64), ("w_max", C.c_int32), ("control", C.c_int32), ("n_segs", C.c_void_p),
                ("dts", C.c_void_p), ("dt_stride", C.c_int64), ("coeff", C.c_void_p), ("coeff_stride", C.c_int64),
                ("src", C.c_void_p), ("src_index", C.c_void_p), ("index_stride", C.c_int64)]


class PolyLoadOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("n_segs", C.c_void_p), ("total_time", C.c_void_p), ("taus", C.c_void_p),
                ("taus_stride", C.c_int64)]


class ShortcutIn(C.Structure):
    _fields_ = [("states", C.c_void_p), ("n_query", C.c_int64), ("w_max", C.c_int32), ("control", C.c_int32),
                ("stride", C.c_int64), ("n_wp", C.c_void_p), ("max_hop", C.c_int32)]


class ShortcutOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("n_keep", C.c_void_p), ("keep", C.c_void_p), ("keep_stride", C.c_int64),
                ("cost", C.c_void_p), ("chain_cost", C.c_void_p), ("edge_cost", C.c_void_p), ("pair_out", C.POINTER(SolveOut))]


class LimitsIn(C.Structure):
    _fields_ = [("mv", C.c_double), ("ma", C.c_double), ("mj", C.c_double), ("mode", C.c_int32)]


class LimitsOut(C.Structure):
    _fields_ = [("max_vel", C.c_void_p), ("max_acc", C.c_void_p), ("max_jrk", C.c_void_p), ("max_stride", C.c_int64),
                ("exceed", C.c_void_p), ("valid", C.c_void_p), ("first_bad", C.c_void_p)]


class LambdaOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("n_lseg", C.c_void_p), ("total", C.c_void_p), ("Ts", C.c_void_p),
                ("ts_stride", C.c_int64), ("segs", C.c_void_p), ("seg_stride", C.c_int64)]


class LambdaIn(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("stride", C.c_int64), ("n_pts", C.c_void_p), ("mode", C.c_int32)]


class ScaleIn(C.Structure):
    _fields_ = [("ri", C.c_double), ("rf", C.c_double), ("ri_arr", C.c_void_p), ("rf_arr", C.c_void_p), ("mode", C.c_int32)]


class ScaleDownIn(C.Structure):
    _fields_ = [("mv", C.c_double), ("ma", C.c_double), ("ri", C.c_double), ("rf", C.c_double), ("mode", C.c_int32)]


class ScaleDownOut(C.Structure):
    _fields_ = [("scaled", C.c_void_p), ("max_l", C.c_void_p), ("t_lo", C.c_void_p), ("t_hi", C.c_void_p), ("lam", LambdaOut)]


class TauOut(C.Structure):
    _fields_ = [("tau", C.c_void_p), ("lam", C.c_void_p), ("lam_dot", C.c_void_p), ("found", C.c_void_p), ("stride", C.c_int64)]


class ConflictIn(C.Structure):
    _fields_ = [("step", C.c_double), ("n_steps", C.c_int32), ("mode", C.c_int32), ("t0", C.c_void_p), ("radius", C.c_void_p),
                ("radius_all", C.c_double), ("group", C.c_void_p), ("rank", C.c_void_p), ("chunk_steps", C.c_int32)]


class ReservePolyIn(C.Structure):
    _fields_ = [("t_start", C.c_void_p), ("radius", C.c_void_p), ("radius_all", C.c_double), ("ignore_group", C.c_void_p)]


class ReservePolyOut(C.Structure):
    _fields_ = [("hit", C.c_void_p), ("status", C.c_void_p), ("n_hit", C.c_void_p)]


class BodyPolyIn(C.Structure):
    _fields_ = [("step", C.c_double)]


class BodyPolyOut(C.Structure):
    _fields_ = [("hit", C.c_void_p), ("status", C.c_void_p), ("n_hit", C.c_void_p)]


class ConflictOut(C.Structure):
    _fields_ = [("first_step", C.c_void_p), ("first_partner", C.c_void_p), ("min_d2", C.c_void_p), ("status", C.c_void_p),
                ("pair_first", C.c_void_p), ("pair_stride", C.c_int64)]


class TableView(C.Structure):
    _fields_ = [("hash", C.c_void_p), ("g", C.c_void_p), ("pred", C.c_void_p), ("pred_action", C.c_void_p),
                ("state", C.c_void_p), ("state_stride", C.c_int64)]


class TableFrontier(C.Structure):
    _fields_ = [("id", C.c_void_p), ("g", C.c_void_p), ("state", C.c_void_p), ("state_stride", C.c_int64),
                ("capacity", C.c_int64), ("count", C.c_void_p)]


class OpenBound(C.Structure):
    """mplx_open_bound (include/mplx_anytime.h)"""
    _fields_ = [("lower", C.c_double), ("n_open", C.c_int64), ("n_pruned", C.c_int64), ("n_rekeyed", C.c_int64)]


class OpenView(C.Structure):
    _fields_ = [("f", C.c_void_p), ("flags", C.c_void_p)]


class OpenResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("goal_id", C.c_int32), ("count", C.c_int64), ("n_open", C.c_int64),
                ("f_min", C.c_double), ("goal_f", C.c_double), ("goal_g", C.c_double)]


class PriorSource(C.Structure):
    _fields_ = [("control", C.c_int32), ("nU", C.c_int32), ("udim", C.c_int32), ("U", C.c_void_p), ("dt", C.c_double)]


class PriorInfo(C.Structure):
    _fields_ = [("status", C.c_void_p), ("n_steps", C.c_void_p)]


class PriorView(C.Structure):
    _fields_ = [("n_steps", C.c_void_p), ("pos", C.c_void_p), ("togo", C.c_void_p), ("goal_row", C.c_void_p),
                ("goal_hash", C.c_void_p), ("step_capacity", C.c_int64)]


class FieldView(C.Structure):
    _fields_ = [("dist", C.c_void_p), ("F", C.c_int32), ("n_cells", C.c_int64)]


class RebaseResult(C.Structure):
    _fields_ = [("n_kept", C.c_int64), ("n_bad_edges", C.c_int64), ("n_roots", C.c_int64)]


class PackedLists(C.Structure):
    _fields_ = [
        ("count", C.c_void_p), ("offs", C.c_void_p), ("action", C.c_void_p), ("cost", C.c_void_p), ("hash", C.c_void_p),
        ("state", C.c_void_p), ("state_stride", C.c_int64), ("capacity", C.c_int64),
    ]


COMM_ID_BYTES = 128
COMM_META = 8
ROWBIT_ACTION, ROWBIT_COST, ROWBIT_HASH, ROWBIT_STATE = 1, 2, 4, 8
COMM_COPY, COMM_SEND, COMM_RECV = 0, 1, 2
ROW_COUNT, ROW_ACTION, ROW_COST, ROW_HASH, ROW_STATE0 = 0, 1, 2, 3, 4


class CommOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("peer", C.c_int32), ("row", C.c_int32), ("elem", C.c_int32),
                ("src_off", C.c_int64), ("dst_off", C.c_int64), ("bytes", C.c_int64)]


class GoalSpec(C.Structure):
    _fields_ = [("goal", C.c_void_p), ("control", C.c_int32), ("goal_control", C.c_int32), ("w", C.c_double),
                ("v_max", C.c_double), ("tol_pos", C.c_double), ("tol_vel", C.c_double), ("tol_acc", C.c_double),
                ("tol_yaw", C.c_double)]


class EdgesOut(C.Structure):
    _fields_ = [("free_flag", C.c_void_p), ("cost", C.c_void_p), ("cells", C.c_void_p), ("cell_count", C.c_void_p),
                ("cell_cap", C.c_int32), ("outside", C.c_void_p)]


class Post(C.Structure):
    _fields_ = [("heur", C.c_void_p), ("flags", C.c_void_p), ("canon", C.c_void_p)]


class PlannerConfig(C.Structure):
    _fields_ = [
        ("control", C.c_int32), ("max_expand", C.c_int32), ("batch", C.c_int32), ("goal_control", C.c_int32),
        ("dt", C.c_double), ("w", C.c_double), ("v_max", C.c_double), ("epsilon", C.c_double),
        ("tol_pos", C.c_double), ("tol_vel", C.c_double), ("tol_acc", C.c_double), ("tol_yaw", C.c_double),
    ]


class PlanSummary(C.Structure):
    _fields_ = [
        ("ok", C.c_int32), ("expansions", C.c_int32), ("closed", C.c_int32), ("opened", C.c_int32),
        ("nodes", C.c_int32), ("device_launches", C.c_int32), ("pairs", C.c_int64),
        ("cost", C.c_double), ("total_time", C.c_double), ("J", C.c_double * 4),
        ("segments", C.c_int32), ("state_mismatches", C.c_int32),
    ]


class PlanTiming(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("total_ms", "provider_ms", "fill_ms", "pick_ms", "relax_ms", "recover_ms")] + \
               [(k, C.c_int64) for k in ("relaxed", "improved", "pushes", "materialised", "heur_from_device")]


class MplxError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("mplx error %d: %s" % (code, text))
        self.code = code


_lib = None


def lib():
    """Load libmplx.so (once).  Fails loudly when the HIP extension is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "motion_primitive_library_amd: %s is missing. Build it with "
            "`python -m motion_primitive_library_amd.build` (needs hipcc); there is no CPU fallback."
            % LIB_PATH)
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64.so not found
        raise ImportError("motion_primitive_library_amd: cannot load %s: %s" % (LIB_PATH, e))
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    sig = {
        "mplx_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(vp)]),
        "mplx_destroy": (None, [vp]),
        "mplx_last_error": (C.c_char_p, [vp]),
        "mplx_abi_version": (C.c_int, []),
        "mplx_set_map": (C.c_int, [vp, vp, vp, vp, dbl]),
        "mplx_set_potential": (C.c_int, [vp, vp]),
        "mplx_set_region": (C.c_int, [vp, vp]),
        "mplx_set_params": (C.c_int, [vp, C.POINTER(Params)]),
        "mplx_set_controls": (C.c_int, [vp, vp, i32, i32]),
        "mplx_edit_map": (C.c_int, [vp, vp, vp, i64]),
        "mplx_map_upload_bytes": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "mplx_read_cells": (C.c_int, [vp, C.c_int, vp, i64, vp]),
        "mplx_set_goal": (C.c_int, [vp, C.POINTER(GoalSpec)]),
        "mplx_update_potential_map": (C.c_int, [vp, vp, vp, vp, dbl, vp]),
        "mplx_set_search_region_path": (C.c_int, [vp, vp, i32, i32, vp, vp]),
        "mplx_expand_device": (C.c_int, [vp, vp, i64, i64, C.POINTER(Succ)]),
        "mplx_expand": (C.c_int, [vp, vp, i64, i64, C.POINTER(Succ)]),
        "mplx_expand_lists_device": (C.c_int, [vp, vp, i64, i64, C.POINTER(SuccLists)]),
        "mplx_expand_lists": (C.c_int, [vp, vp, i64, i64, C.POINTER(SuccLists)]),
        "mplx_lists_zero_fill": (C.c_int, [vp, C.POINTER(SuccLists), C.POINTER(C.c_uint32)]),
        "mplx_expand_lists_device_z": (C.c_int, [vp, vp, i64, i64, C.POINTER(SuccLists), C.POINTER(C.c_uint32)]),
        "mplx_get_succ": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(i32)]),
        "mplx_post_lists_device": (C.c_int, [vp, C.POINTER(SuccLists), i64, C.POINTER(GoalSpec), C.POINTER(Post)]),
        "mplx_check_edges": (C.c_int, [vp, vp, vp, i64, i64, C.POINTER(EdgesOut)]),
        "mplx_pack_lists_device": (C.c_int, [vp, C.POINTER(SuccLists), i64, C.POINTER(PackedLists), C.POINTER(i64)]),
        "mplx_post_packed_device": (C.c_int, [vp, C.POINTER(PackedLists), i64, C.POINTER(GoalSpec), C.POINTER(Post)]),
        "mplx_comm_unique_id": (C.c_int, [vp]),
        "mplx_comm_init": (C.c_int, [vp, vp, i32, i32]),
        "mplx_comm_destroy": (C.c_int, [vp]),
        "mplx_comm_broadcast_map": (C.c_int, [vp, i32]),
        "mplx_comm_allgather_lists": (C.c_int, [vp, C.POINTER(PackedLists), i64, C.POINTER(PackedLists), vp, vp]),
        "mplx_comm_schedule": (i64, [i32, i32, vp, i32, C.POINTER(CommOp), i64, vp, vp]),
        "mplx_device_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
        "mplx_device_free": (C.c_int, [vp, vp]),
        "mplx_memcpy_h2d": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "mplx_memcpy_d2h": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "mplx_memset": (C.c_int, [vp, vp, C.c_int, C.c_size_t]),
        "mplx_synchronize": (C.c_int, [vp]),
        "mplx_timer_begin": (C.c_int, [vp]),
        "mplx_timer_end": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "mplx_planner_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "mplx_planner_destroy": (None, [vp]),
        "mplx_planner_attach_ctx": (C.c_int, [vp, vp]),
        "mplx_planner_set_provider": (C.c_int, [vp, vp, vp, vp]),
        "mplx_planner_set_map": (C.c_int, [vp, vp, vp, vp, dbl]),
        "mplx_planner_edit_map": (C.c_int, [vp, vp, vp, i64]),
        "mplx_planner_set_controls": (C.c_int, [vp, vp, i32, i32]),
        "mplx_planner_configure": (C.c_int, [vp, C.POINTER(PlannerConfig)]),
        "mplx_planner_plan": (C.c_int, [vp, vp, vp, C.POINTER(PlanSummary)]),
        "mplx_planner_trajectory": (C.c_int, [vp, vp, vp, i32]),
        "mplx_planner_trajectory_end": (C.c_int, [vp, vp]),
        "mplx_planner_closed_set": (C.c_int, [vp, vp, i32, C.POINTER(i32)]),
        "mplx_planner_open_set": (C.c_int, [vp, vp, i32, C.POINTER(i32)]),
        "mplx_planner_last_error": (C.c_char_p, [vp]),
        "mplx_planner_timing": (C.c_int, [vp, C.POINTER(PlanTiming)]),
        "mplx_planner_use_device_heuristic": (C.c_int, [vp, C.c_int]),
        "mplx_planner_set_prior_trajectory": (C.c_int, [vp, vp]),
        "mplx_planner_set_prior_trajectory_potential": (C.c_int, [vp, vp, vp, dbl, dbl]),
        "mplx_planner_set_lpastar": (C.c_int, [vp, C.c_int]),
        "mplx_planner_reset": (C.c_int, [vp]),
        "mplx_planner_linked_nodes": (C.c_int, [vp, vp, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
        "mplx_planner_update_blocked_nodes": (C.c_int, [vp, vp, i64]),
        "mplx_planner_update_cleared_nodes": (C.c_int, [vp, vp, i64]),
        "mplx_planner_sub_state_space": (C.c_int, [vp, i32]),
        "mplx_planner_set_edge_provider": (C.c_int, [vp, vp, vp]),
        "mplx_selftest_math": (C.c_int, [vp, C.c_int, vp, vp, vp, i64]),
        "mplx_selftest_forward_state": (C.c_int, [i32, i32, vp, vp, C.c_double, vp]),
        "mplx_set_lists_route": (C.c_int, [vp, C.c_int]),
        "mplx_last_lists_route": (C.c_int, [vp]),
        "mplx_last_lists_zero_rows": (C.c_int, [vp]),
        "mplx_last_grid_kernel": (C.c_int, [vp]),
        "mplx_last_identity_form": (C.c_int, [vp]),
        "mplx_debug_store_model": (C.c_int, [vp, C.POINTER(SuccLists), i64]),
        "mplx_yaw_pin_stats": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64)]),
        "mplx_service": (C.c_int, [vp, C.c_int, C.POINTER(i64)]),
        "mplx_device_info": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.POINTER(i32)]),
        "mplx_map_dilate": (C.c_int, [vp, vp, i32, vp]),
        "mplx_map_free": (C.c_int, [vp, C.c_int, vp]),
        "mplx_map_cloud": (C.c_int, [vp, C.c_int, vp, i64, C.POINTER(i64)]),
        "mplx_rollout_device": (C.c_int, [vp, vp, i64, i64, vp, i64, i32, i64, C.POINTER(RolloutOut)]),
        "mplx_rollout": (C.c_int, [vp, vp, i64, i64, vp, i64, i32, i64, C.POINTER(RolloutOut)]),
        "mplx_ray_trace_device": (C.c_int, [vp, vp, vp, i64, i64, i64, i32, C.POINTER(RayOut)]),
        "mplx_ray_trace": (C.c_int, [vp, vp, vp, i64, i64, i64, i32, C.POINTER(RayOut)]),
        "mplx_goal_sight_device": (C.c_int, [vp, C.POINTER(SuccLists), i64, C.POINTER(GoalSpec), vp]),
        "mplx_traj_info_device": (C.c_int, [vp, C.POINTER(TrajSet), C.POINTER(TrajInfoOut)]),
        "mplx_traj_info": (C.c_int, [vp, C.POINTER(TrajSet), C.POINTER(TrajInfoOut)]),
        "mplx_traj_sample_device": (C.c_int, [vp, C.POINTER(TrajSet), C.POINTER(TrajTimes), C.POINTER(TrajSampleOut)]),
        "mplx_traj_sample": (C.c_int, [vp, C.POINTER(TrajSet), C.POINTER(TrajTimes), C.POINTER(TrajSampleOut)]),
        "mplx_traj_traverse_device": (C.c_int, [vp, C.POINTER(TrajSet), i32, C.POINTER(TrajTraverseOut)]),
        "mplx_traj_traverse": (C.c_int, [vp, C.POINTER(TrajSet), i32, C.POINTER(TrajTraverseOut)]),
        "mplx_poly_create": (C.c_int, [vp, i64, i32, C.POINTER(vp)]),
        "mplx_poly_destroy": (None, [vp]),
        "mplx_solve_device": (C.c_int, [vp, C.POINTER(SolveIn), C.POINTER(SolveOut)]),
        "mplx_solve": (C.c_int, [vp, C.POINTER(SolveIn), C.POINTER(SolveOut)]),
        "mplx_poly_info_device": (C.c_int, [vp, C.POINTER(TrajInfoOut)]),
        "mplx_poly_info": (C.c_int, [vp, C.POINTER(TrajInfoOut)]),
        "mplx_poly_sample_device": (C.c_int, [vp, C.POINTER(TrajTimes), C.POINTER(TrajSampleOut)]),
        "mplx_poly_sample": (C.c_int, [vp, C.POINTER(TrajTimes), C.POINTER(TrajSampleOut)]),
        "mplx_poly_traverse_device": (C.c_int, [vp, i32, C.POINTER(TrajTraverseOut)]),
        "mplx_poly_traverse": (C.c_int, [vp, i32, C.POINTER(TrajTraverseOut)]),
        "mplx_poly_load_device": (C.c_int, [vp, C.POINTER(PolyLoadIn), C.POINTER(PolyLoadOut)]),
        "mplx_poly_load": (C.c_int, [vp, C.POINTER(PolyLoadIn), C.POINTER(PolyLoadOut)]),
        "mplx_poly_limits_device": (C.c_int, [vp, C.POINTER(LimitsIn), C.POINTER(LimitsOut)]),
        "mplx_poly_limits": (C.c_int, [vp, C.POINTER(LimitsIn), C.POINTER(LimitsOut)]),
        "mplx_shortcut_device": (C.c_int, [vp, vp, C.POINTER(ShortcutIn), C.POINTER(ShortcutOut)]),
        "mplx_shortcut": (C.c_int, [vp, vp, C.POINTER(ShortcutIn), C.POINTER(ShortcutOut)]),
        "mplx_poly_set_lambda_device": (C.c_int, [vp, C.POINTER(LambdaIn), C.POINTER(LambdaOut)]),
        "mplx_poly_set_lambda": (C.c_int, [vp, C.POINTER(LambdaIn), C.POINTER(LambdaOut)]),
        "mplx_poly_scale_device": (C.c_int, [vp, C.POINTER(ScaleIn), C.POINTER(LambdaOut)]),
        "mplx_poly_scale": (C.c_int, [vp, C.POINTER(ScaleIn), C.POINTER(LambdaOut)]),
        "mplx_poly_scale_down_device": (C.c_int, [vp, C.POINTER(ScaleDownIn), C.POINTER(ScaleDownOut)]),
        "mplx_poly_scale_down": (C.c_int, [vp, C.POINTER(ScaleDownIn), C.POINTER(ScaleDownOut)]),
        "mplx_poly_tau_device": (C.c_int, [vp, C.POINTER(TrajTimes), C.POINTER(TauOut)]),
        "mplx_poly_tau": (C.c_int, [vp, C.POINTER(TrajTimes), C.POINTER(TauOut)]),
        "mplx_poly_clear_lambda": (C.c_int, [vp]),
        "mplx_poly_conflicts_device": (C.c_int, [vp, C.POINTER(ConflictIn), C.POINTER(ConflictOut)]),
        "mplx_poly_conflicts": (C.c_int, [vp, C.POINTER(ConflictIn), C.POINTER(ConflictOut)]),
        "mplx_traj_conflicts_device": (C.c_int, [vp, C.POINTER(TrajSet), C.POINTER(ConflictIn), C.POINTER(ConflictOut)]),
        "mplx_traj_conflicts": (C.c_int, [vp, C.POINTER(TrajSet), C.POINTER(ConflictIn), C.POINTER(ConflictOut)]),
        "mplx_table_create": (C.c_int, [vp, i64, i32, C.POINTER(vp)]),
        "mplx_table_destroy": (None, [vp]),
        "mplx_table_clear": (C.c_int, [vp]),
        "mplx_table_view_of": (C.c_int, [vp, C.POINTER(TableView)]),
        "mplx_table_stats": (C.c_int, [vp, C.POINTER(i64), C.POINTER(C.c_uint32)]),
        "mplx_table_seed": (C.c_int, [vp, vp, i64, i64, vp, C.POINTER(TableFrontier), C.POINTER(i64)]),
        "mplx_table_relax_device": (C.c_int, [vp, C.POINTER(SuccLists), i64, vp, vp, dbl, C.POINTER(TableFrontier), vp,
                                              C.POINTER(i64)]),
        "mplx_table_find_device": (C.c_int, [vp, vp, i64, vp]),
        "mplx_table_find": (C.c_int, [vp, vp, i64, vp]),
        "mplx_table_path": (C.c_int, [vp, i32, vp, vp, i64, C.POINTER(i64)]),
        "mplx_open_create": (C.c_int, [vp, C.POINTER(vp)]),
        "mplx_open_destroy": (None, [vp]),
        "mplx_open_clear": (C.c_int, [vp]),
        "mplx_open_view_of": (C.c_int, [vp, C.POINTER(OpenView)]),
        "mplx_open_push_device": (C.c_int, [vp, C.POINTER(TableFrontier), i64, dbl, i32]),
        "mplx_open_select_device": (C.c_int, [vp, dbl, C.POINTER(TableFrontier), vp, C.POINTER(OpenResult)]),
        "mplx_table_create_multi": (C.c_int, [vp, i64, i32, i32, C.POINTER(vp)]),
        "mplx_table_query_of": (C.c_int, [vp, C.POINTER(vp), C.POINTER(i32)]),
        "mplx_table_seed_multi": (C.c_int, [vp, vp, i64, i64, vp, vp, C.POINTER(TableFrontier), C.POINTER(i64)]),
        "mplx_table_find_multi_device": (C.c_int, [vp, vp, vp, i64, vp]),
        "mplx_table_find_multi": (C.c_int, [vp, vp, vp, i64, vp]),
        "mplx_open_set_goals": (C.c_int, [vp, C.POINTER(GoalSpec), i32]),
        "mplx_open_select_multi_device": (C.c_int, [vp, dbl, C.POINTER(TableFrontier), vp, C.POINTER(OpenResult)]),
        "mplx_open_select_best_device": (C.c_int, [vp, i64, dbl, C.POINTER(TableFrontier), vp, C.POINTER(OpenResult)]),
        "mplx_open_select_best_multi_device": (C.c_int, [vp, i64, dbl, C.POINTER(TableFrontier), vp, C.POINTER(OpenResult)]),
        "mplx_open_rekey_device": (C.c_int, [vp, dbl, i32, vp, vp, C.POINTER(OpenBound)]),
        "mplx_table_rebase_device": (C.c_int, [vp, i32, i32, C.POINTER(TableFrontier), vp, C.POINTER(RebaseResult)]),
        "mplx_table_rebase_multi_device": (C.c_int, [vp, vp, i32, C.POINTER(TableFrontier), vp, C.POINTER(RebaseResult)]),
        "mplx_open_push_closed_device": (C.c_int, [vp, C.POINTER(TableFrontier), i64, dbl, i32]),
        "mplx_open_set_priors_device": (C.c_int, [vp, C.POINTER(PriorSource), C.POINTER(TrajSet), C.POINTER(PriorInfo)]),
        "mplx_open_clear_priors": (C.c_int, [vp]),
        "mplx_open_prior_view_of": (C.c_int, [vp, C.POINTER(PriorView)]),
        "mplx_planner_prior_table": (C.c_int, [vp, vp, vp, i32, C.POINTER(i32), vp, C.POINTER(i32)]),
        "mplx_reserve_create": (C.c_int, [vp, C.POINTER(vp)]),
        "mplx_reserve_destroy": (None, [vp]),
        "mplx_reserve_fill_poly_device": (C.c_int, [vp, vp, C.POINTER(ConflictIn)]),
        "mplx_reserve_fill_poly": (C.c_int, [vp, vp, C.POINTER(ConflictIn)]),
        "mplx_reserve_fill_traj_device": (C.c_int, [vp, vp, C.POINTER(TrajSet), C.POINTER(ConflictIn)]),
        "mplx_reserve_fill_traj": (C.c_int, [vp, vp, C.POINTER(TrajSet), C.POINTER(ConflictIn)]),
        "mplx_reserve_shape": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(dbl)]),
        "mplx_reserve_positions": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "mplx_reserve_set_queries": (C.c_int, [vp, i32, vp, vp, vp]),
        "mplx_reserve_check_device": (C.c_int, [vp, vp, C.POINTER(SuccLists), i64, vp, vp, i64, vp, vp]),
        "mplx_reserve_park_device": (C.c_int, [vp, vp, C.POINTER(TableFrontier), i64, vp, vp]),
        "mplx_reserve_check_poly_device": (C.c_int, [vp, vp, C.POINTER(ReservePolyIn), C.POINTER(ReservePolyOut)]),
        "mplx_reserve_check_poly": (C.c_int, [vp, vp, C.POINTER(ReservePolyIn), C.POINTER(ReservePolyOut)]),
        "mplx_shortcut_timed_device": (C.c_int, [vp, vp, C.POINTER(ShortcutIn), C.POINTER(ShortcutOut), vp, vp]),
        "mplx_shortcut_timed": (C.c_int, [vp, vp, C.POINTER(ShortcutIn), C.POINTER(ShortcutOut), vp, vp]),
        "mplx_lists_add_wait_device": (C.c_int, [vp, C.POINTER(SuccLists), i64, vp, i64, vp, vp]),
        "mplx_table_rebase_timed_device": (C.c_int, [vp, vp, i32, i32, vp, C.POINTER(TableFrontier), vp, vp, vp,
                                                    C.POINTER(RebaseResult)]),
        "mplx_field_create": (C.c_int, [vp, C.POINTER(vp)]),
        "mplx_field_destroy": (None, [vp]),
        "mplx_field_build": (C.c_int, [vp, i32, vp, vp]),
        "mplx_field_shape": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i64)]),
        "mplx_field_view_of": (C.c_int, [vp, C.POINTER(FieldView)]),
        "mplx_field_download": (C.c_int, [vp, vp]),
        "mplx_field_is_stale": (C.c_int, [vp]),
        "mplx_field_passes": (C.c_int, [vp, C.POINTER(i64)]),
        "mplx_open_set_field": (C.c_int, [vp, vp, vp]),
        "mplx_open_clear_field": (C.c_int, [vp]),
        "mplx_heur_eval": (C.c_int, [vp, C.POINTER(GoalSpec), i32, vp, i64, i64, vp]),
        "mplx_heur_eval_device": (C.c_int, [vp, C.POINTER(GoalSpec), i32, vp, i64, i64, vp]),
        "mplx_open_set_heur": (C.c_int, [vp, i32]),
        "mplx_planner_set_heur_dynamics": (C.c_int, [vp, i32]),
        "mplx_table_set_time_keys": (C.c_int, [vp, i32]),
        "mplx_time_key": (C.c_uint64, [C.c_uint64, dbl]),
        "mplx_body_create": (C.c_int, [vp, C.POINTER(vp)]),
        "mplx_body_destroy": (None, [vp]),
        "mplx_body_set_shape": (C.c_int, [vp, dbl, dbl, dbl, dbl]),
        "mplx_body_fill": (C.c_int, [vp, vp, i64]),
        "mplx_body_fill_device": (C.c_int, [vp, vp, i64]),
        "mplx_body_fill_map": (C.c_int, [vp, C.c_int]),
        "mplx_body_shape": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64), vp, C.POINTER(dbl), vp, C.POINTER(i64)]),
        "mplx_body_cells": (C.c_int, [vp, vp, vp]),
        "mplx_body_check_device": (C.c_int, [vp, C.POINTER(SuccLists), i64, vp, vp, i64, i32, vp, vp]),
        "mplx_body_check_poly_device": (C.c_int, [vp, vp, C.POINTER(BodyPolyIn), C.POINTER(BodyPolyOut)]),
        "mplx_body_check_poly": (C.c_int, [vp, vp, C.POINTER(BodyPolyIn), C.POINTER(BodyPolyOut)]),
    }
    for name in SYMBOLS + MAP_UTIL_SYMBOLS + ROLLOUT_SYMBOLS + RAY_SYMBOLS + TRAJ_SYMBOLS + TABLE_SYMBOLS + OPEN_SYMBOLS + MULTI_SYMBOLS + BEST_SYMBOLS + ANYTIME_SYMBOLS + REPLAN_SYMBOLS + PRIOR_SYMBOLS + SOLVE_SYMBOLS + LIMITS_SYMBOLS + SCALE_SYMBOLS + CONFLICT_SYMBOLS + RESERVE_SYMBOLS + RESERVE_POLY_SYMBOLS + WAIT_SYMBOLS + REPLAN_TIMED_SYMBOLS + FIELD_SYMBOLS + HEUR_SYMBOLS + BODY_SYMBOLS:
        fn = getattr(L, name)  # AttributeError if the library does not export it
        fn.restype, fn.argtypes = sig[name]
    _lib = L
    return L


def check(ctx, rc):
    if rc != OK:
        msg = lib().mplx_last_error(ctx)
        raise MplxError(rc, msg.decode() if msg else "?")
