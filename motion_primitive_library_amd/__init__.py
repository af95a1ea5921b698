"""motion_primitive_library_amd -- MI355X-native successor expansion for
search-based motion-primitive planning (the env_map<Dim>::get_succ path of
sikang/motion_primitive_library), behind the C ABI of include/mplx.h.

The compute path is csrc/libmplx.so (hand-written HIP for gfx950).  Importing
the package does not need a GPU; creating an EnvMap does, and there is no CPU
fallback of any kind.
"""
from . import _abi, shard, workloads
from .env import (ACC, ACCxYAW, JRK, JRKxYAW, SNP, SNPxYAW, VEL, VELxYAW, SLOT_BLOCKED, SLOT_FINITE,
                  SLOT_SKIP_DYN, SLOT_SKIP_SAME, ROLLOUT_BAD_ACTION, ROLLOUT_HEADING_BAND, RAY_LEFT_MAP, RAY_HIT, RAY_BAD,
                  RAY_TRUNCATED, FLAG_GOAL_BLOCKED, TRAJ_EMPTY, TRAJ_BAD_ACTION, TRAJ_BAD, TRAJ_COMMAND,
                  TRAJ_WAYPOINT, SOLVE_EMPTY, SOLVE_BAD_TIME, SOLVE_SINGULAR, USE_POS, USE_VEL, USE_ACC, PolyTrajSet, SolveOut,
                  LIMITS_REFERENCE, LIMITS_ALL_ROOTS, EXCEED_VEL, EXCEED_ACC, EXCEED_JRK, PolyLimits, LoadOut, ShortcutResult, SHORTCUT_BAD_CHAIN,
                  SCALE_REFERENCE, SCALE_ROBUST, LAMBDA_BAD_POINTS, LAMBDA_NOT_POSITIVE, LAMBDA_MAX_SEGS, LambdaRows,
                  CONFLICT_PARK, CONFLICT_GONE, CONFLICT_BAD_INPUT, Conflicts, ConflictResult,
                  TrajInfo, TrajSamples, TrajTraverse, Rays, DeviceArray, EnvMap, Lists, PackedLists,
                  Rollouts, Slots, Waypoint, lists_from_dense, pack_host_lists)

from .table import NodeTable, TableFrontier
from .search import MultiSearchResult, OpenSet, Prior, SearchResult, pick_fastest, stagger
from .planner import MapPlanner, MapUtil, Trajectory, TrajSolver

__all__ = ["MapPlanner", "MapUtil", "Trajectory", "EnvMap", "Waypoint", "Slots", "Lists", "lists_from_dense", "PackedLists", "pack_host_lists", "DeviceArray", "workloads", "VEL", "ACC", "JRK", "SNP", "VELxYAW",
           "ACCxYAW", "JRKxYAW", "SNPxYAW", "SLOT_SKIP_SAME", "SLOT_FINITE", "SLOT_BLOCKED", "SLOT_SKIP_DYN",
           "ROLLOUT_BAD_ACTION", "ROLLOUT_HEADING_BAND", "Rollouts", "Rays", "RAY_LEFT_MAP", "RAY_HIT", "RAY_BAD", "RAY_TRUNCATED",
           "FLAG_GOAL_BLOCKED", "TRAJ_EMPTY", "TRAJ_BAD_ACTION", "TRAJ_BAD", "TRAJ_COMMAND", "TRAJ_WAYPOINT", "TrajInfo",
           "TrajSamples", "TrajTraverse", "NodeTable", "TableFrontier", "OpenSet", "SearchResult", "MultiSearchResult", "Prior",
           "PolyTrajSet", "SolveOut", "TrajSolver", "SOLVE_EMPTY", "SOLVE_BAD_TIME", "SOLVE_SINGULAR", "USE_POS", "USE_VEL", "USE_ACC",
           "LIMITS_REFERENCE", "LIMITS_ALL_ROOTS", "EXCEED_VEL", "EXCEED_ACC", "EXCEED_JRK", "PolyLimits", "LoadOut", "ShortcutResult", "SHORTCUT_BAD_CHAIN", "pick_fastest",
           "SCALE_REFERENCE", "SCALE_ROBUST", "LAMBDA_BAD_POINTS", "LAMBDA_NOT_POSITIVE", "LAMBDA_MAX_SEGS", "LambdaRows",
           "CONFLICT_PARK", "CONFLICT_GONE", "CONFLICT_BAD_INPUT", "Conflicts", "ConflictResult", "stagger"]
