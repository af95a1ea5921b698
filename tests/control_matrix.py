"""The control matrix of the device search layer: the 16 (dim, control) pairs its kernels are instantiated for, the GPU
cases this layer's tests add for them, and per dispatch switch the GPU test cases that run each instantiation.

tests/test_control_matrix.py (no GPU) reads the `case` lines of the switches in csrc/ and holds this registry against
them: a switch that gains a case fails there until a GPU case is named here.  The GPU tests import their added cases
from this file, so a case named here is a case that runs.  No engine, no numpy: data only."""
VEL, ACC, JRK, SNP, YAW = 0x01, 0x03, 0x07, 0x0F, 0x10
FLAGS = {"VEL": VEL, "ACC": ACC, "JRK": JRK, "SNP": SNP,
         "VELxYAW": VEL | YAW, "ACCxYAW": ACC | YAW, "JRKxYAW": JRK | YAW, "SNPxYAW": SNP | YAW}
NAMES = {v: k for k, v in FLAGS.items()}
PAIRS = [(dim, name) for dim in (2, 3) for name in FLAGS]  # the 16 (dim, control) pairs


def order_of(control):
    """1 VEL .. 4 SNP of a flag or of its name."""
    c = FLAGS[control] if isinstance(control, str) else int(control)
    return 4 if c & 8 else 3 if c & 4 else 2 if c & 2 else 1


THREE = [-0.5, 0.0, 0.5]
NINE = [-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0]

# ---- tests/test_gpu_wait.py::test_add_wait_equals_the_model: (dim, control, yaw, nU, S), the axis values are THREE
WAIT_ADDED = [
    (2, "SNP", False, 9, 9),
    (2, "VELxYAW", True, 27, 32),
    (2, "JRKxYAW", True, 27, 27),
    (2, "SNPxYAW", True, 27, 32),
    (3, "SNP", False, 27, 32),
    (3, "VELxYAW", True, 81, 96),
    (3, "ACCxYAW", True, 81, 81),
    (3, "JRKxYAW", True, 81, 96),
    (3, "SNPxYAW", True, 81, 96),
    # JRK once more, with live acc rows: in the two JRK cases the file already had only movers carry an acc, and they are
    # refused by their velocity alone
    (2, "JRK", False, 9, 9),
    (3, "JRK", False, 27, 27),
]


def wait_id(dim, control, yaw, nU, S):
    return "%dd-%s-%s%s" % (dim, control.lower(), "S%d" % S if S == nU else "%dof%d" % (nU, S), "-live" if control == "JRK" else "")


# ---- tests/test_gpu_reserve.py::test_check_equals_the_model: (dim, control, axis values, yaw, S, B, park, step, Q, lanes)
RESERVE_ADDED = [
    (2, "JRK", THREE, False, 9, 70, True, 0.25, 1, None),
    (3, "JRK", THREE, False, 32, 15, False, 0.3, 1, None),
    (2, "SNP", NINE, False, 96, 70, True, 0.3, 1, None),
    (3, "SNP", THREE, False, 32, 257, True, 0.25, 3, None),
    (2, "SNPxYAW", THREE, True, 32, 15, False, 0.25, 1, None),
    (3, "VELxYAW", [-1.0, 0.0, 1.0], True, 32, 70, True, 0.3, 1, None),
]
RESERVE_ADDED_IDS = ["2d-jrk-S9-B70", "3d-jrk-27of32-B15-gone", "2d-snp-81of96-B70", "3d-snp-27of32-B257-Q3", "2d-snpyaw-27of32-B15-gone",
                     "3d-velyaw-S32-B70"]

# ---- tests/test_gpu_timed_replan.py::test_rebase_timed_equals_the_model: name, dim, control, Q, B, step, wait, n nodes, park.
# The first six are the issue's; the last four close the matrix of replan_edge_kernel (the four yaw pairs left)
TIMED_ADDED = [
    ("2d-snp-n257-B64-Q3", 2, SNP, 3, 64, 0.25, True, 257, True),
    ("3d-snp-n65-B15", 3, SNP, 1, 15, 0.3, True, 65, False),
    ("3d-jrk-n257-B70", 3, JRK, 1, 70, 0.25, True, 257, True),
    ("2d-jrkyaw-n65-B15", 2, JRK | YAW, 1, 15, 0.25, True, 65, True),
    ("2d-velyaw-n257-B64-nowait", 2, VEL | YAW, 1, 64, 0.3, False, 257, False),
    ("3d-snpyaw-n65-B1", 3, SNP | YAW, 1, 1, 0.25, True, 65, True),
    ("2d-snpyaw-n65-B15", 2, SNP | YAW, 1, 15, 0.25, True, 65, True),
    ("3d-velyaw-n65-B15-nowait", 3, VEL | YAW, 1, 15, 0.3, False, 65, True),
    ("3d-accyaw-n65-B15", 3, ACC | YAW, 1, 15, 0.25, True, 65, False),
    ("3d-jrkyaw-n65-B15", 3, JRK | YAW, 1, 15, 0.25, True, 65, True),
]
# The yaw cases of 65 nodes run on a control table of 2^(dim + 1) rows: with 27 or 81 controls the first two rounds alone
# make more than 65 nodes and the table would hold no node two edges deep (nothing kept, no hit inside the horizon)
TIMED_SMALL_U = [c[0] for c in TIMED_ADDED if c[2] & YAW and c[7] == 65]
# Limits of the added cases beyond the worlds' v_max = a_max = 1: (j_max, yaw_max).  The K = 4 cases run the j_max branch of
# limits_valid; the VELxYAW cases a heading limit that is tested against a velocity which is the control itself.  With
# velocities along multiples of 45 degrees and yaws that are multiples of 0.3, no heading is within 0.015 rad of 0.5.
TIMED_LIMITS = {c[0]: (1.0 if c[2] & 8 else 0.0, 0.5 if c[2] == (VEL | YAW) else 0.0) for c in TIMED_ADDED}

# ---- tests/test_gpu_replan_untimed.py::test_untimed_edges_of_every_pair: the (dim, control) pairs whose untimed
# replan_edge_kernel<D, K, YAW, false> ran in no GPU case before.  The worlds are those of the timed cases above: the yaw
# pairs on the control table of 2^(dim + 1) rows, the same limits (j_max for K = 4, a heading limit for VELxYAW)
UNTIMED_ADDED = [(2, VEL), (2, JRK), (2, VEL | YAW), (2, SNP | YAW), (3, VEL), (3, ACC), (3, VEL | YAW), (3, ACC | YAW),
                 (3, JRK | YAW), (3, SNP | YAW)]


def untimed_id(dim, control):
    return "%dd-%s" % (dim, NAMES[control].lower().replace("x", ""))


UNTIMED_SMALL_U = [untimed_id(d, c) for d, c in UNTIMED_ADDED if c & YAW]
UNTIMED_LIMITS = {untimed_id(d, c): (1.0 if c & 8 else 0.0, 0.5 if c == (VEL | YAW) else 0.0) for d, c in UNTIMED_ADDED}

# ---- tests/test_gpu_table.py::test_sweeps_round_by_round: id, dim, control, g_max, max_rounds, map edge.  g_max and the
# edge are chosen on the model fed with the oracle's lists (tests/test_control_matrix.py repeats that choice's conditions)
INF = float("inf")
SWEEP_ADDED = [
    ("2d-snp", 2, SNP, 50.0, 99, 32),
    ("3d-snp", 3, SNP, 56.0, 99, 64),
    ("2d-jrkyaw", 2, JRK | YAW, INF, 4, 32),
    ("3d-velyaw", 3, VEL | YAW, INF, 4, 64),
    ("2d-snpyaw", 2, SNP | YAW, INF, 4, 32),
]
# what the model on the oracle gives for them: (rounds, nodes); None with yaw controls, whose lists the device decides
SWEEP_MODEL = {"2d-snp": (5, 1890), "3d-snp": (6, 478), "2d-jrkyaw": None, "3d-velyaw": None, "2d-snpyaw": None}

# ---- the SNP world of tests/test_gpu_open.py, tests/test_gpu_multi.py and tests/test_gpu_replan.py: (dim, control, g_max, edge)
# -> per (eps, delta, capacity): (rounds, truncated selections), from tests/open_model.py on the oracle's lists
SNP_WORLD = (2, SNP, 60.0, 32)
SNP_WORLD_ROUNDS = {(1.0, 0.0, 8192): (93, 0), (1.0, 5.0, 16): (18, 15), (3.0, 5.0, 8192): (4, 0)}
SNP_WORLD_3D = (3, SNP, 56.0, 64)  # (tests/test_gpu_replan.py only)

# ---- tests/test_gpu_field.py::test_push_equals_the_model: (D, control, Q)
PUSH_ADDED = [(2, "SNP", 3), (3, "SNP", 1), (2, "JRKxYAW", 1)]


def live_start(start, dim, control):
    """A copy of the state `start` whose acc row (order >= 3) and jerk row (order 4) are live: the seed's hash folds them
    and the first primitives start from them."""
    s = [float(x) for x in start]
    if order_of(control) >= 3:
        s[2 * dim] = 0.2
    if order_of(control) >= 4:
        s[3 * dim + 1] = 0.3
    return s


# ---------------------------------------------------------------------------------------------------- the registry
def _ids(test, ids):
    return ["%s[%s]" % (test, i) for i in ids]


WAIT = "tests/test_gpu_wait.py::test_add_wait_equals_the_model"
CHECK = "tests/test_gpu_reserve.py::test_check_equals_the_model"
TIMED = "tests/test_gpu_timed_replan.py::test_rebase_timed_equals_the_model"
REBASE = "tests/test_gpu_replan.py::test_rebase_against_the_model"
SEED_HASH = "tests/test_gpu_table.py::test_seed_hashes_equal_the_oracle"
SWEEP = "tests/test_gpu_table.py::test_sweeps_round_by_round"
UNTIMED = "tests/test_gpu_replan_untimed.py::test_untimed_edges_of_every_pair"

# per switch: {instantiation: [GPU test cases that run it]}.  The key is what the switch dispatches on, with dim in front:
# (dim, control name) for the flag switches, (dim, order) for the two reservation switches.
COVERAGE = {
    # wait_kernel.hip launch_dim: lists_add_wait_kernel<D, K, YAW>
    ("wait_kernel.hip", "launch_dim"): dict(
        [((2, "VEL"), _ids(WAIT, ["2d-vel-S9"])), ((2, "ACC"), _ids(WAIT, ["2d-acc-S9", "2d-acc-81of96"])),
         ((3, "ACC"), _ids(WAIT, ["3d-acc-27of32"])), ((2, "ACCxYAW"), _ids(WAIT, ["2d-yaw-27of32"])),
         ((3, "JRK"), _ids(WAIT, ["3d-jrk-27of32", "3d-jrk-S27-live"])), ((2, "JRK"), _ids(WAIT, ["2d-jrk-81of96", "2d-jrk-S9-live"])),
         ((3, "VEL"), _ids(WAIT, ["3d-vel-27of32"]))] +
        [((c[0], c[1]), _ids(WAIT, [wait_id(*c)])) for c in WAIT_ADDED if c[1] != "JRK"]),
    # reserve_kernel.hip check_dim: reserve_check_kernel<D, K>
    ("reserve_kernel.hip", "check_dim"): {
        (2, 1): _ids(CHECK, ["2d-vel-S9-B257-gone"]),
        (2, 2): _ids(CHECK, ["2d-acc-S9-B15", "2d-acc-81of96-B70-gone", "2d-yaw-B1-gone"]),
        (3, 1): _ids(CHECK, ["3d-vel-B257-Q3", "3d-velyaw-S32-B70"]),
        (3, 2): _ids(CHECK, ["3d-acc-B70-Q3"]),
        (2, 3): _ids(CHECK, ["2d-jrk-S9-B70"]),
        (3, 3): _ids(CHECK, ["3d-jrk-27of32-B15-gone"]),
        (2, 4): _ids(CHECK, ["2d-snp-81of96-B70", "2d-snpyaw-27of32-B15-gone"]),
        (3, 4): _ids(CHECK, ["3d-snp-27of32-B257-Q3"]),
    },
    # replan_kernel.hip edge_dim<D, TIMED = true>: replan_edge_kernel<D, K, YAW, true>
    ("replan_kernel.hip", "edge_dim", "timed"): dict(
        [((2, "ACC"), _ids(TIMED, ["2d-acc-n1-B1", "2d-acc-n63-B15"])), ((2, "VEL"), _ids(TIMED, ["2d-vel-n65-B64-nowait"])),
         ((3, "ACC"), _ids(TIMED, ["3d-acc-n257-B70-Q3"])), ((2, "ACCxYAW"), _ids(TIMED, ["2d-accyaw-n257-B257"])),
         ((2, "JRK"), _ids(TIMED, ["2d-jrk-n4100-B64-Q3"])), ((3, "VEL"), _ids(TIMED, ["3d-vel-n4100-B15-nowait"]))] +
        [((c[1], NAMES[c[2]]), _ids(TIMED, [c[0]])) for c in TIMED_ADDED]),
    # replan_kernel.hip edge_dim<D, TIMED = false>: replan_edge_kernel<D, K, YAW, false>
    ("replan_kernel.hip", "edge_dim", "untimed"): dict(
        [((2, "ACC"), _ids(REBASE, ["world_key0"])), ((3, "JRK"), _ids(REBASE, ["world_key1"])),
         ((2, "SNP"), _ids(REBASE, ["2d-snp"])), ((3, "SNP"), _ids(REBASE, ["3d-snp"])),
         ((2, "ACCxYAW"), ["tests/test_gpu_replan.py::test_yaw_controls"]),
         ((2, "JRKxYAW"), ["tests/test_gpu_replan.py::test_yaw_controls_jrk"])] +
        [((d, NAMES[c]), _ids(UNTIMED, [untimed_id(d, c)])) for d, c in UNTIMED_ADDED]),
    # replan_kernel.hip reserve_dim: replan_reserve_kernel<D, K>
    ("replan_kernel.hip", "reserve_dim"): {
        (2, 1): _ids(TIMED, ["2d-vel-n65-B64-nowait", "2d-velyaw-n257-B64-nowait"]),
        (2, 2): _ids(TIMED, ["2d-acc-n63-B15", "2d-accyaw-n257-B257"]),
        (2, 3): _ids(TIMED, ["2d-jrk-n4100-B64-Q3", "2d-jrkyaw-n65-B15"]),
        (2, 4): _ids(TIMED, ["2d-snp-n257-B64-Q3", "2d-snpyaw-n65-B15"]),
        (3, 1): _ids(TIMED, ["3d-vel-n4100-B15-nowait", "3d-velyaw-n65-B15-nowait"]),
        (3, 2): _ids(TIMED, ["3d-acc-n257-B70-Q3", "3d-accyaw-n65-B15"]),
        (3, 3): _ids(TIMED, ["3d-jrk-n257-B70", "3d-jrkyaw-n65-B15"]),
        (3, 4): _ids(TIMED, ["3d-snp-n65-B15", "3d-snpyaw-n65-B1"]),
    },
    # table_kernel.hip hash_dim: table_hash_kernel<D, K, YAW>
    ("table_kernel.hip", "hash_dim"): dict(
        [((d, c), _ids(SEED_HASH, ["%dd-%s" % (d, c.lower())])) for d, c in PAIRS]),
}
for _c in SWEEP_ADDED:
    COVERAGE[("table_kernel.hip", "hash_dim")][(_c[1], NAMES[_c[2]])].append("%s[%s]" % (SWEEP, _c[0]))

# Every pair runs replan_edge_kernel in both forms: nothing is left open (tests/test_control_matrix.py holds the list exact).
UNTIMED_EDGE_NOT_RUN = []
