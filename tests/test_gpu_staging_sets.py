"""The staging walk of tests/test_gpu_staging.py, over the trajectory sets: every host-pointer call of mplx_solve.h,
mplx_limits.h, mplx_scale.h and mplx_poly_conflicts carves the ONE staging block of its context (csrc/mplx_ctx.h,
StageLayout), and here they share it on a long-lived context whose polys live as long as it does.

One long-lived context per configuration runs a fixed order of steps on two polys of k_cap 1000 / w_max 5 (and the pair
and result polys of mplx_shortcut); after every step its output equals, byte for byte, what a context created for that
step alone returns for the same inputs on polys created for that step at the smallest legal capacity.  Every output row
is filled with the same poison in both contexts before the call, so the bytes a call must leave alone (every row but
`status` of a problem with a status, segments past S_k, Lambda rows of a problem without a Lambda, columns past n of a
strided row, the last two sample rows of the waypoint form) compare as well.  No tolerance anywhere, and no row is
cleared: the headers define every byte these host calls write or leave.

A step of a kind that READS what a poly holds (info, sample, traverse, limits, set_lambda, scale, scale_down, tau,
conflicts) is "setter with this step's inputs, then the call": the setter is mplx_solve or mplx_poly_load by visit, its
status / n_segs rows are compared too.  mplx_scale.h: "A new solve or load into the poly clears every Lambda" -- that is
how a step starts from a plain poly (mplx_poly_tau, which needs a Lambda, runs mplx_poly_scale after the setter).  On odd
visits two mplx_read_cells calls (n = 1000, n = 1) run between setter and call on the long-lived context only: the first
overwrites the head of the block and frees it where it grows it, the second carves a tiny layout in a large block -- a
setter that left a pointer into the block in its poly then fails the comparison.  The one step whose setter is the
_device form is the first step of `scale`, its 00 form (neither ri_arr nor rf_arr): a layout of zero bytes, committed on
a fresh context whose block does not exist yet -- and, in the configuration whose order starts with `scale`, on the
long-lived context before anything has carved it.

Where a call has a _device twin, the twin runs on the long-lived context on uploaded copies of the inputs into poisoned
device rows and returns the same bytes wherever both forms define them (twin_defined(): the host twins of the solver,
the loader, info, samples, limits, Lambda builds and tau scatter only the defined entries of a problem, mplx_solve.h "A
problem with any bit writes its status only"; traverse, conflicts and shortcut copy whole rows).

The two timed twins of mplx_reserve_poly.h walk along (reserve_check_poly, shortcut_timed).  Their reservation table
lives as long as the context; a step fills it with mplx_reserve_fill_poly from a second set (poly `b`: this step's set
again, through the same setter) and sets one query per problem with mplx_reserve_set_queries.  The clocks decide what a
check finds, whatever the trajectories are: a problem on its twin's clock is hit, one that starts when every
reservation is gone is clear, one that starts at the table's last instant is past the horizon; a test without a GPU
shows the three values with tests/reserve_poly_model.py.  Variants by visit: radius, ignore_group, each of hit /
status / n_hit given or not (n_hit is added to: both contexts start it from the poison); h_chain_hit null or not.

Sizes, order and poison: as tests/test_gpu_staging.py says.  Two kinds of that walk, expand_lists and ray_trace, are in
this kind list unchanged, so every new kind runs directly after and directly before an old one at its largest size."""
import ctypes as C
import glob
import hashlib
import os
import re

import numpy as np
import pytest

import reserve_poly_model as RPM
import staging_walk as SW
import test_gpu_staging as OLD
from staging_walk import SIZES, assert_same_bytes, fill, poisoned, ptr, raw

SEED = 20261020
W_MAX, W = 5, 4   # waypoints per problem: w_max leaves one unused
N_UNIFORM, Q_TIMES = 4, 3
N_INSTANTS, STEP = 40, 0.12
MAX_HOP = 2
R_STEP, R_STEPS = 0.25, 96   # the reservation tables: 23.75 s of clock, past every trajectory started in its first 12 s
T_CLEAR = 12.0               # ... and at this t_start every reservation (t0 <= 1 s, at most 4 segments) is GONE
OLD_KINDS = ("expand_lists", "ray_trace")
NEW_KINDS = ("scale", "solve", "poly_load", "poly_info", "poly_sample", "poly_traverse", "poly_limits", "shortcut", "set_lambda",
             "scale_down", "poly_tau", "poly_conflicts", "reserve_check_poly", "shortcut_timed")
# `scale` first in one configuration: its first step (visit 0, the 00 form) then commits zero bytes on an empty arena
KINDS = {"2d_acc_yaw": NEW_KINDS[:6] + OLD_KINDS[:1] + NEW_KINDS[6:] + OLD_KINDS[1:],
         "3d_acc": NEW_KINDS[1:7] + OLD_KINDS[1:] + NEW_KINDS[7:] + NEW_KINDS[:1] + OLD_KINDS[:1]}
READS = ("poly_info", "poly_sample", "poly_traverse", "poly_limits", "set_lambda", "scale", "scale_down", "poly_tau", "poly_conflicts",
         "reserve_check_poly")
TIMED = ("reserve_check_poly", "shortcut_timed")  # kinds with a reservation table, filled from the second set (poly `b`)
ENTRY_POINTS = {"solve": ("mplx_solve",), "poly_load": ("mplx_poly_load",), "poly_info": ("mplx_poly_info",),
                "poly_sample": ("mplx_poly_sample",), "poly_traverse": ("mplx_poly_traverse",), "poly_limits": ("mplx_poly_limits",),
                "shortcut": ("mplx_shortcut",), "set_lambda": ("mplx_poly_set_lambda",), "scale": ("mplx_poly_scale",),
                "scale_down": ("mplx_poly_scale_down",), "poly_tau": ("mplx_poly_tau",), "poly_conflicts": ("mplx_poly_conflicts",),
                "reserve_check_poly": ("mplx_reserve_check_poly",), "shortcut_timed": ("mplx_shortcut_timed",)}
EMPTY, BAD_TIME, BAD_CHAIN, BAD_INPUT = 1, 2, 16, 128
CHECK_ROWS = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0))  # hit, status, n_hit asked for
CONFLICT_VARIANTS = ((1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (0, 0, 0, 0))  # t0, radius, group, rank


def schedule(config):
    return SW.schedule(KINDS[config], SEED)


# ---- the variant of a call, by the visit of its kind
def solve_variant(visit):
    """(every output row, durations given, wp_flags given, strides above n)"""
    return visit % 2 == 0, visit % 4 < 2, (visit // 2 + visit // 4) % 2 == 0, visit % 2 == 1


def setter_of(kind, visit):
    if kind == "scale" and visit == 0:  # (the 00 form, variant())
        return "solve_device"
    return ("solve", "poly_load")[(visit + visit // 2) % 2]


def times_variant(visit):
    """(form: 0 TRAJ_COMMAND / 1 TRAJ_WAYPOINT; 0 uniform / 1 the caller's times shared / 2 per trajectory)"""
    return (visit // 2) % 2, visit % 3


def variant(kind, visit):
    if kind == "solve":
        return solve_variant(visit)
    if kind == "poly_load":
        return ("plain", "gather")[visit % 2], visit % 4 >= 2          # strides above n
    if kind in ("poly_sample", "poly_tau"):
        return times_variant(visit)
    if kind == "poly_limits":
        return visit % 2 == 0, (visit // 2) % 2                          # every row, mode
    if kind == "shortcut":
        return (visit % 2 == 1,)                                         # a stride above n
    if kind == "set_lambda":
        return (visit // 2) % 2 == 0, visit % 2                          # n_pts given, mode
    if kind == "scale":
        return visit % 4 // 2 == 1, visit % 2 == 1, (visit // 4) % 2     # ri_arr, rf_arr, mode
    if kind == "scale_down":
        return visit % 4, (visit // 4) % 2                               # ramps: none / ri / rf / both; mode
    if kind == "poly_conflicts":
        return CONFLICT_VARIANTS[visit % 6], visit % 2, (0, 7)[(visit // 2) % 2], visit % 2 == 1   # rows, mode, chunk, pair_stride > K
    if kind == "reserve_check_poly":
        return visit % 2 == 0, (visit // 2) % 2 == 0, CHECK_ROWS[visit % 5]   # radius given, ignore_group given, rows
    if kind == "shortcut_timed":
        return visit % 2 == 1, (visit // 2) % 2 == 0                          # a stride above n, h_chain_hit given
    return ()


# ---- CPU: the order, the variants, the inputs, the completeness of the three walks
@pytest.mark.parametrize("config", sorted(KINDS))
def test_the_order_runs_every_kind_at_every_size(config):
    kinds, steps = KINDS[config], schedule(config)
    assert sorted(kinds) == sorted(NEW_KINDS + OLD_KINDS)
    assert {(kind, n) for kind, n, _ in steps} == {(kind, n) for kind in kinds for n in SIZES}
    sizes = [n for _, n, _ in steps]
    assert any(a == 3 and b == 1000 for a, b in zip(sizes, sizes[1:])) and any(a == 1000 and b == 3 for a, b in zip(sizes, sizes[1:]))
    for kind in kinds:
        assert [visit for k, _, visit in steps if k == kind] == list(range(sum(k == kind for k, _, _ in steps))), kind
    assert steps == schedule(config), "the order must not depend on the run"
    reached = {kind: {variant(kind, visit) for k, _, visit in steps if k == kind} for kind in NEW_KINDS}
    assert reached["solve"] >= {(rows, dts, fl, rows is False) for rows in (False, True) for dts in (False, True) for fl in (False, True)}
    assert reached["poly_load"] == {(f, s) for f in ("plain", "gather") for s in (False, True)}
    for kind in ("poly_sample", "poly_tau"):
        assert reached[kind] == {(f, t) for f in (0, 1) for t in (0, 1, 2)}, kind
    assert reached["poly_limits"] == {(r, m) for r in (False, True) for m in (0, 1)}
    assert reached["shortcut"] == {(False,), (True,)}
    assert reached["set_lambda"] == {(g, m) for g in (False, True) for m in (0, 1)}
    assert reached["scale"] == {(a, b, m) for a in (False, True) for b in (False, True) for m in (0, 1)}
    assert reached["scale_down"] == {(r, m) for r in range(4) for m in (0, 1)}
    assert {v[0] for v in reached["poly_conflicts"]} == set(CONFLICT_VARIANTS)
    assert {v[1:] for v in reached["poly_conflicts"]} >= {(m, c, m == 1) for m in (0, 1) for c in (0, 7)}
    assert {v[:2] for v in reached["reserve_check_poly"]} == {(r, g) for r in (False, True) for g in (False, True)}
    assert {v[2] for v in reached["reserve_check_poly"]} == set(CHECK_ROWS)
    assert reached["shortcut_timed"] == {(s, h) for s in (False, True) for h in (False, True)}
    for kind in READS:  # both setters, and the calls of another kind between setter and call
        visits = [visit for k, _, visit in steps if k == kind]
        assert {setter_of(kind, v) for v in visits} >= {"solve", "poly_load"}, kind
        assert {(setter_of(kind, v), v % 2) for v in visits} >= {(s, d) for s in ("solve", "poly_load") for d in (0, 1)}, kind
    assert steps[0][0] == ("scale" if config == "2d_acc_yaw" else "solve")
    assert (config != "2d_acc_yaw") or setter_of(*steps[0][::2]) == "solve_device"


@pytest.mark.parametrize("config", sorted(KINDS))
def test_every_kind_runs_directly_after_every_other_kinds_largest_size(config):
    kinds, steps = KINDS[config], schedule(config)
    after = {(a, b) for (a, n, _), (b, _, _) in zip(steps, steps[1:]) if n == SIZES[-1] and a != b}
    assert after == {(a, b) for a in kinds for b in kinds if a != b}
    for kind in NEW_KINDS:  # ... an old kind at its largest size among them, on both sides
        assert any((old, kind) in after for old in OLD_KINDS) and any((kind, old) in after for old in OLD_KINDS)


def test_the_first_walk_keeps_its_order():
    """tests/test_gpu_staging.py takes schedule() from tests/staging_walk.py now: the digest of its order, recorded before
    the move."""
    assert hashlib.sha256(repr(OLD.schedule()).encode()).hexdigest() == "1ca242261d96f29cdeff86def29f4ffbaec72bbfa3caa6364ee397d8df43bfa2"
    assert len(OLD.schedule()) == 209 and OLD.SEED == 20261017 and len(OLD.KINDS) == 13


@pytest.mark.parametrize("config", sorted(KINDS))
def test_every_step_has_solved_and_failed_problems(config):
    """The statuses the headers give the inputs of every step (mplx_solve.h, mplx_limits.h), predicted without a device:
    at n >= 65 at least 10 % of the problems are solved / loaded and each failure of the issue is present."""
    w = World(config)
    for i, (kind, n, visit) in enumerate(schedule(config)):
        if kind in OLD_KINDS or n < 65:
            continue
        x = w.inputs(i, kind, n, visit)
        for name in ("solve", "poly_load", "gather", "shortcut"):
            if name in x["predicted"]:
                st = x["predicted"][name]
                assert (st == 0).mean() >= 0.1 and (st & EMPTY).any(), (i, kind, name)
                assert name == "gather" or (st & (BAD_CHAIN if name == "shortcut" else BAD_TIME)).any(), (i, kind, name)


def standin_positions(x):
    """A position function [D] of (problem, local time): the waypoints of the step joined by straight lines.  It stands
    in for the trajectories of BOTH sets in the model below: the condition on the inputs must not depend on how a
    solved or loaded trajectory runs between its ends, only on who shares a clock with whom."""
    pos, tau = x["wp_pos"], x["wp_tau"]   # [D][W_MAX][n], [W_MAX][n]

    def at(k, tl):
        return np.array([np.interp(tl, tau[:, k], pos[d, :, k]) for d in range(pos.shape[0])])
    return at


def model_hits(x, n):
    """(hit, status, n_hit) of tests/reserve_poly_model.py for the inputs of a reserve_check_poly step: the table of the
    second set as include/mplx_reserve.h fills it in mode GONE, on the stand-in positions."""
    at, ok, total = standin_positions(x), x["predicted"][x["setter"]] == 0, x["total"]
    tl = np.arange(R_STEPS)[:, None] * np.float64(R_STEP) - x["res_t0"][None, :]            # [n_steps][B]
    active = ok[None, :] & (tl >= 0) & (tl <= total[None, :])
    pos = np.zeros((R_STEPS, x["wp_pos"].shape[0], n))
    for i, b in zip(*np.nonzero(active)):
        pos[i, :, b] = at(b, tl[i, b])
    table = {"pos": pos, "active": active, "included": ok, "radius": x["res_radius"], "group": x["group"]}
    use_r, use_g, _ = variant("reserve_check_poly", x["visit"])
    return RPM.check(x["predicted"][x["setter"]], np.where(ok, 1, 0), total, x["t_start"], x["c_radius"] if use_r else x["radius_all"],
                     x["c_ignore"] if use_g else None, R_STEP, table, lambda k, i, t: at(k, t))


@pytest.mark.parametrize("config", sorted(KINDS))
def test_every_check_step_has_hits_clear_problems_and_problems_past_the_horizon(config):
    """The hits tests/reserve_poly_model.py gives the inputs of every reserve_check_poly step, without a device: at
    n >= 65 a real hit (>= 0), clear (-1) and past the horizon (-2) are all present, at least 10 % of the problems are
    clear and at least 10 % are hit.  A hit is a problem on the clock of its own twin in the second set (distance 0,
    whatever the trajectory), a clear one starts at T_CLEAR, when every reservation is GONE, and one past the horizon
    starts at the table's last instant."""
    w = World(config)
    seen = 0
    for i, (kind, n, visit) in enumerate(schedule(config)):
        if kind != "reserve_check_poly" or n < 65:
            continue
        x = w.inputs(i, kind, n, visit)
        hit, status, n_hit = model_hits(x, n)
        assert (hit >= 0).mean() >= 0.1 and (hit == RPM.NO_HIT).mean() >= 0.1 and (hit == RPM.HORIZON).any(), (i, n, visit)
        assert n_hit == int((hit != RPM.NO_HIT).sum()) and (status & BAD_INPUT).any(), (i, n, visit)
        seen += 1
    assert seen >= 3


# file-local helpers that reach stage_commit -> the public entry points that call them
HELPERS = {"seed_table": ("mplx_table_seed", "mplx_table_seed_multi"), "find_host": ("mplx_table_find", "mplx_table_find_multi"),
           "expand_lists_packed": ("mplx_planner_plan",), "shortcut_host": ("mplx_shortcut", "mplx_shortcut_timed")}
# ... and the one that no walk runs: the planner stages its frontiers through the context it is attached to inside its own
# search loop (tests/test_gpu_plan.py pins it against the reference planner), not as a call a walk can place
NOT_WALKED = {"mplx_planner_plan"}


def staging_sites():
    """[(file, function)] of every function definition in csrc/*.cpp whose body contains `stage_commit(`, and the number
    of times the text occurs in those files outside comments (the scan must account for each)."""
    here = os.path.dirname(os.path.abspath(__file__))
    head = re.compile(r'^(?:extern\s+"C"\s+)?(?:static\s+|inline\s+)*[A-Za-z_][\w:<>\s\*&]*?[\s\*&]([A-Za-z_]\w*)\(')
    sites, occurrences = [], 0
    for path in sorted(glob.glob(os.path.join(here, "..", "motion_primitive_library_amd", "csrc", "*.cpp"))):
        name, depth, pending = None, 0, None
        for line in open(path):
            code = line.split("//")[0]
            occurrences += code.count("stage_commit(")
            if name is None and pending is None and not line.startswith(("}", "#", "/", " ", "\t")):
                m = head.match(code)
                pending = m.group(1) if m else None
            if pending is not None:  # a head: a definition once its `{` comes, a declaration if `;` comes first
                if "{" in code:
                    name, pending, depth = pending, None, 0
                elif code.rstrip().endswith(";"):
                    pending = None
                    continue
                else:
                    continue
            if name is not None:
                if "stage_commit(" in code:
                    sites.append((os.path.basename(path), name))
                depth += code.count("{") - code.count("}")
                if depth <= 0:
                    name = None
    return sites, occurrences


def test_every_host_pointer_call_that_stages_is_in_a_walk():
    import test_gpu_staging_search as SEARCH
    sites, occurrences = staging_sites()  # (34 sites in 17 files, mplx_rollout twice, both shortcuts in shortcut_host)
    assert len(sites) == occurrences >= 34 and sites.count(("rollout_api.cpp", "mplx_rollout")) == 2, (occurrences, sites)
    found = set()
    for _, fn in sites:
        assert fn.startswith("mplx_") or fn in HELPERS, "%s reaches stage_commit: name its public callers in HELPERS" % fn
        found.update(HELPERS.get(fn, (fn,)))
    walked = set()
    for module in (OLD, SEARCH, __import__(__name__)):
        for kind, names in module.ENTRY_POINTS.items():
            walked.update(names)
    assert found - NOT_WALKED == walked, "staged but in no walk: %s; in a walk but not staged: %s" % (
        sorted(found - NOT_WALKED - walked), sorted(walked - found))


# ---- the inputs of a step (numpy only; the same for both contexts and the twin)
class World(OLD.World):
    def extent(self):
        return np.array(self.map_dim, np.float64) * self.res

    def inputs(self, i, kind, n, visit):
        if kind in OLD_KINDS:
            return OLD.World.inputs(self, i, kind, n, visit)
        rng = np.random.default_rng(SEED + i)
        D, F, ext, k = self.dim, self.F, self.extent(), np.arange(n)
        x = {"setter": setter_of(kind, visit) if kind in READS + TIMED else None, "predicted": {}, "visit": visit}
        wide = visit % 2 == 1                                            # the strides of the inputs: above n
        sv = solve_variant(visit)
        if kind == "poly_load":
            wide = variant(kind, visit)[1]
        stride = n + 3 if wide else n
        x["stride"] = stride
        # -- waypoints (mplx_solve) and chain states (mplx_shortcut): [F][w_max][stride]
        wp = np.zeros((F, W_MAX, stride))
        pos = np.empty((D, W_MAX, n))
        pos[:, 0] = rng.uniform(0.2, 0.8, size=(D, n)) * ext[:, None]
        hop = rng.uniform(0.04, 0.12, size=(D, W_MAX - 1, n)) * rng.choice([-1.0, 1.0], size=(D, W_MAX - 1, n)) * ext[:, None, None]
        pos[:, 1:] = pos[:, :1] + np.cumsum(hop, axis=1)
        dts = rng.uniform(0.5, 1.5, size=(W_MAX - 1, n))
        n_wp = np.full(n, W, np.int32)
        n_wp[k % 13 == 3] = (k[k % 13 == 3] // 13) % 2                   # EMPTY: 0 or 1 waypoint
        n_wp[k % 13 == 9], n_wp[k % 13 == 11], n_wp[k % 29 == 5] = 2, 3, 7   # (7: above w_max, counts as w_max)
        bad = k % 13 == 7                                                # BAD_TIME, whichever way the durations come
        dts[1, bad] = np.array([0.0, -0.75, np.nan, np.inf])[(k[bad] // 13) % 4]
        coincide = bad & ((k // 13) % 2 == 1)
        pos[:, 2, coincide] = pos[:, 1, coincide]
        v = rng.uniform(0.3, 1.0, size=n)
        v[bad & ~coincide] = np.array([0.0, -1.0])[(k[bad & ~coincide] // 26) % 2]
        if n > 2:
            pos[:, :, 2], dts[:, 2], v[2] = pos[:, :, 1], dts[:, 1], v[1]    # two robots on one path: a conflict by construction
        if n > 4:
            pos[0, :, 4] += 100.0                                        # ... and one far from everybody: none
        wp[:D, :, :n] = pos
        wp[D:2 * D, :, :n] = rng.uniform(-0.2, 0.2, size=(D, W_MAX, n))
        if self.control & 0x10:
            wp[4 * D, :, :n] = rng.uniform(-1.0, 1.0, size=(W_MAX, n))
        given = np.where(np.isfinite(dts), dts, 0.0)
        wp[4 * D + 1, 1:, :n] = np.cumsum(np.where(given > 0, given, -0.25), axis=0)    # t of a chain state; a step back where dt is bad
        flags = np.zeros((W_MAX, stride), np.uint8)
        flags[:, :n] = 1 | (2 * rng.integers(0, 2, size=(W_MAX, n))) | (4 * rng.integers(0, 2, size=(W_MAX, n)))
        dts_wide = np.zeros((W_MAX - 1, stride))
        dts_wide[:, :n] = dts
        x.update(wp=wp, n_wp=n_wp, dts=dts_wide, v_arr=v, flags=flags)
        # -- segments (mplx_poly_load): c(0) .. c(5) per axis and the yaw primitive
        coeff = np.zeros((W_MAX - 1, D + 1, 6, stride))
        coeff[:, :, :, :n] = rng.uniform(-1.0, 1.0, size=(W_MAX - 1, D + 1, 6, n)) * np.array([0.5, 0.5, 0.5, 0.5, 0.4, 0.0])[None, None, :, None]
        coeff[:, :D, 5, :n] = np.moveaxis(pos[:, :W_MAX - 1], 0, 1)
        n_segs = np.where(n_wp == 7, 9, n_wp - 1).astype(np.int32)        # 0 and -1: EMPTY; 9: above w_max - 1, counts as w_max - 1
        if n > 2:
            coeff[..., 2] = coeff[..., 1]
        x.update(coeff=coeff, n_segs=n_segs)
        S = np.clip(np.where(n_wp > W_MAX, W_MAX, n_wp) - 1, 0, W_MAX - 1)
        x["predicted"]["poly_load"] = predicted_status(S, dts)
        with np.errstate(divide="ignore", invalid="ignore"):
            alloc = np.max(np.abs(np.diff(pos, axis=1)), axis=0) / v[None, :]
        x["predicted"]["solve"] = predicted_status(S, dts if sv[1] else alloc)
        x["predicted"]["solve_device"] = x["predicted"]["solve"]
        if kind == "poly_load" and variant(kind, visit)[0] == "gather":
            src_S = np.where(k % 13 == 3, 0, 1).astype(np.int32)
            idx = rng.integers(0, n, size=(W_MAX - 1, stride)).astype(np.int32)
            idx[:, :n][(np.arange(W_MAX - 1)[:, None] >= (1 + k % 4)[None, :])] = -1     # -1 ends the trajectory
            idx[0, :n][k % 13 == 4] = n + 2                               # outside the set src holds: EMPTY
            idx[0, :n][k % 13 == 8] = -1                                  # no segment at all: EMPTY
            x.update(src_n_segs=src_S, src_index=idx)
            used = np.cumsum(idx[:, :n] == -1, axis=0) == 0          # the segments before the first -1
            src_ok = predicted_status(src_S, dts[:1]) == 0
            good = (idx[:, :n] >= 0) & (idx[:, :n] < n) & src_ok[np.clip(idx[:, :n], 0, n - 1)]
            x["predicted"]["gather"] = np.where(used[0] & (~used | good).all(axis=0), 0, EMPTY).astype(np.uint8)
        if kind in ("shortcut", "shortcut_timed"):
            t = wp[4 * D + 1, :, :n]
            chain_bad = (np.diff(t, axis=0) <= 0) & (np.arange(W_MAX - 1)[:, None] < S[None, :])
            x["predicted"]["shortcut"] = np.where(S < 1, EMPTY, np.where(chain_bad.any(axis=0), BAD_CHAIN, 0)).astype(np.uint8)
        # -- times (samples, tau), virtual points and ratios (Lambda), the clock of the conflicts
        form, how = times_variant(visit)
        x["form"], x["how"] = form, how
        x["times"] = np.ascontiguousarray(rng.uniform(-0.5, 5.0, size=(n, Q_TIMES) if how == 2 else (Q_TIMES,)))
        pts = np.zeros((9, 3, stride))
        pts[:, 0, :n], pts[:, 1, :n] = rng.uniform(0.6, 1.8, size=(9, n)), rng.uniform(-0.2, 0.2, size=(9, n))
        pts[:, 2, :n] = 0.5 * np.arange(9)[:, None]
        pts[3, 0, :n][k % 13 == 6] = -0.5                                # ROBUST: MPLX_LAMBDA_BAD_POINTS
        n_pts = rng.integers(2, 10, size=n).astype(np.int32)
        n_pts[k % 13 == 5] = 1                                           # MPLX_LAMBDA_BAD_POINTS in both modes ...
        pts[1, 1, :n][k % 13 == 5] = np.inf                              # ... also where n_pts is not given
        ri, rf = rng.uniform(0.5, 2.0, size=n), rng.uniform(0.5, 2.0, size=n)
        ri[k % 13 == 5], rf[k % 13 == 6] = -1.0, np.nan
        x.update(pts=pts, n_pts=n_pts, ri=ri, rf=rf)
        r0 = 0.15 * (float(np.prod(ext)) / max(n, 65)) ** (1.0 / D)
        t0 = rng.uniform(-0.5, 1.0, size=n)
        t0[:min(n, 3)] = 0.0
        t0[k % 17 == 5] = np.array([np.nan, np.inf])[(k[k % 17 == 5] // 17) % 2]
        radius = rng.uniform(0.5, 1.5, size=n) * r0
        radius[k % 17 == 11] = -1.0
        x.update(t0=t0, radius=radius, radius_all=r0, group=(k % 5).astype(np.int32), rank=rng.integers(0, 4, size=n).astype(np.int32))
        if kind == "poly_conflicts":  # a t0 that is not finite / a negative radius, where the row is given at all
            ut, ur = variant(kind, visit)[0][:2]
            x["bad_input"] = bool((ut and (k % 17 == 5).any()) or (ur and (k % 17 == 11).any()))
        if kind in TIMED:
            # -- the second set is this step's set again (poly `b`, the same setter): reservation b is the twin of problem b,
            # on the clock res_t0.  A problem on its twin's clock is hit, one that starts at T_CLEAR finds every reservation
            # GONE, one that starts at the table's last instant leaves the horizon.
            res_t0 = rng.uniform(0.0, 1.0, size=n)
            t_start = np.where(k % 3 == 0, res_t0, np.where(k % 3 == 1, T_CLEAR, (R_STEPS - 1) * R_STEP))
            t_start[k % 17 == 5] = np.nan                                # MPLX_CONFLICT_BAD_INPUT
            c_radius = rng.uniform(0.5, 1.5, size=n) * r0
            c_radius[k % 17 == 11] = -1.0                                # ... where the row is given
            used = dts if (x["setter"] == "poly_load" or sv[1]) else alloc
            with np.errstate(invalid="ignore"):
                dur = np.where(np.arange(W_MAX - 1)[:, None] < S[None, :], np.where(np.isfinite(used) & (used > 0), used, 0.0), 0.0)
            x.update(res_t0=res_t0, res_radius=rng.uniform(0.5, 1.5, size=n) * r0, t_start=t_start, c_radius=c_radius,
                     c_ignore=((k + 1) % 5).astype(np.int32), total=dur.sum(axis=0), wp_pos=pos,
                     wp_tau=np.concatenate([np.zeros((1, n)), np.cumsum(dur, axis=0)]),
                     q_t0=rng.uniform(0.0, 1.0, size=n), q_ignore=(k % 7 - 1).astype(np.int32),
                     # (every fourth query as wide as the map: its chain is hit while any reservation is there; an EMPTY chain never is)
                     q_radius=np.where(k % 4 == 0, 10.0, rng.uniform(0.5, 1.5, size=n) * r0))
        return x


def predicted_status(S, dts):
    """MPLX_SOLVE_EMPTY for S < 1, else MPLX_SOLVE_BAD_TIME for a duration of a segment below S that is not finite or <= 0."""
    used = np.arange(dts.shape[0])[:, None] < S[None, :]
    with np.errstate(invalid="ignore"):
        bad = (used & ~(np.isfinite(dts) & (dts > 0))).any(axis=0)
    return np.where(S < 1, EMPTY, np.where(bad, BAD_TIME, 0)).astype(np.uint8)


# ---- the polys of a context
class Polys:
    def __init__(self, abi, env, k_cap, kind=None):
        """`kind`: only what a step of that kind needs (a context created for one step)."""
        self.abi, self.env, self.h = abi, env, {}
        L = abi.lib()
        want = {"a": (k_cap, W_MAX)}
        if kind in (None, "poly_load"):
            want["src"] = (k_cap, 2 if kind else W_MAX)
        if kind in (None, "shortcut", "shortcut_timed"):
            want["pairs"], want["result"] = (k_cap * (W_MAX - 1) * MAX_HOP, 2), (k_cap, W_MAX)
        if kind in (None,) + TIMED:
            want["b"] = (k_cap, W_MAX)
        for name, (cap, w_max) in want.items():
            self.h[name] = SW.handle(abi, env._ctx, L.mplx_poly_create, env._ctx, cap, w_max)
        self.table = SW.handle(abi, env._ctx, L.mplx_reserve_create, env._ctx) if kind in (None,) + TIMED else None

    def free(self):
        for h in self.h.values():
            self.abi.lib().mplx_poly_destroy(h)
        if self.table is not None:
            self.abi.lib().mplx_reserve_destroy(self.table)
        self.h, self.table = {}, None


# ---- the rows a call is asked for: name -> (dtype, shape)
def lambda_rows(n):
    return {"status": ("u1", (n,)), "n_lseg": ("<i4", (n,)), "total": ("<f8", (n,)), "Ts": ("<f8", (W_MAX, n)), "segs": ("<f8", (64, n))}


def out_spec(w, kind, n, visit, x):
    D, F = w.dim, w.F
    N = 2 * 2  # ACC ends: so = 1
    if kind in ("solve", "solve_device"):
        cs = x["stride"]
        s = {"status": ("u1", (n,)), "n_segs": ("<i4", (n,)), "total_time": ("<f8", (n,))}
        if solve_variant(visit)[0] and kind == "solve":
            s.update(coeff=("<f8", ((W_MAX - 1) * N * D, cs)), dts_out=("<f8", (W_MAX - 1, cs)), yaw_coeff=("<f8", (2 * (W_MAX - 1), cs)),
                     taus=("<f8", (W_MAX, cs)))
        return s
    if kind in ("poly_load", "gather"):
        return {"status": ("u1", (n,)), "n_segs": ("<i4", (n,)), "total_time": ("<f8", (n,)), "taus": ("<f8", (W_MAX, x["stride"]))}
    if kind == "poly_info":
        return {"status": ("u1", (n,)), "n_segs": ("<i4", (n,)), "total_time": ("<f8", (n,)), "effort": ("<f8", (5, n)),
                "seg_state": ("<f8", (F, W_MAX, n))}
    if kind == "poly_sample":
        return {"out": ("<f8", (4 * D + 3, n, N_UNIFORM + 1 if x["how"] == 0 else Q_TIMES)), "status": ("u1", (n,))}
    if kind == "poly_traverse":
        return {"status": ("u1", (n,)), "cost": ("<f8", (n,)), "n_samples": ("<i4", (n,)), "n_cells": ("<i4", (n,)), "stop_sample": ("<i4", (n,))}
    if kind == "poly_limits":
        s = {"valid": ("u1", (n,))}
        if variant(kind, visit)[0]:
            s.update(max_vel=("<f8", (D, n)), max_acc=("<f8", (D, n)), max_jrk=("<f8", (D, n)), exceed=("u1", (n,)), first_bad=("<i4", (n,)))
        return s
    if kind in ("shortcut", "shortcut_timed"):
        s = {"status": ("u1", (n,)), "n_keep": ("<i4", (n,)), "keep": ("<i4", (W_MAX, x["stride"])), "cost": ("<f8", (n,)),
             "chain_cost": ("<f8", (n,)), "edge_cost": ("<f8", (n, W_MAX - 1, MAX_HOP))}
        if kind == "shortcut_timed" and variant(kind, visit)[1]:
            s["chain_hit"] = ("<i8", (n,))
        return s
    if kind == "reserve_check_poly":
        rows = variant(kind, visit)[2]
        return {k: v for k, v, asked in (("hit", ("<i8", (n,)), rows[0]), ("status", ("u1", (n,)), rows[1]), ("n_hit", ("<i8", (1,)), rows[2])) if asked}
    if kind in ("set_lambda", "scale"):
        return lambda_rows(n)
    if kind == "scale_down":
        s = {"scaled": ("u1", (n,)), "max_l": ("<f8", (n,)), "t_lo": ("<f8", (n,)), "t_hi": ("<f8", (n,))}
        s.update(lambda_rows(n))
        return s
    if kind == "poly_tau":
        c = N_UNIFORM + 1 if x["how"] == 0 else Q_TIMES
        return {"tau": ("<f8", (n, c)), "lambda": ("<f8", (n, c)), "lambda_dot": ("<f8", (n, c)), "found": ("u1", (n, c))}
    assert kind == "poly_conflicts"
    s = {"first_step": ("<i4", (n,)), "first_partner": ("<i4", (n,)), "min_d2": ("<f8", (n,)), "status": ("u1", (n,))}
    if n <= 257:
        s["pair_first"] = ("<i4", (n, n + 5 if variant(kind, visit)[3] else n))
    return s


def times_struct(abi, x, I):
    t = abi.TrajTimes()
    t.form = x["form"]
    if x["how"] == 0:
        t.n_uniform = N_UNIFORM
    else:
        t.times, t.n_times, t.time_stride = I["times"], Q_TIMES, Q_TIMES if x["how"] == 2 else 0
    return t


def lambda_out(abi, P, n):
    return fill(abi.LambdaOut(), {k: P.get(k) for k in ("status", "n_lseg", "total", "Ts", "segs")}, ts_stride=n, seg_stride=n)


def call(abi, polys, w, kind, n, visit, x, P, I, sfx="", poly="a"):
    """One call through the C ABI: P names the output rows, I the inputs (host addresses, or device addresses for the
    _device form; src_index is device memory in both)."""
    L, ctx, a = abi.lib(), polys.env._ctx, polys.h[poly]
    stride = x["stride"]
    if kind in ("solve", "solve_device"):
        _, given, flagged, _ = solve_variant(visit)
        i = fill(abi.SolveIn(), {}, waypoints=I["wp"], n_prob=n, w_max=W_MAX, wp_stride=stride, n_wp=I["n_wp"], v=1.0, control=w.control, yaw_control=1)
        if given:
            i.dts, i.dt_stride = I["dts"], stride
        else:
            i.v_arr = I["v_arr"]
        if flagged:
            i.wp_flags, i.flag_stride = I["flags"], stride
        o = fill(abi.SolveOut(), P, coeff_stride=stride, dts_out_stride=stride, yaw_stride=stride, taus_stride=stride)
        rc = getattr(L, "mplx_solve" + ("_device" if kind == "solve_device" else sfx))(a, C.byref(i), C.byref(o))
    elif kind == "poly_load":
        i = fill(abi.PolyLoadIn(), {}, n_prob=n, w_max=W_MAX, control=w.control, n_segs=I["n_segs"], dts=I["dts"], dt_stride=stride,
                 coeff=I["coeff"], coeff_stride=stride)
        rc = getattr(L, "mplx_poly_load" + sfx)(a, C.byref(i), C.byref(fill(abi.PolyLoadOut(), P, taus_stride=stride)))
    elif kind == "load_src":  # the source of a gather: one segment per problem (none where src_n_segs is 0)
        i = fill(abi.PolyLoadIn(), {}, n_prob=n, w_max=2, control=w.control, n_segs=I["src_n_segs"], dts=I["dts"], dt_stride=stride,
                 coeff=I["coeff"], coeff_stride=stride)
        rc = L.mplx_poly_load(polys.h["src"], C.byref(i), C.byref(abi.PolyLoadOut()))
    elif kind == "gather":
        i = fill(abi.PolyLoadIn(), {}, n_prob=n, w_max=W_MAX, control=w.control, src=polys.h["src"], src_index=I["src_index"], index_stride=stride)
        rc = getattr(L, "mplx_poly_load" + sfx)(a, C.byref(i), C.byref(fill(abi.PolyLoadOut(), P, taus_stride=stride)))
    elif kind == "poly_info":
        rc = getattr(L, "mplx_poly_info" + sfx)(a, C.byref(fill(abi.TrajInfoOut(), P, effort_stride=n, seg_stride=n)))
    elif kind == "poly_sample":
        c = N_UNIFORM + 1 if x["how"] == 0 else Q_TIMES
        o = fill(abi.TrajSampleOut(), P, row_stride=n * c, sample_stride=c)
        rc = getattr(L, "mplx_poly_sample" + sfx)(a, C.byref(times_struct(abi, x, I)), C.byref(o))
    elif kind == "poly_traverse":
        rc = getattr(L, "mplx_poly_traverse" + sfx)(a, 0, C.byref(fill(abi.TrajTraverseOut(), P)))
    elif kind == "poly_limits":
        i = fill(abi.LimitsIn(), {}, mv=1.0, ma=1.0, mj=2.0, mode=variant(kind, visit)[1])
        rc = getattr(L, "mplx_poly_limits" + sfx)(a, C.byref(i), C.byref(fill(abi.LimitsOut(), P, max_stride=n)))
    elif kind == "shortcut":
        i = fill(abi.ShortcutIn(), {}, states=I["wp"], n_query=n, w_max=W_MAX, control=w.control, stride=stride, n_wp=I["n_wp"], max_hop=MAX_HOP)
        o = fill(abi.ShortcutOut(), P, keep_stride=stride)
        rc = getattr(L, "mplx_shortcut" + sfx)(polys.h["pairs"], polys.h["result"], C.byref(i), C.byref(o))
    elif kind == "fill_table":  # the reservation table of the step from the second set, then one query per problem
        i = fill(abi.ConflictIn(), {}, step=R_STEP, n_steps=R_STEPS, mode=1, t0=I["res_t0"], radius=I["res_radius"], group=I["group"])
        abi.check(ctx, L.mplx_reserve_fill_poly(polys.table, polys.h["b"], C.byref(i)))
        rc = L.mplx_reserve_set_queries(polys.table, n, I["q_t0"], I["q_radius"], I["q_ignore"])
    elif kind == "reserve_check_poly":
        use_r, use_g, _ = variant(kind, visit)
        i = fill(abi.ReservePolyIn(), {}, t_start=I["t_start"], radius=I["c_radius"] if use_r else None, radius_all=x["radius_all"],
                 ignore_group=I["c_ignore"] if use_g else None)
        rc = getattr(L, "mplx_reserve_check_poly" + sfx)(polys.table, a, C.byref(i), C.byref(fill(abi.ReservePolyOut(), P)))
    elif kind == "shortcut_timed":
        i = fill(abi.ShortcutIn(), {}, states=I["wp"], n_query=n, w_max=W_MAX, control=w.control, stride=stride, n_wp=I["n_wp"], max_hop=MAX_HOP)
        o = fill(abi.ShortcutOut(), {k: v for k, v in P.items() if k != "chain_hit"}, keep_stride=stride)
        rc = getattr(L, "mplx_shortcut_timed" + sfx)(polys.h["pairs"], polys.h["result"], C.byref(i), C.byref(o), polys.table, P.get("chain_hit"))
    elif kind == "set_lambda":
        with_n, mode = variant(kind, visit)
        i = fill(abi.LambdaIn(), {}, pts=I["pts"], stride=stride, n_pts=I["n_pts"] if with_n else None, mode=mode)
        rc = getattr(L, "mplx_poly_set_lambda" + sfx)(a, C.byref(i), C.byref(lambda_out(abi, P, n)))
    elif kind == "scale":
        ri_arr, rf_arr, mode = variant(kind, visit)
        i = fill(abi.ScaleIn(), {}, ri=0.8, rf=1.25, ri_arr=I["ri"] if ri_arr else None, rf_arr=I["rf"] if rf_arr else None, mode=mode)
        rc = getattr(L, "mplx_poly_scale" + sfx)(a, C.byref(i), C.byref(lambda_out(abi, P, n)))
    elif kind == "scale_for_tau":  # (mplx_poly_tau needs a Lambda; the scalars, no array)
        i = fill(abi.ScaleIn(), {}, ri=0.7, rf=1.6, mode=visit % 2)
        rc = L.mplx_poly_scale(a, C.byref(i), C.byref(abi.LambdaOut()))
    elif kind == "scale_down":
        ramps, mode = variant(kind, visit)
        i = fill(abi.ScaleDownIn(), {}, mv=0.8, ma=0.7, ri=1.0 if ramps & 1 else 0.0, rf=1.0 if ramps & 2 else 0.0, mode=mode)
        o = fill(abi.ScaleDownOut(), {k: P.get(k) for k in ("scaled", "max_l", "t_lo", "t_hi")}, lam=lambda_out(abi, P, n))
        rc = getattr(L, "mplx_poly_scale_down" + sfx)(a, C.byref(i), C.byref(o))
    elif kind == "poly_tau":
        rc = getattr(L, "mplx_poly_tau" + sfx)(a, C.byref(times_struct(abi, x, I)), C.byref(fill(abi.TauOut(), P, stride=N_UNIFORM + 1 if x["how"] == 0 else Q_TIMES)))
    else:
        assert kind == "poly_conflicts", kind
        (ut, ur, ug, uk), mode, chunk, wide = variant(kind, visit)
        i = fill(abi.ConflictIn(), {}, step=STEP, n_steps=N_INSTANTS, mode=mode, t0=I["t0"] if ut else None, radius=I["radius"] if ur else None,
                 radius_all=x["radius_all"], group=I["group"] if ug else None, rank=I["rank"] if uk else None, chunk_steps=chunk)
        o = fill(abi.ConflictOut(), P, pair_stride=n + 5 if wide else n)
        rc = getattr(L, "mplx_poly_conflicts" + sfx)(a, C.byref(i), C.byref(o))
    abi.check(ctx, rc)


ARRAYS = ("wp", "n_wp", "dts", "v_arr", "flags", "coeff", "n_segs", "src_n_segs", "times", "pts", "n_pts", "ri", "rf", "t0", "radius", "group", "rank",
          "res_t0", "res_radius", "t_start", "c_radius", "c_ignore", "q_t0", "q_radius", "q_ignore")
NEEDS = {"solve": ("wp", "n_wp", "dts", "v_arr", "flags"), "poly_load": ("n_segs", "dts", "coeff"), "poly_sample": ("times",), "poly_tau": ("times",),
         "shortcut": ("wp", "n_wp"), "shortcut_timed": ("wp", "n_wp"), "reserve_check_poly": ("t_start", "c_radius", "c_ignore"), "set_lambda": ("pts", "n_pts"), "scale": ("ri", "rf"), "poly_conflicts": ("t0", "radius", "group", "rank")}


def host_rows(spec):
    out = {k: poisoned(dt, shape) for k, (dt, shape) in spec.items()}
    P = {k: a.ctypes.data for k, a in out.items()}
    return out, P


def host_step(engine, polys, w, kind, n, visit, x, long_lived):
    """The step on one context: name -> row.  The rows of the setter are `set_*`, those of the result poly `res_*`."""
    abi, env = engine._abi, polys.env
    I = {k: ptr(x[k]) for k in ARRAYS if k in x}
    dev, out = SW.Device(engine, env), {}
    between = long_lived and visit % 2 == 1
    try:
        if x["setter"]:
            setter = x["setter"]
            target = "b" if kind == "shortcut_timed" else "a"  # (the timed shortcut takes the chain states themselves: its setter fills the second set)
            got, P = host_rows(out_spec(w, "solve_device" if setter != "poly_load" else "poly_load", n, visit, x))
            if setter == "solve_device":  # the same rows through device memory: nothing is staged
                Id = {k: dev.up(x[k]) for k in ("wp", "n_wp", "dts", "v_arr", "flags")}
                Pd = dev.rows({k: v for k, v in out_spec(w, "solve_device", n, visit, x).items()})
                call(abi, polys, w, "solve_device", n, visit, x, Pd, Id)
                got = dev.download()
            else:
                call(abi, polys, w, setter, n, visit, x, P, I, poly=target)
            out.update({"set_" + k: v for k, v in got.items()})
            if between:
                SW.disturb(abi, env, w.cells.size)
        if kind == "poly_load" and variant(kind, visit)[0] == "gather":
            call(abi, polys, w, "load_src", n, visit, x, {}, I)
            if between:
                SW.disturb(abi, env, w.cells.size)
            I["src_index"] = dev.up(x["src_index"])
            kind = "gather"
        if kind == "poly_tau":
            call(abi, polys, w, "scale_for_tau", n, visit, x, {}, I)
            if between:
                SW.disturb(abi, env, w.cells.size)
        if kind in TIMED:
            if kind == "reserve_check_poly":
                call(abi, polys, w, x["setter"], n, visit, x, {}, I, poly="b")
            call(abi, polys, w, "fill_table", n, visit, x, {}, I)
            if between:
                SW.disturb(abi, env, w.cells.size)
        got, P = host_rows(out_spec(w, kind, n, visit, x))
        call(abi, polys, w, kind, n, visit, x, P, I)
        out.update(got)
        if kind in ("shortcut", "shortcut_timed"):  # what the call left in its result poly
            got, P = host_rows({k: v for k, v in out_spec(w, "poly_info", n, visit, x).items() if k != "seg_state"})
            L = abi.lib()
            abi.check(env._ctx, L.mplx_poly_info(polys.h["result"], C.byref(fill(abi.TrajInfoOut(), P, effort_stride=n))))
            out.update({"res_" + k: v for k, v in got.items()})
    finally:
        dev.free()
    return out


def device_step(engine, polys, w, kind, n, visit, x):
    """The _device twin of the call of a step, on the poly as the host step left it."""
    abi = engine._abi
    dev = SW.Device(engine, polys.env)
    try:
        I = {k: dev.up(x[k]) for k in NEEDS.get(kind, ())}
        if kind == "poly_load" and variant(kind, visit)[0] == "gather":
            I["src_index"] = dev.up(x["src_index"])
            kind = "gather"
        spec = out_spec(w, kind, n, visit, x)
        P = dev.rows(spec)
        call(abi, polys, w, kind, n, visit, x, P, I, "_device")
        return dev.download()
    finally:
        dev.free()


def twin_defined(kind, n, host):
    """name -> mask of the entries BOTH forms define (True alone: the whole row)."""
    def pad(m, width):  # a mask over the n problems, over a row of `width` >= n columns
        return np.concatenate([m, np.zeros(width - n, bool)])

    whole = {k: True for k in host if not k.startswith(("set_", "res_"))}
    if kind in ("poly_traverse", "poly_conflicts", "shortcut", "shortcut_timed", "reserve_check_poly"):
        return whole
    ok = host["set_status"] == 0 if "set_status" in host else host["status"] == 0
    S = np.where(ok, host["set_n_segs"] if "set_n_segs" in host else host["n_segs"], 0)
    m = {}
    for k in whole:
        a = host[k]
        if k == "status" and kind in ("solve", "poly_load", "gather", "poly_info", "poly_sample"):
            m[k] = True
        elif kind in ("solve", "poly_load", "gather", "poly_info"):
            if a.ndim == 1:
                m[k] = ok
            elif k == "seg_state":
                m[k] = np.broadcast_to((np.arange(W_MAX)[:, None] <= S[None, :]) & ok[None, :], a.shape)
            elif k == "effort":
                m[k] = np.broadcast_to(ok[None, :], a.shape)
            else:  # rows of segment r // per (taus: of waypoint r), columns past n never
                per = {"coeff": a.shape[0] // (W_MAX - 1), "dts_out": 1, "yaw_coeff": 2, "taus": 1}[k]
                seg = np.arange(a.shape[0])[:, None] // per
                m[k] = (seg <= pad(S, a.shape[1])[None, :]) if k == "taus" else (seg < pad(S, a.shape[1])[None, :])
                m[k] = m[k] & pad(ok, a.shape[1])[None, :]
        elif kind == "poly_sample":
            m[k] = np.broadcast_to(ok[None, :, None], a.shape)
        elif kind == "poly_limits":
            m[k] = np.broadcast_to(ok, a.shape)
        elif kind == "poly_tau":
            m[k] = np.broadcast_to(ok[:, None], a.shape)
        else:  # the Lambda builds
            built = ok & (host["scaled"] == 1) if kind == "scale_down" else ok
            lam = built & (host["status"] == 0)
            if k == "scaled":
                m[k] = ok
            elif k in ("max_l", "t_lo", "t_hi", "status"):
                m[k] = built
            elif k in ("n_lseg", "total"):
                m[k] = lam
            elif k == "Ts":
                m[k] = (np.arange(W_MAX)[:, None] <= S[None, :]) & lam[None, :]
            else:
                m[k] = (np.arange(64)[:, None] // 8 < np.where(lam, host["n_lseg"], 0)[None, :]) & lam[None, :]
    return m


def assert_equals_twin(kind, n, host, dev, what):
    for k, mask in twin_defined(kind, n, host).items():
        h, d = host[k], dev[k]
        assert h.shape == d.shape, (what, k)
        if mask is True:
            mask = np.ones(h.shape, bool)
        assert n < SIZES[-1] or mask.any(), "%s: row `%s`: nothing that both forms define" % (what, k)
        assert np.array_equal(raw(h[mask]), raw(d[mask])), "%s: row `%s` differs from the _device form (%d defined entries)" % (
            what, k, int(mask.sum()))


def assert_not_vacuous(kind, n, x, want, what):
    """On the output of the fresh context, the reference: the step has solved and failed problems, hits and misses."""
    if n < 65:
        return
    checks = [(x["setter"], "set_status")] if x["setter"] else []
    checks += {"solve": [("solve", "status")], "shortcut": [("shortcut", "status")], "shortcut_timed": [("shortcut", "status")],
               "poly_load": [("gather" if "src_index" in x else "poly_load", "status")]}.get(kind, [])
    for name, row in checks:
        st, pred = want[row], x["predicted"][name]
        assert np.array_equal(st & (EMPTY | BAD_TIME | BAD_CHAIN), pred), what + ": not the statuses the headers give these inputs"
        assert (st == 0).mean() >= 0.1 and (st & EMPTY).any(), what
        assert name == "gather" or (st & (BAD_CHAIN if name == "shortcut" else BAD_TIME)).any(), what
    if kind in ("set_lambda", "scale", "scale_down", "poly_traverse", "poly_info", "poly_sample", "poly_conflicts"):
        assert (want["status"] == 0).mean() >= 0.1, what + ": fewer than 10 % of the items at status 0"
    if kind == "set_lambda" or (kind == "scale" and any(variant(kind, x["visit"])[:2])):  # (the scalars of `scale` are good ratios)
        assert (want["status"] == 32).any(), what + ": no MPLX_LAMBDA_BAD_POINTS"
    if kind == "reserve_check_poly" and "hit" in want:
        hit = want["hit"]
        assert (hit >= 0).mean() >= 0.1 and (hit == RPM.NO_HIT).mean() >= 0.1 and (hit == RPM.HORIZON).any(), what + ": hits, clear, past the horizon"
    if kind == "shortcut_timed" and "chain_hit" in want:
        assert (want["chain_hit"] != RPM.NO_HIT).any() and (want["chain_hit"] == RPM.NO_HIT).any(), what + ": no chain with a hit, or none without"
    if kind == "poly_conflicts":
        included = (want["set_status"] == 0) & ((want["status"] & BAD_INPUT) == 0)
        assert (want["first_step"][included] >= 0).any() and (want["first_step"][included] == -1).any(), what + ": no hit, or no miss"
        assert ((want["status"] & BAD_INPUT) != 0).any() == bool(x["bad_input"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(KINDS))
def test_trajectory_sets_share_the_staging_block_of_a_long_lived_context(engine, monkeypatch, config):
    monkeypatch.setenv("MPLX_ARENA_KB", "1")  # read by mplx_create: every lists batch takes the large path
    abi, w = engine._abi, World(config)
    env = engine.EnvMap(w.dim, 0)
    w.configure(env)
    polys = Polys(abi, env, SIZES[-1])
    stats = {}
    for i, (kind, n, visit) in enumerate(schedule(config)):
        what = "%s step %d: %s n=%d visit %d" % (config, i, kind, n, visit)
        x = w.inputs(i, kind, n, visit)
        fresh = engine.EnvMap(w.dim, 0)
        w.configure(fresh)
        if kind in OLD_KINDS:
            want = OLD.host_call(abi, fresh, w, kind, n, x)
            fresh.close()
            got = OLD.host_call(abi, env, w, kind, n, x)
            assert_same_bytes(got, want, what)
            OLD.assert_equals_twin(w, kind, n, got, OLD.device_call(engine, env, w, kind, n, x), what)
            stats.setdefault(kind, []).append((n, None))
            continue
        own = Polys(abi, fresh, n, kind)
        want = host_step(engine, own, w, kind, n, visit, x, False)
        own.free()
        fresh.close()
        assert_not_vacuous(kind, n, x, want, what)
        got = host_step(engine, polys, w, kind, n, visit, x, True)
        assert_same_bytes(got, want, what)
        assert_equals_twin("gather" if kind == "poly_load" and "src_index" in x else kind, n, got,
                           device_step(engine, polys, w, kind, n, visit, x), what)
        row = want["status"] if "status" in want else want.get("set_status")
        stats.setdefault(kind, []).append((n, None if row is None else float((row == 0).mean())))
    polys.free()
    env.close()
    for kind in KINDS[config]:
        at_1000 = [s for n, s in stats[kind] if n == SIZES[-1] and s is not None]
        print("%s %-14s steps %3d  status 0 at n = 1000: %s" % (config, kind, len(stats[kind]),
              "%.3f .. %.3f" % (min(at_1000), max(at_1000)) if at_1000 else "-"))
