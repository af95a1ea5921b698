"""Hand cases for tests/wait_model.py, the sequential restatement of include/mplx_wait.h and of the park veto of
include/mplx_reserve.h, and the two scenarios of tests/test_gpu_wait.py on the models.  No GPU: the device side is held
against the same model in tests/test_gpu_wait.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wait_model as WM  # noqa: E402
from table_model import oracle_provider  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEL, ACC, JRK, ACCxYAW = 0x01, 0x03, 0x07, 0x13
U9 = np.array([[x, y] for x in (-0.5, 0.0, 0.5) for y in (-0.5, 0.0, 0.5)])


def row2(pos, vel=(0, 0), acc=(0, 0), yaw=0.0, t=0.0):
    return np.array(list(pos) + list(vel) + list(acc) + [0, 0] + [yaw, t], dtype=np.float64)


def lists_for(n, S, count, with_state=True):
    L = {"stride": S, "count": np.array(count, np.int32), "action": np.full(n * S, -7, np.int32), "cost": np.full(n * S, -1.0),
         "hash": np.zeros(n * S, np.uint64)}
    if with_state:
        L["state"] = np.full((10, n * S), -3.0)
    return L


# ---------------------------------------------------------------------------------------------------- eligibility
def test_eligibility_on_hand_states():
    states = np.stack([
        row2([1.5, 2.5], t=3.0),                      # at rest: eligible
        row2([1.5, 2.5], vel=[0.5, 0.0]),             # moving: another hash
        row2([1.5, 2.5], vel=[0.004, 0.0]),           # below the velocity lattice (0.1): same hash, but the position moves
        row2([1.5, 2.5], vel=[0.04, 0.0]),            # same velocity bin, the position leaves its cell of 0.01: another hash
        row2([1.5, 2.5], vel=[1e-20, 0.0]),           # so slow that pos + v T == pos: eligible (the position does not move)
    ], axis=1)
    L = lists_for(5, 9, [8, 9, 8, 8, 0])
    n, el = WM.add_wait(L, 5, states, None, 2, ACC, U9, 1.0, 10.0, v_max=1.0, a_max=1.0)
    assert el.tolist() == [True, False, False, False, True] and n == 2
    assert L["count"].tolist() == [9, 9, 8, 8, 1]
    e = 0 * 9 + 8
    assert L["action"][e] == 4 and L["cost"][e] == 10.0 and L["state"][:, e].tolist() == [1.5, 2.5, 0, 0, 0, 0, 0, 0, 0, 4.0]
    assert L["hash"][e] == WM.lattice_hash(2, ACC, states[:, 0])
    p = WM.pair_eval(2, ACC, states[:, 2], U9[4], 1.0)
    assert p["h_next"] == p["h_curr"] and not p["same_pos"] and p["next"][0] == 1.504
    # nothing else changed
    assert (L["action"] != -7).sum() == 2 and (L["cost"] != -1.0).sum() == 2 and (L["state"][0] != -3.0).sum() == 2
    # the row of the fifth state was empty: its wait is entry 0
    assert L["action"][4 * 9] == 4 and L["state"][4, 4 * 9] == 0.0  # acc row: +0.0
    # parent_id < 0 skips; a full list (count == S) takes no entry
    L = lists_for(2, 9, [3, 9])
    n, el = WM.add_wait(L, 2, states[:, [0, 0]], np.array([-1, 0]), 2, ACC, U9, 1.0, 10.0)
    assert n == 0 and el.all() and L["count"].tolist() == [3, 9] and (L["action"] == -7).all()


def test_a_limit_violated_is_no_wait():
    # JRK at rest but for an acceleration above a_max: the hash stays (u = 0 keeps acc), the limits say no.  v = 0, a = 0.04:
    # the position moves too; so take a state whose only fault is the limit: VEL-free case through v_max with ACC
    st = row2([1.0, 1.0], vel=[1e-20, 0.0]).reshape(-1, 1)
    L = lists_for(1, 9, [0])
    assert WM.add_wait(L, 1, st, None, 2, ACC, U9, 1.0, 10.0, v_max=1e-21)[0] == 0   # |v| > v_max
    assert WM.add_wait(L, 1, st, None, 2, ACC, U9, 1.0, 10.0, v_max=1e-19)[0] == 1
    # heading: the tiny velocity points along +x, the robot looks along +y, yaw_max = 0.5
    Uy = np.array([[x, y, r] for x in (-0.5, 0.0, 0.5) for y in (-0.5, 0.0, 0.5) for r in (-0.3, 0.0, 0.3)])
    sty = row2([1.0, 1.0], vel=[1e-20, 0.0], yaw=1.5).reshape(-1, 1)
    L = lists_for(1, 32, [0])
    assert WM.add_wait(L, 1, sty, None, 2, ACCxYAW, Uy, 1.0, 10.0, yaw_max=0.5)[0] == 0
    sty[8] = 0.1
    n, _ = WM.add_wait(L, 1, sty, None, 2, ACCxYAW, Uy, 1.0, 10.0, yaw_max=0.5)
    assert n == 1 and L["action"][0] == 13 and L["state"][8, 0] == 0.1


def test_a0_in_a_shuffled_table():
    rng = np.random.default_rng(3)
    for _ in range(20):
        perm = rng.permutation(9)
        U = U9[perm]
        assert WM.zero_action(U) == int(np.nonzero(perm == 4)[0][0])
    U = np.concatenate([U9[[0, 4, 8]], [[-0.0, 0.0]], U9[[4]]])
    assert WM.zero_action(U) == 1                       # the smallest
    assert WM.zero_action(U[[0, 3, 2]]) == 1            # -0.0 == 0.0
    assert WM.zero_action(U9[[0, 1, 2, 3, 5]]) == -1
    assert WM.zero_action(np.array([[0.0, 0.0, 0.3], [0.0, 0.0, 0.0]])) == 1  # the yaw rate counts
    with pytest.raises(ValueError):
        WM.add_wait(lists_for(1, 9, [0]), 1, row2([0, 0]).reshape(-1, 1), None, 2, ACC, U9[[0, 1]], 1.0, 10.0)


# ---------------------------------------------------------------------------------------------------- the park veto
def test_park_scan_finds_the_stated_set():
    rng = np.random.default_rng(11)
    n_checked = 0
    for _ in range(4000):
        step = float(rng.choice([0.25, 0.3, 0.1, 1.0 / 3.0, 0.7, 1.7]))
        n_steps = int(rng.integers(1, 200))
        t0 = float(rng.choice([0.0, 0.3, 2.0, 1e-9, 7.1]))
        kind = rng.integers(0, 4)
        if kind == 0:
            t_node = float(rng.integers(0, 60))
        elif kind == 1:
            t_node = float(rng.random() * 70 - 5)
        else:  # exactly on an instant, and one ulp either side
            i = int(rng.integers(0, n_steps + 3))
            on = np.float64(i) * np.float64(step) - np.float64(t0)
            t_node = float([on, np.nextafter(on, -np.inf), np.nextafter(on, np.inf)][int(rng.integers(0, 3))])
        want = WM.park_instants(step, n_steps, t0, t_node)
        first = WM.park_first_scan(step, n_steps, t0, t_node)
        assert first == (int(want[0]) if len(want) else n_steps), (step, n_steps, t0, t_node)
        assert len(want) == 0 or want.tolist() == list(range(first, n_steps))  # tl_i is monotone: the set is a tail
        n_checked += len(want) > 0
    assert n_checked > 1000
    for t_node in (np.nan, np.inf, 1e300):
        assert WM.park_first_scan(0.25, 100, 0.0, t_node) == 100 and len(WM.park_instants(0.25, 100, 0.0, t_node)) == 0
    assert WM.park_first_scan(0.25, 100, 0.0, -np.inf) == 0 and WM.park_first_scan(0.25, 100, 3.0, -1e300) == 0


def table(pos_fn, n_steps, step, B, D=2, active=None, radius=0.5, group=None, included=None):
    pos = np.zeros((n_steps, D, B))
    for i in range(n_steps):
        for b in range(B):
            pos[i, :, b] = pos_fn(b, np.float64(i) * np.float64(step))
    return {"pos": pos, "active": np.ones((n_steps, B), np.uint8) if active is None else np.asarray(active, np.uint8),
            "included": np.ones(B, np.uint8) if included is None else np.asarray(included, np.uint8),
            "radius": np.broadcast_to(np.float64(radius), (B,)).copy(),
            "group": np.arange(B, dtype=np.int32) if group is None else np.asarray(group, np.int32), "step": step}


def goal_rows(pts, ts):
    n = len(pts)
    st = np.zeros((10, n))
    st[:2] = np.asarray(pts, dtype=np.float64).T
    st[9] = ts
    return {"count": n, "id": np.arange(n, dtype=np.int32), "state": st}


def run_park(res, fr, t0=0.0, radius=0.5, ignore=-1, flags=None, n_max=None):
    n = fr["count"]
    fl = np.full(n, WM.SEEN | WM.IS_OPEN | WM.IS_GOAL, np.uint8) if flags is None else flags
    return WM.park(fl, n, fr, n if n_max is None else n_max, n, res, ([t0], [radius], [ignore]), 2)


def test_park_veto_and_touching():
    # b drives x = 10 - t along y = 0; nodes stand at x = 5: it comes within rr = 1 for t in (4, 6)
    res = table(lambda b, t: [10.0 - t, 0.0], 64, 0.25, 1)
    fr = goal_rows([[5, 0], [5, 0], [5, 0], [5, 1.0], [5, np.nextafter(1.0, 0)]], [0.0, 5.0, 6.0, 0.0, 0.0])
    fl, hit, nv = run_park(res, fr)
    # arriving before it or while it passes: vetoed at the first instant inside; at t = 6 it is touching, then gone
    assert hit.tolist() == [17 << 32, 20 << 32, -1, -1, 20 << 32] and nv == 3
    assert fl.tolist() == [5, 5, 7, 7, 5]  # only IS_GOAL goes
    # closed at t_node: a node AT an instant is tested at it
    fr = goal_rows([[5, 0]] * 3, [5.75, np.nextafter(5.75, 10), 5.5])
    assert run_park(res, fr)[1].tolist() == [23 << 32, -1, 22 << 32]
    # rows that are not looked at: no goal bit, id out of range, n_max
    fr = goal_rows([[5, 0]] * 4, [0.0] * 4)
    fr["id"] = np.array([0, 7, -1, 3], np.int32)
    fl, hit, nv = run_park(res, fr, flags=np.array([7, 7, 7, 5], np.uint8))
    assert hit.tolist() == [17 << 32, -1, -1, -1] and nv == 1 and fl.tolist() == [5, 7, 7, 5]
    fr["id"] = np.arange(4, dtype=np.int32)
    assert run_park(res, fr, n_max=2)[1].tolist() == [17 << 32, 17 << 32]
    # past the horizon (instants end at t = 15.75): no instants, no veto
    assert run_park(table(lambda b, t: [5.0, 0.0], 64, 0.25, 1), goal_rows([[5, 0]] * 2, [15.75, 16.0]))[1].tolist() == [63 << 32, -1]


def test_park_gone_park_and_groups():
    import conflict_model as cm
    # b stands at x = 5 from t0 = 2 on and its trajectory lasts 3 s
    tl = cm.local_times(0.25, 64, [2.0], 1)
    gone = table(lambda b, t: [5.0, 0.0], 64, 0.25, 1, active=cm.active_mask(tl, [3.0], cm.GONE))
    parked = table(lambda b, t: [5.0, 0.0], 64, 0.25, 1, active=cm.active_mask(tl, [3.0], cm.PARK))
    fr = goal_rows([[5, 0]] * 4, [0.0, 2.0, 5.0, 5.25])
    assert run_park(gone, fr)[1].tolist() == [8 << 32, 8 << 32, 20 << 32, -1]        # GONE: nothing after its end
    assert run_park(parked, fr)[1].tolist() == [0, 8 << 32, 20 << 32, 21 << 32]      # PARK: always there
    # groups and exclusion
    res = table(lambda b, t: [5.0, 0.0], 8, 0.25, 3, group=[7, 7, 9], included=[1, 0, 1])
    one = goal_rows([[5, 0]], [0.0])
    assert run_park(res, one)[1].tolist() == [0]
    assert run_park(res, one, ignore=7)[1].tolist() == [2]
    res["included"][2] = 0
    fl, hit, nv = run_park(res, one, ignore=7)
    assert hit.tolist() == [-1] and nv == 0 and fl.tolist() == [7]
    # the query's own clock: t0 = 1 shifts the instants
    assert run_park(gone, goal_rows([[5, 0]], [3.0]), t0=1.0)[1].tolist() == [16 << 32]  # tl_16 = 4 - 1 = 3
    assert run_park(gone, goal_rows([[5, 0]], [4.25]), t0=1.0)[1].tolist() == [-1]


# ---------------------------------------------------------------------------------------------------- the header
def test_every_function_of_the_header_is_declared_in_abi(engine):
    text = open(os.path.join(ROOT, "include", "mplx_wait.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(mplx_[a-z0-9_]+)\s*\(", text)))
    assert syms == ["mplx_lists_add_wait_device"] == sorted(engine._abi.WAIT_SYMBOLS)
    assert "mplx_reserve_park_device" in engine._abi.RESERVE_SYMBOLS
    lib = engine._abi.lib()
    for s in syms + ["mplx_reserve_park_device"]:
        assert getattr(lib, s).argtypes is not None, s


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_wait.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------------- the scenarios
STEP, R = 0.25, 0.3
LIMITS = (1.0, 1.0, 0.0, 0.0)  # v_max, a_max, j_max, yaw_max


def plan(O, grid, dims, start, goal, res, wait, park_goal, n_steps):
    oenv = O.Env(2, O.ACC, U9, grid, dims, [0.0, 0.0], 1.0, v_max=1.0, a_max=1.0, dt=1.0)
    s, g = row2(start), row2(goal)
    out, tab, opn = WM.search_many(oracle_provider(O, oenv), 2, ACC, U9, 1.0, 10.0, LIMITS, s.reshape(-1, 1), [O.lattice_hash(2, O.ACC, s)],
                                   g.reshape(1, -1), [O.lattice_hash(2, O.ACC, g)], res, ([0.0], [R], [-1]), n_steps, wait, park_goal,
                                   max_rounds=400)
    r = out["results"][0]
    if out["status"][0] != WM.MM.FOUND:
        return out["status"][0], np.inf, None, opn
    ids, acts = WM.path_of(tab, r["goal_id"])
    return out["status"][0], r["goal_g"], acts, opn


def empty_table(n_steps):
    return {"pos": np.zeros((n_steps, 2, 0)), "active": np.zeros((n_steps, 0), np.uint8), "included": np.zeros(0, np.uint8),
            "radius": np.zeros(0), "group": np.zeros(0, np.int32), "step": STEP}


def charged(U, paths, starts, n_steps):
    """Whether robot 1 comes within 2 R of robot 0 at any instant (both parked after their ends)."""
    H = max(len(p) for p in paths)
    ac = np.full((H, 2), -1, np.int64)
    for b, p in enumerate(paths):
        ac[:len(p), b] = p
    t = WM.chain_table(2, ACC, U, 1.0, np.stack([row2(s) for s in starts], axis=1), ac, STEP, n_steps, 0.0, R)
    d = np.linalg.norm(t["pos"][:, :, 0] - t["pos"][:, :, 1], axis=1)
    return bool((d < 2 * R).any()), float(d.min())


def test_scenario_parking_on_the_models(oracle_lib):
    """A crossing of two one-cell lanes on a 13 x 13 map.  Robot 0 drives west to east through it; robot 1 starts 4 m south
    of the crossing and its goal is the crossing cell.  Recorded from the models: robot 0 alone costs 110.5 over 11
    primitives and is at the crossing at t = 6; robot 1 with today's arguments arrives there at t = 5 (5 primitives, 50.5)
    and stands in its way; with wait and park_goal its arrivals up to t = 5 are vetoed (26 vetoes) and it arrives at
    t = 6 for 61.0, by a slower profile that ends in the corner of the goal region 0.71 m from robot 0 -- cheaper than two
    waits (70.5); one wait (60.5) would end where robot 0 is.  Nobody comes within 2 R."""
    O = oracle_lib
    n = 13
    grid = np.full((n, n), 100, np.int8)
    grid[6, :] = 0
    grid[:, 6] = 0
    n_steps = int(40 / STEP)
    s0, g0, s1, g1 = [1.5, 6.5], [11.5, 6.5], [6.5, 2.5], [6.5, 6.5]
    st0, c0, p0, _ = plan(O, grid.ravel(), [n, n], s0, g0, empty_table(n_steps), False, False, n_steps)
    assert st0 == WM.MM.FOUND
    res = WM.chain_table(2, ACC, U9, 1.0, row2(s0).reshape(-1, 1), np.array(p0).reshape(-1, 1), STEP, n_steps, 0.0, R)
    st, c_old, p_old, _ = plan(O, grid.ravel(), [n, n], s1, g1, res, False, False, n_steps)
    st2, c_new, p_new, opn = plan(O, grid.ravel(), [n, n], s1, g1, res, True, True, n_steps)
    print("robot 0:", c0, p0, "| robot 1 today:", c_old, p_old, "| wait + park:", c_new, p_new, "vetoed", opn.n_vetoed)
    assert st == WM.MM.FOUND and charged(U9, [p0, p_old], [s0, s1], n_steps)[0]          # the gap
    assert st2 == WM.MM.FOUND and not charged(U9, [p0, p_new], [s0, s1], n_steps)[0]
    assert 4 in p_new and len(p_new) > len(p_old) and opn.n_vetoed > 0
    assert (c0, len(p0), c_old, len(p_old), c_new, len(p_new), p_new.count(4)) == (110.5, 11, 50.5, 5, 61.0, 6, 3)


def test_scenario_waiting_mid_path_on_the_models(oracle_lib):
    """One east-west lane with a side pocket two cells deep.  Robot 1 starts at rest on the lane below the pocket, in robot
    0's way, and its goal is further along the lane.  It has to leave the lane, let robot 0 pass and go on.  Recorded
    from the models: robot 0 alone 150.5 (15 primitives); robot 1 with wait and park_goal 141.5 (14 primitives: six waits
    on the lane, then into the pocket and out); with park_goal alone 142.0 (14 primitives: it fills the time by moving)."""
    O = oracle_lib
    grid = np.full((7, 17), 100, np.int8)  # [y][x]
    grid[3, :] = 0
    grid[4:6, 9] = 0
    n_steps = int(60 / STEP)
    s0, g0, s1, g1 = [1.5, 3.5], [15.5, 3.5], [9.5, 3.5], [13.5, 3.5]
    st0, c0, p0, _ = plan(O, grid.ravel(), [17, 7], s0, g0, empty_table(n_steps), False, False, n_steps)
    assert st0 == WM.MM.FOUND
    res = WM.chain_table(2, ACC, U9, 1.0, row2(s0).reshape(-1, 1), np.array(p0).reshape(-1, 1), STEP, n_steps, 0.0, R)
    st_w, c_w, p_w, _ = plan(O, grid.ravel(), [17, 7], s1, g1, res, True, True, n_steps)
    st_n, c_n, p_n, _ = plan(O, grid.ravel(), [17, 7], s1, g1, res, False, True, n_steps)
    print("robot 0:", c0, p0, "| wait + park:", c_w, p_w, "| park only:", st_n, c_n, p_n)
    assert st_w == WM.MM.FOUND and not charged(U9, [p0, p_w], [s0, s1], n_steps)[0] and 4 in p_w
    assert st_n != WM.MM.FOUND or (c_w < c_n and not charged(U9, [p0, p_n], [s0, s1], n_steps)[0])
    assert (c0, len(p0)) == (150.5, 15) and (c_w, len(p_w), p_w[:6]) == (141.5, 14, [4] * 6) and (st_n, c_n, len(p_n)) == (WM.MM.FOUND, 142.0, 14)
