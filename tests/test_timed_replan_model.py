"""Hand cases for tests/timed_replan_model.py, the sequential restatement of include/mplx_replan_timed.h, and the timed
replan of the pocket lane of tests/test_wait_model.py on the models.  No GPU: the device side is held against the same
model in tests/test_gpu_timed_replan.py."""
import copy
import math
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_model as MM  # noqa: E402
import replan_model as RP  # noqa: E402
import reserve_model as RM  # noqa: E402
import timed_replan_model as TR  # noqa: E402
import wait_model as WM  # noqa: E402
from prior_model import lattice_hash  # noqa: E402
from table_model import oracle_provider  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACC = 0x03
U9 = np.array([[x, y] for x in (-0.5, 0.0, 0.5) for y in (-0.5, 0.0, 0.5)])
A0, EAST, WEST, NORTH, SOUTH, NE = 4, 7, 1, 5, 3, 8
LIMITS = (1.0, 1.0, 0.0, 0.0)
CFG = TR.Config(2, ACC, U9, 1.0, 10.0, LIMITS)
STEP = 0.25


def row2(pos, vel=(0, 0), t=0.0):
    return np.array(list(pos) + list(vel) + [0, 0, 0, 0] + [0.0, t], dtype=np.float64)


class PairEdge:
    """edge(p, a) on an all-free map without a potential: the pair's own status, hash and cost; `blocked`: (p, a) pairs
    the map blocks."""

    def __init__(self, table, cfg, blocked=()):
        self.table, self.cfg, self.blocked = table, cfg, set(blocked)

    def __call__(self, p, a):
        c = self.cfg
        pe = WM.pair_eval(c.dim, c.control, self.table.state[p], c.U[a], c.dt, *c.limits)
        if pe["h_next"] == pe["h_curr"]:
            return 0, pe["h_next"], math.inf
        if not pe["valid"]:
            return 3, pe["h_next"], math.inf
        if (p, a) in self.blocked:
            return 2, pe["h_next"], math.inf
        return 1, pe["h_next"], 0.0 + (pe["J"] + c.w * c.dt)


class Builder:
    """A consistent time-keyed table of two queries, grown edge by edge."""

    def __init__(self):
        self.t = MM.MultiTableModel(10, 2)
        self.name = {}

    def raw(self, name, q, state, g, pred=-1, action=-1, key=None):
        t = self.t
        state = np.array(state, dtype=np.float64)
        key = RM.time_key(lattice_hash(2, ACC, state), float(state[-1])) if key is None else key
        i = t.n_nodes
        t.hash.append(int(key)); t.g.append(float(g)); t.pred.append(pred); t.pred_action.append(action)
        t.state.append(state); t.query.append(q)
        t.ids[(q, int(key))] = i
        self.name[name] = i
        return i

    def child(self, name, parent, a, dg=0.0):
        t, p = self.t, self.name[parent]
        pe = WM.pair_eval(2, ACC, t.state[p], U9[a], 1.0, *LIMITS)
        cost = 0.0 + (pe["J"] + 10.0 * 1.0)
        return self.raw(name, t.query[p], pe["next"], t.g[p] + cost + dg, p, a, RM.time_key(pe["h_next"], pe["next"][-1]))


def hand_table():
    b = Builder()
    b.raw("R", 0, row2([1.5, 3.5]), 0.0)
    b.child("E1", "R", EAST)            # x 1.75, v 0.5, t 1
    for k in range(2, 8):
        b.child("E%d" % k, "E%d" % (k - 1), A0)   # coasting east (no wait: the hash changes): x 2.25 .. 4.75, t 2 .. 7
    b.raw("S", 0, row2([9.5, 9.5]), 3.0)           # a node without a predecessor that is no root
    b.child("BLK", "R", NORTH)          # the map blocks this edge now
    b.child("LOW", "R", SOUTH, dg=-1.0)  # a g below what the edge gives
    b.child("STALE", "R", WEST, dg=5.0)  # a stale child: kept
    b.child("K1", "R", NE)
    b.child("K2", "K1", A0)
    b.child("W1", "R", A0)              # a wait at the root
    b.child("W2", "W1", A0)
    c1 = b.raw("C1", 0, row2([20.5, 20.5], t=3.0), 7.0, pred=-5, action=EAST)
    c2 = b.raw("C2", 0, row2([20.5, 21.5], t=4.0), 8.0, pred=c1, action=EAST)
    b.t.pred[c1] = c2                   # a cycle of predecessors
    b.raw("R1", 1, row2([5.5, 1.5], vel=[0.004, 0.0]), 0.0)
    b.child("X", "R1", A0)              # below the velocity lattice: the hash stays, the position moves
    b.child("Y", "R1", EAST)
    b.t.state[b.name["K1"]][-1] = 1.5   # K1's t altered: the key of its child no longer matches
    return b


def reservations(n_steps=29):
    """b0 stands at (3.0, 3.5) in the way of the east chain; b1 (group 5) at (5.65, 1.5) on the edge R1 -> Y."""
    pos = np.zeros((n_steps, 2, 2))
    pos[:, :, 0] = [3.0, 3.5]
    pos[:, :, 1] = [5.65, 1.5]
    return {"pos": pos, "active": np.ones((n_steps, 2), np.uint8), "included": np.ones(2, np.uint8), "radius": np.array([0.25, 0.25]),
            "group": np.array([0, 5], np.int32), "step": STEP}


def run(b, check_edges=True, allow_wait=True, res=None, ignore=(-1, 5), n_steps=29, capacity=None):
    t = copy.deepcopy(b.t)
    edge = PairEdge(t, CFG, blocked=[(b.name["R"], NORTH)])
    q = ([0.0, 0.5], [0.25, 0.25], list(ignore))
    fr, info, hit, nb, st = TR.rebase_timed(t, edge, CFG, [b.name["R"], b.name["R1"]], check_edges, allow_wait, True, res, q, n_steps,
                                            capacity)
    return t, fr, info, hit, nb, st


def test_every_class_of_node_on_a_hand_table():
    b = hand_table()
    N = b.name
    ids = lambda *names: sorted(N[x] for x in names)
    # ---- edges only
    t, fr, info, hit, nb, st = run(b)
    east = ["E%d" % k for k in range(1, 8)]
    assert fr["id"].tolist() == ids("R", "R1", "STALE", "K1", "W1", "W2", "Y", *east) and st == 0
    assert info == {"n_kept": 14, "n_roots": 2, "n_bad_edges": 6}  # BLK, LOW, K2, X, C1, C2
    assert hit is None and nb == 0
    for x in ("BLK", "LOW", "K2", "X", "S", "C1", "C2"):
        assert t.g[N[x]] == math.inf and t.pred[N[x]] == t.pred_action[N[x]] == -1, x
    assert t.g[N["STALE"]] == b.t.g[N["STALE"]] == 15.25 and t.pred[N["STALE"]] == N["R"]
    assert t.g[N["W2"]] == 20.0 and t.pred_action[N["W2"]] == A0 and t.state[N["W2"]][-1] == 2.0
    assert t.pred[N["R"]] == t.pred[N["R1"]] == -1
    assert fr["g"].tolist() == [t.g[i] for i in fr["id"]] and np.array_equal(fr["state"][:, 1], t.state[fr["id"][1]])
    # t, the hash column and the queries' nodes are untouched
    assert t.hash == b.t.hash and all(np.array_equal(x, y) for x, y in zip(t.state, b.t.state)) and t.query == b.t.query
    # the reason K2 is bad is its key alone: with K1's t back it holds
    t2 = copy.deepcopy(b.t)
    t2.state[N["K1"]][-1] = 1.0
    e2 = PairEdge(t2, CFG)
    assert TR.edge_is_bad(copy.deepcopy(b.t), N["K2"], PairEdge(b.t, CFG), CFG, True, True) and not TR.edge_is_bad(t2, N["K2"], e2, CFG, True, True)
    # ... and without time keys the stored key is not the lattice hash: every edge is bad
    assert TR.edge_is_bad(t2, N["E1"], e2, CFG, False, True)
    # X: the same hash, a valid pair, but the position moves
    pe = WM.pair_eval(2, ACC, b.t.state[N["R1"]], U9[A0], 1.0, *LIMITS)
    assert pe["h_next"] == pe["h_curr"] and pe["valid"] and not pe["same_pos"]
    # ---- allow_wait = 0: the waits at the root go, with what hangs below them
    t, fr, info, *_ = run(b, allow_wait=False)
    assert fr["id"].tolist() == ids("R", "R1", "STALE", "K1", "Y", *east) and info["n_bad_edges"] == 8
    # ---- check_edges = 0: every edge holds; the seed that is no root and the cycle are dropped all the same
    t, fr, info, *_ = run(b, check_edges=False)
    assert info == {"n_kept": len(b.t.hash) - 3, "n_roots": 2, "n_bad_edges": 0}
    assert not set(fr["id"].tolist()) & set(ids("S", "C1", "C2"))
    # ---- a frontier one row too small
    t, fr, info, hit, nb, st = run(b, capacity=13)
    assert st == TR.FRONTIER_FULL and fr["count"] == 13 and info["n_kept"] == 14


def test_reservations_on_the_hand_table():
    b = hand_table()
    N = b.name
    res = reservations()
    t, fr, info, hit, nb, st = run(b, res=res)
    # the east chain: E3's edge (x 2.25 -> 2.75 during t 2 .. 3) touches at s = 0.5 (no hit: strict) and is inside at
    # s = 0.75 = instant 11; E4's and E5's edges are inside at their first instant; E6's and E7's are clear, E8 does not exist
    want = {"E3": 11 << 32, "E4": 12 << 32, "E5": 16 << 32}
    for x, i in N.items():
        assert hit[i] == want.get(x, -1), (x, hit[i])
    assert nb == 3
    # the whole chain under the blocked edge goes, E6 and E7 with it though their own edges are clear
    assert all(t.g[N["E%d" % k]] == math.inf for k in range(3, 8)) and t.g[N["E2"]] == b.t.g[N["E2"]]
    assert info["n_bad_edges"] == 6 + 3 and info["n_kept"] == 14 - 5
    # roots, nodes without a predecessor and the cycle's out-of-range predecessor are never looked at
    assert hit[N["R"]] == hit[N["S"]] == hit[N["C1"]] == -1
    # the horizon: 25 instants end at t = 6.0; E7's edge lasts to t = 7 (query 0: t0 = 0); E6's ends at 6.0 and stays
    t, fr, info, hit, nb, st = run(b, res=reservations(25), n_steps=25)
    assert hit[N["E7"]] == -2 and hit[N["E6"]] == -1 and hit[N["E3"]] == 11 << 32 and nb == 4
    # query 1 runs on its own clock (t0 = 0.5): its edges end at table time 1.5
    t, fr, info, hit, nb, st = run(b, res=reservations(7), n_steps=7)   # instants to 1.5
    assert hit[N["Y"]] == -1 and hit[N["X"]] == -1 and hit[N["E2"]] == -2 and hit[N["E1"]] == -1
    t, fr, info, hit, nb, st = run(b, res=reservations(6), n_steps=6)   # instants to 1.25
    assert hit[N["Y"]] == -2 and hit[N["X"]] == -2
    # the ignored group: b1 stands on the edge R1 -> Y; query 1 ignores group 5, or does not
    t, fr, info, hit, nb, st = run(b, res=res, ignore=(-1, -1))
    assert hit[N["Y"]] == (2 << 32) | 1 and hit[N["X"]] == (2 << 32) | 1 and t.g[N["Y"]] == math.inf and nb == 5
    # with check_edges = 0 the reservations alone decide
    t, fr, info, hit, nb, st = run(b, check_edges=False, res=res)
    assert info["n_bad_edges"] == 3 and nb == 3 and t.g[N["K2"]] == b.t.g[N["K2"]] and t.g[N["E7"]] == math.inf
    # excluded and inactive reservations block nothing
    off = reservations()
    off["included"][0] = 0
    assert run(b, res=off)[4] == 0
    off = reservations()
    off["active"][:, 0] = 0
    assert run(b, res=off)[4] == 0


def test_instants_of_an_edge_are_the_stated_set():
    rng = np.random.default_rng(5)
    n_some = 0
    for _ in range(4000):
        step = float(rng.choice([0.25, 0.3, 0.1, 1.0 / 3.0, 0.7]))
        n_steps = int(rng.integers(1, 200))
        t0 = float(rng.choice([0.0, 0.5, 2.0, 0.3, 7.1]))
        tp = float(rng.integers(0, 40)) if rng.integers(0, 2) else float(rng.random() * 40)
        tc = np.float64(tp) + np.float64(1.0)
        want = RM.instants(step, n_steps, t0, tp, tc)
        got = RM.instants_scan(step, n_steps, t0, tp, tc, 1.0)
        assert want.tolist() == got.tolist(), (step, n_steps, t0, tp)
        n_some += len(want) > 0
    assert n_some > 1000
    # ... and the per-node test of the new model looks at exactly the instants the kernel's scan finds: a wait edge at the
    # root against one reservation that stands on it and is active at ONE instant i is hit iff i is in the scan's set
    n_hit = n_horizon = 0
    for _ in range(600):
        step = float(rng.choice([0.25, 0.3, 1.0 / 3.0, 0.7]))
        n_steps = int(rng.integers(1, 120))
        t0 = float(rng.choice([0.0, 0.5, 0.3, 7.1]))
        tp = float(rng.integers(0, 30)) if rng.integers(0, 2) else float(rng.random() * 30)
        t = MM.MultiTableModel(10, 1)
        t.hash, t.g, t.pred, t.pred_action, t.query = [1, 2], [0.0, 10.0], [-1, 0], [-1, A0], [0, 0]
        t.state = [row2([1.5, 3.5], t=tp), row2([1.5, 3.5], t=tp + 1.0)]
        scan = RM.instants_scan(step, n_steps, t0, tp, np.float64(tp) + np.float64(1.0), 1.0).tolist()
        i = int(rng.integers(0, n_steps))
        if scan and rng.integers(0, 2):
            i = int(rng.choice(scan))
        res = {"pos": np.tile(np.array([1.5, 3.5]).reshape(1, 2, 1), (n_steps, 1, 1)), "active": np.zeros((n_steps, 1), np.uint8),
               "included": np.ones(1, np.uint8), "radius": np.array([0.25]), "group": np.zeros(1, np.int32), "step": step}
        res["active"][i, 0] = 1
        hit = TR.reserve_hits(t, [True, False], CFG, res, ([t0], [0.25], [-1]), n_steps)
        off = RM.leaves_horizon(step, n_steps, t0, np.float64(tp) + np.float64(1.0))
        assert hit.tolist() == [-1, -2 if off else (i << 32 if i in scan else -1)], (step, n_steps, t0, tp, i)
        n_hit += hit[1] >= 0
        n_horizon += off
    assert n_hit > 50 and n_horizon > 50
    # step = 0.3 against dt = 1: three or four instants per edge, never a fixed count
    assert {len(RM.instants(0.3, 100, 0.0, float(k), float(k) + 1.0)) for k in range(12)} == {3, 4}


# ---------------------------------------------------------------------------------------------------- the header
def test_every_function_of_the_header_is_declared_in_abi(engine):
    text = open(os.path.join(ROOT, "include", "mplx_replan_timed.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(mplx_[a-z0-9_]+)\s*\(", text)))
    assert syms == ["mplx_table_rebase_timed_device"] == sorted(engine._abi.REPLAN_TIMED_SYMBOLS)
    assert not set(syms) & set(engine._abi.SYMBOLS)
    assert getattr(engine._abi.lib(), syms[0]).argtypes is not None


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_replan_timed.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------------- the scenario
R_ROBOT = 0.3
# recorded from the models: k -> cost of the timed replan after robot 0 was delayed by DELAY (equal to the fresh search's)
DELAY, DELAY2 = 2.5, 4.0
# ... and (n_kept, n_bad_edges, n_blocked, the actions of full_path); "5+3": the second replan on the table of k = 5
_LATE = [4, 4, 4, 4, 4, 4, 4, 5, 4, 3, 4, 6, 4, 7, 5, 4]
POCKET_RECORD = {0: (4886, 13, 13, _LATE), 2: (1703, 13, 13, _LATE), 5: (502, 13, 13, _LATE),
                 "5+3": (157, 87, 87, [4, 4, 4, 4, 4, 4, 4, 5, 4, 3, 4, 4, 4, 6, 7, 5, 4, 4]),
                 8: (79, 13, 13, [4, 4, 4, 4, 4, 4, 5, 4, 4, 3, 3, 7, 4, 7, 5, 4])}
POCKET_COSTS = {0: 161.5, 2: 161.5, 5: 161.5, "5+3": 181.5, 8: 161.5}  # 141.5 and two more waits (20.0) for the 2.5 s; then two more


def pocket():
    grid = np.full((7, 17), 100, np.int8)  # [y][x]
    grid[3, :] = 0
    grid[4:6, 9] = 0
    return grid, [17, 7]


def chains_clear(paths, starts, t0, n_steps):
    H = max(len(p) for p in paths)
    ac = np.full((H, 2), -1, np.int64)
    for k, p in enumerate(paths):
        ac[:len(p), k] = p
    t = WM.chain_table(2, ACC, U9, 1.0, np.stack(starts, axis=1), ac, STEP, n_steps, t0, R_ROBOT)
    d = np.linalg.norm(t["pos"][:, :, 0] - t["pos"][:, :, 1], axis=1)
    return not bool((d < 2 * R_ROBOT).any())


def test_scenario_pocket_lane_timed_replan(oracle_lib):
    """The pocket lane of tests/test_wait_model.py at delta = 0.  Robot 1 is planned among robot 0 with waits and the park
    veto, advances k primitives, robot 0 is delayed by 2.5 s and robot 1 replans on its table.  The cost must be that of a
    fresh search from the root state (t = 0, t0 + t_root, start_g = g_root), and the two full chains must keep clear."""
    O = oracle_lib
    grid, dims = pocket()
    oenv = O.Env(2, O.ACC, U9, grid.ravel(), dims, [0.0, 0.0], 1.0, v_max=1.0, a_max=1.0, dt=1.0)
    provider = oracle_provider(O, oenv)
    n_steps = int(60 / STEP)
    s0, g0, s1, g1 = row2([1.5, 3.5]), row2([15.5, 3.5]), row2([9.5, 3.5]), row2([13.5, 3.5])
    none = {"pos": np.zeros((n_steps, 2, 0)), "active": np.zeros((n_steps, 0), np.uint8), "included": np.zeros(0, np.uint8),
            "radius": np.zeros(0), "group": np.zeros(0, np.int32), "step": STEP}
    q1 = ([0.0], [R_ROBOT], [-1])
    out0, tab0, _ = TR.fresh(provider, CFG, s0.reshape(-1, 1), [lattice_hash(2, ACC, s0)], 0.0, g0.reshape(1, -1), none, q1, n_steps,
                             False, False)
    assert out0["status"] == [MM.FOUND]
    p0 = WM.path_of(tab0, out0["results"][0]["goal_id"])[1]
    res_of = lambda t0: WM.chain_table(2, ACC, U9, 1.0, s0.reshape(-1, 1), np.array(p0).reshape(-1, 1), STEP, n_steps, t0, R_ROBOT)
    res = res_of(0.0)
    out1, tab1, opn1 = TR.fresh(provider, CFG, s1.reshape(-1, 1), [lattice_hash(2, ACC, s1)], 0.0, g1.reshape(1, -1), res, q1, n_steps,
                                True, True)
    assert out1["status"] == [MM.FOUND]
    cost1 = out1["results"][0]["goal_g"]
    ids1, p1 = WM.path_of(tab1, out1["results"][0]["goal_id"])
    print("robot 0:", out0["results"][0]["goal_g"], p0, "| robot 1:", cost1, p1)
    assert (out0["results"][0]["goal_g"], len(p0), cost1, len(p1)) == (150.5, 15, 141.5, 14)

    # ---- nothing changed: every edge holds, nothing is blocked, the cost stays
    for k in (0, 3):
        tab, opn = copy.deepcopy((tab1, opn1))
        out = TR.replan_timed(tab, opn, provider, RP.OracleEdges(O, oenv, tab), CFG, [ids1[k]], res, q1, n_steps, True, True)
        assert out["status"] == [MM.FOUND] and out["results"][0]["goal_g"] == cost1
        assert out["info"]["n_bad_edges"] == 0 and out["n_blocked"] == 0 and out["info"]["n_roots"] == 1
        assert TR.full_path(tab, out, 0)[1] == p1

    # ---- robot 0 is delayed
    res2 = res_of(DELAY)
    costs, record = {}, {}
    for k in (0, 2, 5, 8):
        tab, opn = copy.deepcopy((tab1, opn1))
        root = ids1[k]
        t_root, g_root = float(tab.state[root][-1]), tab.g[root]
        assert t_root == float(k)
        out = TR.replan_timed(tab, opn, provider, RP.OracleEdges(O, oenv, tab), CFG, [root], res2, q1, n_steps, True, True)
        start = np.array(tab1.state[root])
        start[-1] = 0.0
        fr, ftab, _ = TR.fresh(provider, CFG, start.reshape(-1, 1), [lattice_hash(2, ACC, start)], g_root, g1.reshape(1, -1), res2,
                               ([0.0 + t_root], [R_ROBOT], [-1]), n_steps, True, True)
        print("k = %d: replan %s %r (kept %d, bad %d, blocked %d, rounds %d) | fresh %s %r (rounds %d)" % (
            k, out["status"], out["results"][0]["goal_g"], out["info"]["n_kept"], out["info"]["n_bad_edges"], out["n_blocked"],
            out["total_rounds"], fr["status"], fr["results"][0]["goal_g"], fr["total_rounds"]))
        assert out["status"] == fr["status"] == [MM.FOUND]
        assert out["results"][0]["goal_g"] == fr["results"][0]["goal_g"]
        start_full, acts = TR.full_path(tab, out, 0)
        assert np.array_equal(start_full, s1) and acts[:k] == p1[:k] and len(out["executed"][0][1]) == k
        assert chains_clear([p0, acts], [s0, s1], [DELAY, 0.0], n_steps)
        costs[k] = out["results"][0]["goal_g"]
        record[k] = (out["info"]["n_kept"], out["info"]["n_bad_edges"], out["n_blocked"], acts)
        if k == 5:  # a second replan on the same table: robot 0 is delayed once more, robot 1 has made three more primitives
            res3 = res_of(DELAY2)
            ids2 = WM.path_of(tab, out["results"][0]["goal_id"])[0]
            out2 = TR.replan_timed(tab, opn, provider, RP.OracleEdges(O, oenv, tab), CFG, [ids2[3]], res3, q1, n_steps, True, True,
                                   executed=out["executed"])
            start2 = np.array(tab.state[ids2[3]])
            g2, t2 = tab.g[ids2[3]], float(start2[-1])
            start2[-1] = 0.0
            fr2, _, _ = TR.fresh(provider, CFG, start2.reshape(-1, 1), [lattice_hash(2, ACC, start2)], g2, g1.reshape(1, -1), res3,
                                 ([t2], [R_ROBOT], [-1]), n_steps, True, True)
            s2, acts2 = TR.full_path(tab, out2, 0)
            assert t2 == 8.0 and out2["status"] == fr2["status"] == [MM.FOUND]
            assert out2["results"][0]["goal_g"] == fr2["results"][0]["goal_g"]
            assert np.array_equal(s2, s1) and acts2[:8] == acts[:8] and len(out2["executed"][0][1]) == 8
            assert chains_clear([p0, acts2], [s0, s1], [DELAY2, 0.0], n_steps)
            record["5+3"] = (out2["info"]["n_kept"], out2["info"]["n_bad_edges"], out2["n_blocked"], acts2)
            costs["5+3"] = out2["results"][0]["goal_g"]
    print("costs", costs)
    print("record", record)
    assert costs == POCKET_COSTS
    assert record == POCKET_RECORD


# recorded from the models: the crossing of tests/test_gpu_wait.py with three delay candidates (see the test below)
CROSSING_DELAYS = [0.0, 2.0, 4.0]
CROSSING_K = 3
CROSSING_RECORD = {"first_costs": [181.0, 161.0, 141.0], "winner": 0, "status": [1, 2, 2], "cost": 151.0, "n_kept": 3585,
                   "n_bad_edges": 3154, "n_roots": 1, "n_blocked": 3154, "actions": [4, 4, 4, 4, 4, 4, 4, 4, 5, 4, 4, 4, 4, 1, 8]}


def test_scenario_crossing_timed_replan(oracle_lib):
    """The 33 x 33 crossing.  Robot 1 is planned as three delay candidates among a robot 0 that starts 2.5 s late; robot 0
    then starts on time after all and the winning candidate replans after 3 primitives, the losers with roots out of
    range.  tests/test_gpu_timed_replan.py pins what is recorded here on the device."""
    O = oracle_lib
    n = 33
    grid = np.full((n, n), 100, np.int8)
    grid[16, :] = 0
    grid[:, 16] = 0
    oenv = O.Env(2, O.ACC, U9, grid.ravel(), [n, n], [0.0, 0.0], 1.0, v_max=1.0, a_max=1.0, dt=1.0)
    provider = oracle_provider(O, oenv)
    n_steps = int(120 / STEP)
    s0, g0, s1, g1 = row2([2.5, 16.5]), row2([30.5, 16.5]), row2([16.5, 12.5]), row2([16.5, 16.5])
    none = {"pos": np.zeros((n_steps, 2, 0)), "active": np.zeros((n_steps, 0), np.uint8), "included": np.zeros(0, np.uint8),
            "radius": np.zeros(0), "group": np.zeros(0, np.int32), "step": STEP}
    out0, tab0, _ = TR.fresh(provider, CFG, s0.reshape(-1, 1), [lattice_hash(2, ACC, s0)], 0.0, g0.reshape(1, -1), none,
                             ([0.0], [R_ROBOT], [-1]), n_steps, False, False)
    p0 = WM.path_of(tab0, out0["results"][0]["goal_id"])[1]
    assert (out0["results"][0]["goal_g"], len(p0)) == (290.5, 29)
    res_of = lambda t0: WM.chain_table(2, ACC, U9, 1.0, s0.reshape(-1, 1), np.array(p0).reshape(-1, 1), STEP, n_steps, t0, R_ROBOT)
    q3 = (CROSSING_DELAYS, [R_ROBOT] * 3, [-1] * 3)
    out1, tab, opn = TR.fresh(provider, CFG, np.repeat(s1.reshape(-1, 1), 3, axis=1), [lattice_hash(2, ACC, s1)] * 3, 0.0,
                              np.repeat(g1.reshape(1, -1), 3, axis=0), res_of(DELAY), q3, n_steps, True, True)
    assert out1["status"] == [MM.FOUND] * 3
    chains = [WM.path_of(tab, r["goal_id"]) for r in out1["results"]]
    win = int(np.argmin([CROSSING_DELAYS[q] + len(chains[q][1]) for q in range(3)]))
    roots = [1 << 17] * 3
    roots[win] = chains[win][0][CROSSING_K]
    out = TR.replan_timed(tab, opn, provider, RP.OracleEdges(O, oenv, tab), CFG, roots, res_of(0.0), q3, n_steps, True, True)
    acts = TR.full_path(tab, out, win)[1]
    record = {"first_costs": [r["goal_g"] for r in out1["results"]], "winner": win, "status": out["status"],
              "cost": out["results"][win]["goal_g"], "n_kept": out["info"]["n_kept"], "n_bad_edges": out["info"]["n_bad_edges"],
              "n_roots": out["info"]["n_roots"], "n_blocked": out["n_blocked"], "actions": acts}
    print("crossing record", record)
    assert out["status"][win] == MM.FOUND and [out["status"][q] for q in range(3) if q != win] == [MM.EMPTY] * 2
    assert out["n_blocked"] > 0 and acts[:CROSSING_K] == chains[win][1][:CROSSING_K]
    assert chains_clear([p0, acts], [s0, s1], [0.0, CROSSING_DELAYS[win]], n_steps)
    assert record == CROSSING_RECORD
