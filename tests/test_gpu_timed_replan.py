"""The timed rebase (include/mplx_replan_timed.h, replan_kernel.hip), SearchResult.replan_timed / full_path and the fleet
layer (search.plan_prioritised(keep=True), search.replan_prioritised) on the device, against
tests/timed_replan_model.py, a fresh search from the root state and conflicts().  The model is fed with the device's
own table and reservation table (downloads), so what is compared is the rebase alone; its ordinary edges come from the
CPU oracle on the edited map."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import control_matrix as CM
import replan_model as RP
import timed_replan_model as TR
from test_gpu_open import assert_spare_untouched, patterned_frontier
from test_gpu_replan import assert_rebased_equal, cell_index, depths, restore
from test_gpu_table import assert_frontier_equal, bits
from test_timed_replan_model import CROSSING_DELAYS, CROSSING_K, CROSSING_RECORD, DELAY, DELAY2, POCKET_COSTS, POCKET_RECORD

pytestmark = pytest.mark.gpu

POISON = 0xAB
VEL, ACC, JRK, YAW = 0x01, 0x03, 0x07, 0x10
THREE = (-0.5, 0.0, 0.5)
STEP = 0.25
R_ROBOT = 0.3


def poison(dtype, n):
    return np.frombuffer(bytes([POISON]) * (np.dtype(dtype).itemsize * n), dtype).copy()


def upload(env, m, a):
    a = np.ascontiguousarray(a)
    buf = m.DeviceArray(env, max(a.nbytes, 8))
    buf.upload(a)
    return buf


def code(m, fn):
    with pytest.raises(m._abi.MplxError) as e:
        fn()
    return e.value.code


def rebase_raw(m, env, tab, roots, check, allow_wait, res, fr):
    """The C call with buffers of the test's own: 0xAB behind hit's n entries, behind the result and in n_blocked's
    neighbour.  Returns (rc, result dict, hit [capacity], n_blocked delta, device result bytes [40])."""
    lib = m._abi.lib()
    d_roots = upload(env, m, np.asarray(roots, np.int32))
    d_hit = upload(env, m, poison(np.int64, tab.capacity))
    d_nb = upload(env, m, np.concatenate([np.array([5], np.int64).view(np.uint8), poison(np.uint8, 8)]))  # the call adds to 5
    d_res = upload(env, m, poison(np.uint8, 40))
    h = m._abi.RebaseResult()
    f = fr.c_struct()
    rc = lib.mplx_table_rebase_timed_device(tab._tab, d_roots.ptr, 1 if check else 0, 1 if allow_wait else 0,
                                            None if res is None else res._res, C.byref(f), d_hit.ptr, d_nb.ptr, d_res.ptr, C.byref(h))
    out = None
    if rc == 0:
        nb = d_nb.download(np.uint8, (16,))
        assert np.all(nb[8:] == POISON)
        out = ({"n_kept": int(h.n_kept), "n_bad_edges": int(h.n_bad_edges), "n_roots": int(h.n_roots)},
               d_hit.download(np.int64, (tab.capacity,)), int(nb[:8].view(np.int64)[0]) - 5, d_res.download(np.uint8, (40,)))
    for b in (d_roots, d_hit, d_nb, d_res):
        b.free()
    return (rc,) + (out if out is not None else (None, None, None, None))


# ------------------------------------------------------------------------------------------------------ the worlds
def controls(dim, control, small=False):
    """small: two values per axis and two yaw rates, 2^(dim + 1) controls -- so that a table of 65 nodes holds nodes two
    edges deep although the equal keys of a round are expanded together."""
    axes = [THREE] * dim + ([(-0.3, 0.0, 0.3)] if control & YAW else [])
    if small:
        axes = [(0.0, 0.5)] * dim + ([(0.0, 0.3)] if control & YAW else [])
    return np.array(list(itertools.product(*axes)), dtype=np.float64)


def world(m, O, dim, control, small=False, j_max=0.0, yaw_max=0.0):
    """A free map with a few blocked cells, the engine's EnvMap and the oracle's Env of the same world."""
    n = 24 if dim == 2 else 12
    dims = [n] * dim
    grid = np.zeros(n ** dim, np.int8)
    rng = np.random.default_rng(dim * 100 + control)
    grid[rng.choice(n ** dim, size=n, replace=False)] = 100
    for q in range(3):  # the starts of the queries stand on free cells
        grid[cell_index(dims, [0.0] * dim, 1.0, [n / 2 + 0.5 + 2.0 * q] + [n / 2 + 0.5] * (dim - 1))] = 0
    U = controls(dim, control, small)
    env = m.EnvMap(dim)
    env.setMap([0.0] * dim, dims, grid, 1.0)
    env.set_control(control)
    env.set_u(U)
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    if j_max > 0:
        env.set_j_max(j_max)
    if yaw_max > 0:
        env.set_yaw_max(yaw_max)
    if control & YAW:
        env.set_wyaw(0.0)  # (the yaw term of the cost goes through the device's cos / sin: out of this comparison)

    def oenv(g):
        more = dict(j_max=j_max) if j_max > 0 else {}
        if yaw_max > 0:
            more["yaw_max"] = yaw_max
        return O.Env(dim, control, U, g, dims, [0.0] * dim, 1.0, dt=1.0, w=float(env._p.w), wyaw=0.0 if control & YAW else 1.0,
                     v_max=1.0, a_max=1.0, **more)
    cfg = TR.Config(dim, control, U, 1.0, float(env._p.w), (1.0, 1.0, j_max, yaw_max))
    return env, grid, dims, oenv, cfg


def standing(m, env, dim, control, positions, H, small=False):
    """Chains that stand still: the zero action H times from rest at `positions` [B][D]."""
    a0 = TR.WM.zero_action(controls(dim, control, small))
    starts = np.stack([m.Waypoint(dim, control, pos=list(p)).to_row() for p in positions], axis=1)
    return starts, np.full((H, len(positions)), a0, np.int32)


def restore_all(m, tab, d, jerk_rows=False):
    """restore() and the t row of the states (what poked_table_classes alters besides g and pred); jerk_rows: and the
    jerk rows, which it alters at order 4."""
    restore(m, tab, d)
    v, n = tab.view(), d["n_nodes"]
    D = (tab.n_fields - 2) // 4
    for f in [tab.n_fields - 1] + (list(range(3 * D, 4 * D)) if jerk_rows else []):
        row = np.ascontiguousarray(d["state"][f, :n])
        m._abi.check(tab._env._ctx, m._abi.lib().mplx_memcpy_h2d(tab._env._ctx, int(v.state + 8 * f * v.state_stride), row.ctypes.data,
                                                                 row.nbytes))


def is_wait_edge(T, cfg, i):
    if T.pred[i] < 0 or T.pred_action[i] != cfg.a0:
        return False
    pe = TR.WM.pair_eval(cfg.dim, cfg.control, T.state[T.pred[i]], cfg.U[cfg.a0], cfg.dt, *cfg.limits)
    return pe["h_next"] == pe["h_curr"]


def poked_table_classes(m, O, env, tab, d0, Q, cfg, oenv, roots, wait, res, table, queries, n_steps, n0, name):
    """The classes of node a map edit and a refill never make, poked into the downloaded table: a parent whose t was
    altered (its children's keys no longer match), a g below what the edge gives, a cycle of predecessors; and the call
    with allow_wait = 0 on a table that holds wait edges.  Each class is asserted from the model before the device is
    compared with it."""
    T0 = TR.multi_table(d0, Q)
    e0 = RP.OracleEdges(O, oenv, T0)
    held = lambda T, e, i, aw: not TR.edge_is_bad(T, i, e, cfg, True, aw)
    # (never a root of the call: a root is kept whatever its edge is)
    plain = [i for i in range(n0) if 0 <= T0.pred[i] < n0 and T0.pred_action[i] != cfg.a0 and math.isfinite(T0.g[i]) and i not in roots]
    e0.prepare([T0.pred[i] for i in plain])
    good = [i for i in plain if held(T0, e0, i, False)]  # ordinary edges that hold on the edited map
    parents = {}
    for i in good:
        parents.setdefault(T0.pred[i], i)
    has_child = set(p for p in T0.pred if p >= 0)
    P = next(p for p in parents if T0.pred[p] >= 0)          # a non-root parent of a holding edge
    child = parents[P]
    low = next(i for i in good if i not in (P, child) and T0.pred[i] != P)
    leaves = [i for i in good if i not in has_child and i not in (P, child, low)][:2]
    assert len(leaves) == 2, name
    x, y = leaves
    d1 = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in d0.items()}
    d1["state"][-1, P] += 0.5
    d1["g"][low] -= 1.0
    d1["pred"][x], d1["pred"][y] = y, x
    T1 = TR.multi_table(d1, Q)
    e1 = RP.OracleEdges(O, oenv, T1)
    assert held(T0, e0, child, False) and not held(T1, e1, child, False), name + ": the key of an altered parent's child"
    assert held(T0, e0, low, False) and not held(T1, e1, low, False), name + ": a g that is too small"
    if wait:  # a wait edge that holds with allow_wait and is bad without
        waits = [i for i in range(n0) if is_wait_edge(T1, cfg, i) and i not in (x, y)]
        assert any(held(T1, e1, i, True) and not held(T1, e1, i, False) for i in waits[:50]), name + ": no wait edge in the table"
    restore_all(m, tab, d1)
    want_fr, want, want_hit, want_nb, status = TR.rebase_timed(T1, e1, cfg, roots, True, False, True, table, queries, n_steps)
    assert status == 0 and math.isinf(T1.g[x]) and math.isinf(T1.g[y]) and math.isinf(T1.g[child]) and math.isinf(T1.g[low]), name
    fr = patterned_frontier(m, env, d0["n_nodes"], 32)
    rc, got, hit, nb, dres = rebase_raw(m, env, tab, roots, True, False, res, fr)
    what = name + " poked, allow_wait 0"
    print(what, want, "blocked", want_nb)
    assert rc == 0 and got == want, "%s: %r != %r" % (what, got, want)
    assert_frontier_equal(fr.download(), want_fr, what)
    assert_rebased_equal(tab, T1, what)
    assert np.array_equal(hit[:d0["n_nodes"]], want_hit) and nb == want_nb, what
    assert_spare_untouched(fr, what)
    fr.free()


def poked_jerk_rows(m, O, env, tab, d0, Q, cfg, oenv, roots, wait, res, table, queries, n_steps, n0, name):
    """Order 4: the jerk row of up to three parents moved by one hash bin, nothing else.  Edge by edge, the edges that held
    and no longer do are exactly the children of those parents -- some of them by their key alone, on an edge the map and
    the limits still accept --, and the rebase drops them as the model says.  The call is made without the reservation
    table: in the small tables every edge is blocked or past the horizon, which would drop the children whatever the edge
    kernel says of them."""
    D = cfg.dim
    T0 = TR.multi_table(d0, Q)
    e0 = RP.OracleEdges(O, oenv, T0)
    held = lambda T, e, i: not TR.edge_is_bad(T, i, e, cfg, True, wait)
    edges = [i for i in range(n0) if 0 <= T0.pred[i] < n0 and math.isfinite(T0.g[i]) and i not in roots]
    e0.prepare([T0.pred[i] for i in edges])
    good = [i for i in edges if held(T0, e0, i)]
    jerked = sorted(set(T0.pred[i] for i in good))[:3]
    assert jerked, name
    d1 = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in d0.items()}
    d1["state"][3 * D, jerked] += 0.1
    T1 = TR.multi_table(d1, Q)
    e1 = RP.OracleEdges(O, oenv, T1)
    e1.prepare([T1.pred[i] for i in edges])
    children = [i for i in good if T0.pred[i] in jerked]
    assert [i for i in good if not held(T1, e1, i)] == children and len(children) >= 2, (name, children)
    by_key = []
    for i in children:
        if T0.pred_action[i] == cfg.a0 and is_wait_edge(T0, cfg, i):
            continue
        st, h, _ = e1(T0.pred[i], T0.pred_action[i])
        if st == RP.SLOT_FINITE and TR.RM.time_key(h, float(np.float64(T1.state[T0.pred[i]][-1]) + np.float64(cfg.dt))) != T1.hash[i]:
            by_key.append(i)
    assert by_key, name + ": no child of a parent with an altered jerk row is dropped by its key alone"
    restore_all(m, tab, d1, jerk_rows=True)
    # (the same call on the unaltered table keeps them: what drops them is the moved jerk row)
    Tk = TR.multi_table(d0, Q)
    TR.rebase_timed(Tk, e0, cfg, roots, True, wait, True, None, queries, n_steps)
    kept_before = [i for i in children if math.isfinite(Tk.g[i])]
    assert kept_before, name
    want_fr, want, want_hit, want_nb, status = TR.rebase_timed(T1, e1, cfg, roots, True, wait, True, None, queries, n_steps)
    assert status == 0 and all(math.isinf(T1.g[i]) for i in children), name
    fr = patterned_frontier(m, env, d0["n_nodes"], 32)
    rc, got, hit, nb, dres = rebase_raw(m, env, tab, roots, True, wait, None, fr)
    what = name + " jerk rows of %s moved by one bin" % jerked
    print(what, want, "children", len(children), "by key alone", len(by_key))
    assert rc == 0 and got == want, "%s: %r != %r" % (what, got, want)
    assert_frontier_equal(fr.download(), want_fr, what)
    assert_rebased_equal(tab, T1, what)
    assert want_hit is None and nb == want_nb == 0, what
    assert_spare_untouched(fr, what)
    fr.free()
    restore_all(m, tab, d0, jerk_rows=True)


# name, dim, control, Q, B, step, wait, n nodes, park (False: GONE, reservations end)
CASES = [
    ("2d-acc-n1-B1", 2, ACC, 1, 1, 0.25, True, 1, True),
    ("2d-acc-n63-B15", 2, ACC, 1, 15, 0.25, True, 63, True),
    ("2d-vel-n65-B64-nowait", 2, VEL, 1, 64, 0.3, False, 65, False),
    ("3d-acc-n257-B70-Q3", 3, ACC, 3, 70, 0.25, True, 257, True),
    ("2d-accyaw-n257-B257", 2, ACC | YAW, 1, 257, 0.3, True, 257, False),
    ("2d-jrk-n4100-B64-Q3", 2, JRK, 3, 64, 0.25, True, 4100, True),
    ("3d-vel-n4100-B15-nowait", 3, VEL, 1, 15, 0.3, False, 4100, True),
]
# SNP, the yaw flags and K = 3 in 3-D (tests/control_matrix.py)
CASES = CASES + CM.TIMED_ADDED


@pytest.mark.parametrize("name,dim,control,Q,B,step,wait,n_target,park", CASES, ids=[c[0] for c in CASES])
def test_rebase_timed_equals_the_model(engine, oracle_lib, name, dim, control, Q, B, step, wait, n_target, park):
    m, O = engine, oracle_lib
    small = name in CM.TIMED_SMALL_U
    j_max, yaw_max = CM.TIMED_LIMITS.get(name, (0.0, 0.0))
    env, grid, dims, oenv_of, cfg = world(m, O, dim, control, small, j_max, yaw_max)
    n = dims[0]
    rng = np.random.default_rng(len(name) + n_target)
    centre = np.full(dim, n / 2 + 0.5)
    starts = np.stack([m.Waypoint(dim, control, pos=list(centre + (np.arange(dim) == 0) * 2.0 * q)).to_row() for q in range(Q)], axis=1)
    goals = np.stack([m.Waypoint(dim, control, pos=[n - 1.5] * dim).to_row() for _ in range(Q)])
    q_t0, q_r, q_ign = [0.0, 0.5, 1.0][:Q], [0.2] * Q, [-1, 1, 2][:Q]
    st, ac = standing(m, env, dim, control, [centre + 3.0, centre - 3.0], 3, small)
    res = m.search.Reservations(env, (st, ac), step, 200, None, 0.2, None, True)
    # ---- a time-keyed table of at most n_target nodes from a short search, padded to n_target with seeds
    # (delta = 0: a round expands one key's nodes, so the node count grows in small steps; the largest max_rounds whose
    # table still fits is found by doubling and bisection -- the count is monotone in max_rounds)
    def grown(rounds):
        return env.search_many(starts, goals, avoid=res, t0=q_t0, radius=q_r, ignore_group=q_ign, time_keys=True, wait=wait,
                               delta=0.0, max_rounds=rounds, capacity=1 << 16, max_frontier=8192, sight=False)
    sr, lo, hi = grown(0), 0, 1
    while hi < 8192:
        nxt = grown(hi)
        if nxt.table.stats()[0] > n_target:
            nxt.free()
            break
        sr.free()
        sr, lo, hi = nxt, hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        nxt = grown(mid)
        if nxt.table.stats()[0] > n_target:
            nxt.free()
            hi = mid
        else:
            sr.free()
            sr, lo = nxt, mid
    tab = sr.table
    n0 = tab.stats()[0]
    assert Q <= n0 <= n_target
    if n_target > n0:
        pad = np.stack([m.Waypoint(dim, control, pos=[100.0 + j] + [100.0] * (dim - 1)).to_row() for j in range(n_target - n0)], axis=1)
        tmp = m.TableFrontier(env, n_target)
        tab.seed(pad, 1.0, frontier=tmp, query=None if Q == 1 else np.arange(n_target - n0) % Q)
        tmp.free()
    d0 = tab.download()
    assert d0["n_nodes"] == n_target and d0["status"] == 0
    T0 = TR.multi_table(d0, Q)
    dep = depths(T0)
    has_child = set(p for p in T0.pred if p >= 0)
    # ---- the disturbance: a map edit under nodes with children, and a refill
    seed_cells = [cell_index(dims, [0.0] * dim, 1.0, starts[:dim, q]) for q in range(Q)]
    cells = []
    for i in [i for i in range(n0) if dep[i] >= 2 and i in has_child][::7]:
        c = cell_index(dims, [0.0] * dim, 1.0, T0.state[i])
        if c not in seed_cells and c not in cells and len(cells) < 3:
            cells.append(c)
    grid2 = grid.copy()
    if cells:
        env.editMap(cells, 100)
        grid2[cells] = 100
    oenv = oenv_of(grid2)
    below = [i for i in range(n0) if dep[i] >= 1]
    where = [T0.state[i][:dim] for i in below[::max(len(below) // 6, 1)][:min(B, 6)]]
    where += [rng.uniform(1.0, n - 1.0, dim) for _ in range(B - len(where))]
    st, ac = standing(m, env, dim, control, where, 8, small)
    b_t0 = np.array([0.0] * min(B, 6) + [float(x) for x in rng.integers(0, 8, B - min(B, 6)) * 0.5])[:B]
    b_r = np.full(B, 0.2)
    b_r[4::5] = -1.0  # excluded (BAD_INPUT): they block nothing
    t_max = max([T0.state[i][-1] for i in range(n0) if T0.pred[i] >= 0] + [1.0])
    n_steps = int((t_max - 0.5) / step) + 1  # the deepest edges of query 0 (t0 = 0) leave the horizon
    res.fill((st, ac), step, n_steps, b_t0, b_r, np.arange(B, dtype=np.int32) % 4, park)
    res.set_queries(q_t0, q_r, q_ign)
    table = dict(res.positions(), step=step)
    queries = (q_t0, q_r, q_ign)
    # ---- roots: query 0 one edge down where the model keeps and drops; query 1 its seed; query 2 out of range
    root0 = -1
    for r in [i for i in range(n0) if dep[i] == 1 and i in has_child and T0.query[i] == 0][:2]:
        T = TR.multi_table(d0, Q)
        _, info, _, _, _ = TR.rebase_timed(T, RP.OracleEdges(O, oenv, T), cfg, ([r, -1, n_target + 7])[:Q], True, wait, True, table, queries,
                                           n_steps)
        if info["n_kept"] >= 2:
            root0 = r
            break
    roots = ([root0, -1, tab.capacity + 7])[:Q]
    seen = {"kept": False, "dropped": False, "hit": False, "horizon": False, "bad": False}
    for check, use_res in ((True, True), (False, True), (True, False)):
        what = "%s check %d res %d" % (name, check, use_res)
        restore(m, tab, d0)
        T = TR.multi_table(d0, Q)
        want_fr, want, want_hit, want_nb, status = TR.rebase_timed(T, RP.OracleEdges(O, oenv, T), cfg, roots, check, wait, True,
                                                                   table if use_res else None, queries, n_steps)
        assert status == 0
        fr = patterned_frontier(m, env, n_target, 32)
        rc, got, hit, nb, dres = rebase_raw(m, env, tab, roots, check, wait, res if use_res else None, fr)
        assert rc == 0 and got == want, "%s: %r != %r" % (what, got, want)
        assert_frontier_equal(fr.download(), want_fr, what)
        assert_rebased_equal(tab, T, what)
        assert_spare_untouched(fr, what)
        assert np.all(dres[24:] == POISON) and dres[:24].view(np.int64).tolist() == [want["n_kept"], want["n_bad_edges"], want["n_roots"]]
        assert np.all(hit[n_target:] == poison(np.int64, 1)[0]), what
        if use_res:
            assert np.array_equal(hit[:n_target], want_hit), what + ": hit"
            assert nb == want_nb == int((want_hit != -1).sum()), what
            seen["hit"] |= bool((want_hit >= 0).any())
            seen["horizon"] |= bool((want_hit == -2).any())
        else:
            assert np.all(hit[:n_target] == poison(np.int64, 1)[0]) and nb == 0, what  # without res nothing of either is written
        seen["kept"] |= want["n_kept"] > want["n_roots"]
        seen["dropped"] |= want["n_kept"] < n_target
        seen["bad"] |= want["n_bad_edges"] > 0
        print(what, want, "blocked", want_nb, "hits", None if want_hit is None else int((want_hit >= 0).sum()),
              "horizon", None if want_hit is None else int((want_hit == -2).sum()))
        fr.free()
    if n_target == 1:
        assert not any(seen.values())  # one node: a root, kept, and nothing else to say
    else:
        assert all(seen.values()), (name, seen)
        poked_table_classes(m, O, env, tab, d0, Q, cfg, oenv, roots, wait, res, table, queries, n_steps, n0, name)
        if cfg.K == 4:
            poked_jerk_rows(m, O, env, tab, d0, Q, cfg, oenv, roots, wait, res, table, queries, n_steps, n0, name)
        # a frontier one row too small
        restore_all(m, tab, d0)
        T = TR.multi_table(d0, Q)
        want_fr, want, _, _, _ = TR.rebase_timed(T, RP.OracleEdges(O, oenv, T), cfg, roots, True, wait, True, table, queries, n_steps)
        short = patterned_frontier(m, env, want["n_kept"] - 1, 8)
        rc, got, hit, nb, dres = rebase_raw(m, env, tab, roots, True, wait, res, short)
        assert rc == 0 and got == want and tab.stats()[1] & m.table.FRONTIER_FULL
        assert int(short.count.download(np.int64, (1,))[0]) == want["n_kept"] - 1
        assert_spare_untouched(short, name)
        short.free()
    sr.free()
    res.free()
    env.close()


def test_without_the_new_features_the_bytes_of_the_multi_rebase(engine, oracle_lib):
    m, O = engine, oracle_lib
    env, grid, dims, oenv_of, cfg = world(m, O, 2, ACC)
    start = m.Waypoint(2, ACC, pos=[12.5, 12.5]).to_row()
    goal = m.Waypoint(2, ACC, pos=[22.5, 22.5]).to_row()
    sr = env.search(start, goal, max_rounds=6, capacity=1 << 14, max_frontier=8192, sight=False)
    tab = sr.table
    d0 = tab.download()
    T0 = RP.table_from_arrays(d0)
    dep = depths(T0)
    seed_cell = cell_index(dims, [0.0, 0.0], 1.0, start)
    cells = [c for c in (cell_index(dims, [0.0, 0.0], 1.0, T0.state[i]) for i in range(d0["n_nodes"]) if dep[i] >= 4) if c != seed_cell]
    cells = sorted(set(cells))[:3]  # (from rest a robot leaves its cell only after a few primitives)
    assert cells
    env.editMap(cells, 100)
    has_child = set(p for p in T0.pred if p >= 0)
    for root in (-1, [i for i in range(d0["n_nodes"]) if dep[i] == 1 and i in has_child][0]):
        outs = []
        for timed in (False, True):
            restore(m, tab, d0)
            fr = patterned_frontier(m, env, d0["n_nodes"], 16)
            if timed:
                rc, info, hit, nb, _ = rebase_raw(m, env, tab, [root], True, False, None, fr)
                assert rc == 0
            else:
                info = tab.rebase(roots=[root], check_edges=True, frontier=fr)
            d = tab.download()
            outs.append((info, fr.download(), d))
            assert_spare_untouched(fr)
            fr.free()
        (i0, f0, t0), (i1, f1, t1) = outs
        print("root", root, i0)
        assert i0 == i1 and (root >= 0 or (i0["n_bad_edges"] >= 1 and 2 <= i0["n_kept"] < d0["n_nodes"]))
        assert_frontier_equal(f1, f0)
        for k in ("hash", "g", "pred", "pred_action", "state"):
            assert np.array_equal(t0[k].view(np.uint8), t1[k].view(np.uint8)), k
    sr.free()
    env.close()


def test_errors_of_the_header_and_both_python_refusals(engine, oracle_lib):
    m, O = engine, oracle_lib
    lib, A = m._abi.lib(), m._abi
    env, grid, dims, oenv_of, cfg = world(m, O, 2, ACC)
    start = m.Waypoint(2, ACC, pos=[12.5, 12.5]).to_row()
    goal = m.Waypoint(2, ACC, pos=[22.5, 22.5]).to_row()
    st, ac = standing(m, env, 2, ACC, [[15.5, 12.5]], 4)
    res = m.search.Reservations(env, (st, ac), STEP, 100, None, 0.2, None, True)
    sr = env.search(start, goal, avoid=res, radius=0.2, wait=True, max_rounds=3, capacity=1 << 12, sight=False)
    tab = sr.table
    n = tab.stats()[0]
    fr = m.TableFrontier(env, n)
    roots = upload(env, m, np.array([-1], np.int32))
    h = A.RebaseResult()

    def call(t=tab._tab, r=roots.ptr, check=1, w=1, rs=res._res, f=fr, hit=None, nb=None):
        fs = f.c_struct() if f is not None else None
        return lib.mplx_table_rebase_timed_device(t, r, check, w, rs, C.byref(fs) if fs is not None else None, hit, nb, None, C.byref(h))
    d0 = tab.download()
    assert call() == A.OK and h.n_kept == n and h.n_bad_edges == 0 and h.n_roots == 1  # nothing changed: everything holds
    restore(m, tab, d0)
    # the untimed rebases still refuse the table, and replan() names the new method
    assert code(m, lambda: tab.rebase(roots=[-1], frontier=fr)) == A.ERR_STATE
    assert code(m, lambda: tab.rebase(root=-1, frontier=fr)) == A.ERR_STATE
    with pytest.raises(RuntimeError, match="replan_timed"):
        sr.replan()
    with pytest.raises(ValueError):
        sr.replan_timed()  # the search ran with avoid: the reservations are required
    # NULL and malformed arguments
    assert call(t=None) == A.ERR_ARG and call(r=None) == A.ERR_ARG and call(f=None) == A.ERR_ARG
    bad = m.TableFrontier(env, n)
    bad.state_stride = n - 1
    assert call(f=bad) == A.ERR_ARG
    # a reservation table of another context, set for another Q, before a fill, before set_queries
    env2, *_ = world(m, O, 2, ACC)
    st2, ac2 = standing(m, env2, 2, ACC, [[15.5, 12.5]], 4)
    other = m.search.Reservations(env2, (st2, ac2), STEP, 100, None, 0.2, None, True)
    other.set_queries(0.0, 0.2)
    assert call(rs=other._res) == A.ERR_ARG
    res.set_queries([0.0, 1.0], [0.2, 0.2])
    assert call() == A.ERR_ARG
    empty = C.c_void_p()
    A.check(env._ctx, lib.mplx_reserve_create(env._ctx, C.byref(empty)))
    assert call(rs=empty) == A.ERR_STATE
    lib.mplx_reserve_destroy(empty)
    unset = m.search.Reservations(env, (st, ac), STEP, 100, None, 0.2, None, True)
    assert call(rs=unset._res) == A.ERR_STATE
    unset.free()
    res.set_queries(0.0, 0.2)
    assert call() == A.OK
    restore(m, tab, d0)
    # check_edges without a map, parameters or controls; res = NULL and check_edges = 0 need none of them
    bare = m.EnvMap(2)
    tb = m.NodeTable(bare, 64)
    fb = m.TableFrontier(bare, 64)
    rb = upload(bare, m, np.array([-1], np.int32))
    assert call(t=tb._tab, r=rb.ptr, check=1, rs=None, f=fb) == A.ERR_STATE
    assert call(t=tb._tab, r=rb.ptr, check=0, rs=None, f=fb) == A.OK and h.n_kept == 0  # a table without nodes: a no-op
    assert int(fb.count.download(np.int64, (1,))[0]) == 0
    for b in (rb, fb, tb):
        b.free()
    bare.close()
    # a table with a status bit
    short = m.TableFrontier(env, n - 1)
    assert call(f=short) == A.OK and tab.stats()[1] & m.table.FRONTIER_FULL
    assert call() == A.ERR_STATE
    # a search without time keys and without avoid is refused by replan_timed
    plain = env.search(start, goal, max_rounds=2, capacity=1 << 12, sight=False)
    with pytest.raises(ValueError, match="replan"):
        plain.replan_timed()
    plain.free()
    for b in (short, bad, fr, roots, other, sr, res):
        b.free()
    env2.close()
    env.close()


# ------------------------------------------------------------------------------------------------------ scenarios
def lane_env(m, cells):
    env = m.EnvMap(2)
    env.setMap([0.0, 0.0], [cells.shape[1], cells.shape[0]], cells.ravel(), 1.0)
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls(list(THREE), 2))
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    return env


def fresh_from(env, result, root, goal, res, t0, kw):
    """EnvMap.search from the state of `root` with t = 0, on the clock t0 + t_root, seeded with g_root."""
    s = result.table.state_of(root)
    g = float(result.table._read(result.table.view().g + 8 * int(root), np.float64, 1)[0])
    t_root = float(s[-1])
    s[-1] = 0.0
    out = env.search(s, goal, avoid=res, t0=t0 + t_root, start_g=g, **kw)
    cost = out.cost
    st = out.status
    out.free()
    return st, cost, t_root


def charged(env, chains, t0, n_steps):
    H = max(len(a) for _, a in chains)
    st = np.stack([s for s, _ in chains], axis=1)
    ac = np.full((H, len(chains)), -1, np.int32)
    for k, (_, a) in enumerate(chains):
        ac[:len(a), k] = a
    return env.traj_conflicts(st, ac, STEP, n_steps=n_steps, t0=np.asarray(t0, dtype=np.float64), radius=R_ROBOT, park=True).charged


def test_scenario_pocket_lane(engine):
    """The pocket lane of tests/test_wait_model.py at delta = 0: robot 1, planned among robot 0 with waits and the park
    veto, advances k primitives; robot 0 is delayed by 2.5 s; robot 1 replans on its table.  Status, cost, the rebase's
    counts and full_path() action for action are the model's (tests/test_timed_replan_model.py records them); the cost is
    that of a fresh search from the root state; nobody is charged.  For k = 5 a second replan follows (robot 0 delayed
    to 4.0 s, three more primitives made) and the executed part accumulates."""
    m = engine
    cells = np.full((7, 17), 100, np.int8)  # [y][x]
    cells[3, :] = 0
    cells[4:6, 9] = 0
    env = lane_env(m, cells)
    wp = lambda p: m.Waypoint(2, m.ACC, pos=p).to_row()
    s0, g0, s1, g1 = wp([1.5, 3.5]), wp([15.5, 3.5]), wp([9.5, 3.5]), wp([13.5, 3.5])
    n_steps = int(60 / STEP)
    kw = dict(radius=R_ROBOT, time_keys=True, wait=True, park_goal=True, delta=0.0, capacity=1 << 17, max_frontier=4096, sight=False)
    solo = env.search(s0, g0, delta=0.0, capacity=1 << 15, max_frontier=4096, sight=False)
    p0 = solo.path()
    assert solo.cost == 150.5
    chain0 = (p0[0].reshape(-1, 1), p0[1].reshape(-1, 1))
    res = m.search.Reservations(env, chain0, STEP, n_steps, [0.0], R_ROBOT, None, True)
    for k in (0, 2, 5, 8):
        res.fill(chain0, STEP, n_steps, [0.0], R_ROBOT, None, True)
        r1 = env.search(s1, g1, avoid=res, t0=0.0, **kw)
        assert r1.found and r1.cost == 141.5
        old_actions = r1.path()[1]
        assert np.array_equal(r1.full_path()[1], old_actions)  # never replanned: full_path is path
        root = int(r1.table.path(r1.goal_id)[0][k])
        res.fill(chain0, STEP, n_steps, [DELAY], R_ROBOT, None, True)
        new = r1.replan_timed(avoid=res, advance=k)
        assert r1.table is None and new.found
        start, acts = new.full_path()
        want = POCKET_RECORD[k]
        print("k =", k, new, new.rebase_info, acts.tolist())
        assert new.cost == POCKET_COSTS[k]
        assert (new.rebase_info["n_kept"], new.rebase_info["n_bad_edges"], new.rebase_info["n_blocked"]) == want[:3]
        assert new.rebase_info["n_blocked"] > 0 and new.rebase_info["n_roots"] == 1
        assert acts.tolist() == want[3] and np.array_equal(bits(start), bits(s1)) and np.array_equal(acts[:k], old_actions[:k])
        assert new.path()[0][-1] == float(k) and len(new.path()[1]) == len(acts) - k
        st, cost, t_root = fresh_from(env, new, root, g1, res, 0.0, kw)
        assert st == m.search.FOUND and cost == new.cost and t_root == float(k)
        assert not charged(env, [p0, (start, acts)], [DELAY, 0.0], n_steps).any()
        if k == 5:
            res.fill(chain0, STEP, n_steps, [DELAY2], R_ROBOT, None, True)
            root2 = int(new.table.path(new.goal_id)[0][3])
            again = new.replan_timed(avoid=res, advance=3)
            start2, acts2 = again.full_path()
            want = POCKET_RECORD["5+3"]
            print("k = 5 + 3", again, again.rebase_info, acts2.tolist())
            assert again.found and again.cost == POCKET_COSTS["5+3"] and acts2.tolist() == want[3]
            assert (again.rebase_info["n_kept"], again.rebase_info["n_bad_edges"], again.rebase_info["n_blocked"]) == want[:3]
            assert np.array_equal(acts2[:8], acts[:8]) and again.path()[0][-1] == 8.0 and np.array_equal(bits(start2), bits(s1))
            st, cost, t_root = fresh_from(env, again, root2, g1, res, 0.0, kw)
            assert st == m.search.FOUND and cost == again.cost and t_root == 8.0
            assert not charged(env, [p0, (start2, acts2)], [DELAY2, 0.0], n_steps).any()
            new = again
        new.free()
    # nothing changed: no bad edge, nothing blocked, the old cost and the old chain
    res.fill(chain0, STEP, n_steps, [0.0], R_ROBOT, None, True)
    r1 = env.search(s1, g1, avoid=res, t0=0.0, **kw)
    old_actions = r1.path()[1]
    same = r1.replan_timed(avoid=res, advance=3)
    assert same.found and same.cost == 141.5 and same.rebase_info["n_bad_edges"] == same.rebase_info["n_blocked"] == 0
    assert np.array_equal(same.full_path()[1], old_actions)
    same.free()
    solo.free()
    res.free()
    env.close()


def crossing(m):
    n = 33
    cells = np.full((n, n), 100, np.int8)  # [y][x]
    cells[16, :] = 0
    cells[:, 16] = 0
    env = lane_env(m, cells)
    wp = lambda p: m.Waypoint(2, m.ACC, pos=p).to_row()
    starts = np.stack([wp([2.5, 16.5]), wp([16.5, 12.5])], axis=1)
    goals = np.stack([wp([30.5, 16.5]), wp([16.5, 16.5])])
    return env, cells, starts, goals


def test_scenario_crossing_with_delay_candidates(engine):
    """The 33 x 33 crossing of tests/test_gpu_wait.py.  Robot 1 is planned as a MultiSearchResult of three delay candidates
    among a robot 0 that starts 2.5 s late; robot 0 then starts on time after all, so it passes the crossing while the old
    plan of robot 1 is still on it, and the winner replans after 3 primitives while the losers, given roots out of range,
    end EMPTY.  Status, cost, the rebase's counts and full_path() are those the model records.  The cost is that of a fresh search from the root state and nobody is charged."""
    m = engine
    env, cells, starts, goals = crossing(m)
    n_steps = int(120 / STEP)
    solo = env.search(starts[:, 0], goals[0], delta=0.0, capacity=1 << 15, max_frontier=4096)
    p0 = solo.path()
    chain0 = (p0[0].reshape(-1, 1), p0[1].reshape(-1, 1))
    res = m.search.Reservations(env, chain0, STEP, n_steps, [DELAY], R_ROBOT, None, True)
    delays = np.array(CROSSING_DELAYS)
    kw = dict(radius=R_ROBOT, time_keys=True, wait=True, park_goal=True, delta=0.0, capacity=1 << 17, max_frontier=4096, sight=False)
    many = env.search_many(np.repeat(starts[:, 1:2], 3, axis=1), np.repeat(goals[1:2], 3, axis=0), avoid=res, t0=delays, **kw)
    assert all(many.found)
    ends = [delays[q] + len(many.path(q)[1]) for q in range(3)]
    win = int(np.argmin(ends))
    k = CROSSING_K
    want = CROSSING_RECORD  # from tests/timed_replan_model.py on the CPU (tests/test_timed_replan_model.py)
    assert [many.cost[q] for q in range(3)] == want["first_costs"] and win == want["winner"]
    root = int(many.table.path(many.goal_id[win])[0][k])
    roots = [many.table.capacity] * 3
    roots[win] = root
    res.fill(chain0, STEP, n_steps, [0.0], R_ROBOT, None, True)
    new = many.replan_timed(avoid=res, roots=roots)
    print("crossing:", new, new.rebase_info, "winner", win)
    assert new.found[win] and [new.status[q] for q in range(3) if q != win] == [m.search.EMPTY] * 2
    assert new.rebase_info["n_roots"] == 1 and new.rebase_info["n_blocked"] > 0
    start, acts = new.full_path(win)
    assert np.array_equal(bits(start), bits(starts[:, 1])) and len(acts) - k == len(new.path(win)[1])
    # status, cost, the rebase's counts and full_path action for action are the model's
    assert new.status == want["status"] and new.cost[win] == want["cost"] and acts.tolist() == want["actions"]
    assert {x: new.rebase_info[x] for x in ("n_kept", "n_bad_edges", "n_roots", "n_blocked")} == {
        x: want[x] for x in ("n_kept", "n_bad_edges", "n_roots", "n_blocked")}
    s = new.table.state_of(root)
    g_root = float(new.table._read(new.table.view().g + 8 * root, np.float64, 1)[0])
    t_root = float(s[-1])
    s[-1] = 0.0
    fresh = env.search(s, goals[1], avoid=res, t0=float(delays[win]) + t_root, start_g=g_root, **kw)
    assert t_root == float(k) and fresh.found and fresh.cost == new.cost[win]
    assert not charged(env, [p0, (start, acts)], [0.0, float(delays[win])], n_steps).any()
    for b in (fresh, new, solo, res):
        b.free()
    env.close()


def test_fleet_replan_prioritised(engine):
    """plan_prioritised(keep=True) on the crossing, then at now = 4 a lane cell ahead of robot 0 is blocked and a bypass
    is opened; replan_prioritised replans both robots in order.  Nobody is charged, robot 1's new plan keeps clear of
    robot 0's new one, both chains start at the original starts and keep the primitives made so far; replanned once more
    after both have arrived, every robot keeps its goal and its chain."""
    m = engine
    env, cells, starts, goals = crossing(m)
    kw = dict(capacity=1 << 17, max_frontier=4096, n_steps=int(160 / STEP))
    plan = m.search.plan_prioritised(env, starts, goals, STEP, R_ROBOT, wait=True, park_goal=True, keep=True, **kw)
    assert plan["status"] == [m.search.FOUND] * 2 and not plan["conflicts"].charged.any() and plan["winner"] == [0, 0]
    old = [(p[0].copy(), p[1].copy()) for p in plan["paths"]]
    # robot 0 is at x = 2.5 + ... along y = 16.5; block the lane at x = 10 and open a bypass through y = 17
    idx = lambda x, y: x + 33 * y
    env.editMap([idx(10, 16)], 100)
    env.editMap([idx(x, 17) for x in range(8, 13)], 0)
    new = m.search.replan_prioritised(env, plan, 4.0, STEP)
    print("fleet:", new["status"], new["cost"], [len(p[1]) for p in new["paths"]], new["rebase"], new["conflicts"].first_step)
    assert new["status"] == [m.search.FOUND] * 2 and not new["conflicts"].charged.any()
    assert new["rebase"][0]["n_bad_edges"] > 0 and new["cost"][0] > plan["cost"][0]  # the lane is cut: robot 0 goes round
    for r in range(2):
        assert np.array_equal(bits(new["paths"][r][0]), bits(starts[:, r])) and np.array_equal(new["paths"][r][1][:4], old[r][1][:4])
    # both have arrived: every robot keeps its goal and its chain
    late = m.search.replan_prioritised(env, new, 1000.0, STEP)
    assert late["status"] == [m.search.FOUND] * 2 and not late["conflicts"].charged.any()
    for r in range(2):
        assert np.array_equal(late["paths"][r][1], new["paths"][r][1]) and late["cost"][r] == new["cost"][r]
        assert len(late["results"][r].path(late["winner"][r])[1]) == 0
    for o in late["results"]:
        o.free()
    env.close()
