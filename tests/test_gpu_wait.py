"""Wait edges (include/mplx_wait.h, wait_kernel.hip), park-safe goals (mplx_reserve_park_device of include/mplx_reserve.h,
reserve_kernel.hip) and the search that uses both (EnvMap.search(wait=, park_goal=), search.plan_prioritised), on the
device, against tests/wait_model.py, tests/reserve_model.py and conflicts()."""
import ctypes as C
import math

import numpy as np
import pytest

import control_matrix as CM
import reserve_model as RM
import wait_model as WM

pytestmark = pytest.mark.gpu

POISON = 0xAB
STEP = 0.25


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def poison(dtype, n):
    return np.frombuffer(bytes([POISON]) * (np.dtype(dtype).itemsize * n), dtype).copy()


def upload(env, m, a):
    buf = m.DeviceArray(env, max(a.nbytes, 8))
    buf.upload(a)
    return buf


def plain_env(m, dim, control, U, dt=1.0):
    """Parameters and controls on an all-free map (neither call reads a map cell)."""
    env = m.EnvMap(dim)
    env.setMap([0.0] * dim, [8] * dim, np.zeros(8 ** dim, np.int8), 1.0)
    env.set_control(control)
    env.set_u(U)
    env.set_v_max(3.0)
    env.set_a_max(3.0)
    env.set_dt(dt)
    return env


def code(m, fn):
    with pytest.raises(m._abi.MplxError) as e:
        fn()
    return e.value.code


# ------------------------------------------------------------------------------------------------------ add_wait
NINE, THREE = CM.NINE, CM.THREE
# (dim, control, axis values, yaw, nU, S)
WAIT_CASES = [
    (2, "VEL", THREE, False, 9, 9),
    (2, "ACC", THREE, False, 9, 9),
    (3, "ACC", THREE, False, 27, 32),
    (2, "ACC", NINE, False, 81, 96),
    (2, "ACCxYAW", THREE, True, 27, 32),
    (3, "JRK", THREE, False, 27, 32),
    (2, "JRK", NINE, False, 81, 96),
    (3, "VEL", THREE, False, 27, 32),
]
WAIT_IDS = ["2d-vel-S9", "2d-acc-S9", "3d-acc-27of32", "2d-acc-81of96", "2d-yaw-27of32", "3d-jrk-27of32", "2d-jrk-81of96",
            "3d-vel-27of32"]
# the other nine instantiations of lists_add_wait_kernel (tests/control_matrix.py): their parents carry live acc and jerk rows
WAIT_CASES = WAIT_CASES + [(d, c, THREE, y, nU, S) for (d, c, y, nU, S) in CM.WAIT_ADDED]
WAIT_IDS = WAIT_IDS + [CM.wait_id(*c) for c in CM.WAIT_ADDED]
N_ROWS, N_ALLOC = 70, 72  # more than one wave of lanes; two rows behind n_nodes that no call may touch
MIN_SENSITIVE = 5         # parents whose answer a zeroed acc (order >= 3) or jerk (order 4) row has to change


def wait_inputs(rng, dim, order, yaw, F, nU, S, live_rows=False):
    """70 parents of the kinds: at rest (eligible), moving, same hash with a moved position, too slow to move at all
    (eligible), and with yaw controls a velocity the heading limit refuses; counts with 0 and -- where S == nU -- S among
    them; two rows with parent_id = -1.

    live_rows (the added cases): eight parents at rest each become kind 5 (order >= 3: an acceleration inside the hash bin
    of 0 that moves the position; not eligible), kind 6 (order 4: vel == acc == 0 and a jerk inside the hash bin of 0
    that moves the position; not eligible) and kind 7 (order 4: a jerk of 1e-20, eligible, and the successor's vel, acc
    and jrk rows carry it); half of the movers of order 4 carry a jerk as well."""
    n = N_ROWS
    pst = np.zeros((F, N_ALLOC))
    pst[:dim, :n] = np.round(rng.uniform(1.0, 7.0, size=(dim, n)), 2)
    kind = rng.choice(5, p=[0.45, 0.25, 0.15, 0.1, 0.05], size=n)
    kind[:5] = [0, 1, 2, 3, 4]
    if order >= 2:
        ax = np.zeros(n, np.int64) if yaw else rng.integers(0, dim, size=n)  # (with a heading limit: along +x, inside it)
        for k in range(n):
            if kind[k] == 1:
                pst[dim + ax[k], k] = rng.choice([-1.0, -0.5, 0.5, 1.0])
            elif kind[k] == 2:
                pst[dim + ax[k], k] = 0.004      # inside the velocity bin of 0, and 4 mm in one primitive: inside the cell
            elif kind[k] == 3:
                pst[dim + ax[k], k] = 1e-20      # pos + v T == pos
            elif kind[k] == 4 and yaw:
                pst[dim, k], pst[dim + 1, k] = 1e-20, 0.0
    if order >= 3:
        pst[2 * dim, :n] = np.where((kind == 1) & (rng.random(n) < 0.5), 0.5, 0.0)  # some movers accelerate as well
    if yaw:
        pst[4 * dim, :n] = rng.choice([0.0, 0.1, -0.2, 0.3], size=n)
        pst[4 * dim, :n][kind == 4] = 1.5        # looks along +y while creeping along +x: outside yaw_max = 0.5
    pst[F - 1, :n] = rng.integers(0, 9, size=n) * 1.0
    count = rng.integers(0, min(S, nU), size=N_ALLOC).astype(np.int32)
    count[[1, 9]] = 0
    if S == nU:
        count[[6, 13, 20]] = S                   # a full list takes no entry
    parent_id = np.arange(N_ALLOC, dtype=np.int32)
    parent_id[[7, 33]] = -1
    if order == 1:  # a VEL state has no velocity and every parent is eligible: rows without a parent keep the share down
        parent_id[:n][rng.random(n) < 0.3] = -1
        parent_id[0] = 0
    if live_rows and order >= 3:  # (after every draw of the cases above: their inputs are what they were)
        rest = [k for k in np.nonzero(kind == 0)[0] if k >= 5 and parent_id[k] >= 0 and 0 < count[k] < S]  # (rows that are written)
        assert len(rest) >= (24 if order >= 4 else 8), len(rest)
        new_kinds = {5: (2 * dim, 0.004)}
        if order >= 4:
            new_kinds.update({6: (3 * dim, 0.004), 7: (3 * dim, 1e-20)})
            jerked = (kind == 1) & (rng.random(n) < 0.5)
            for k in np.nonzero(jerked)[0]:
                pst[3 * dim + ax[k], k] = rng.choice([-0.5, 0.5])
        for which, (row, value) in sorted(new_kinds.items()):
            for k in rest[:8]:
                kind[k] = which
                pst[row + ax[k], k] = value
            rest = rest[8:]
    return pst, kind, count, parent_id


def wait_sensitivity(pst, parent_id, count, dim, flag, U, w, yaw, goal, F, S):
    """On the model alone: per parent, has the answer (eligibility, or any byte of its list row) changed with the acc
    rows zeroed, and for order 4 with the jerk rows zeroed?  {row name: number of parents}."""
    n, N, order = N_ROWS, N_ALLOC * S, WM.order_of(flag)

    def answer(states):
        host = {"stride": S, "count": count.copy(), "action": poison(np.int32, N), "cost": poison(np.float64, N),
                "hash": poison(np.uint64, N), "state": poison(np.float64, F * N).reshape(F, N), "heur": poison(np.float64, N),
                "flags": poison(np.uint8, N), "iters": poison(np.int32, N)}
        _, eligible = WM.add_wait(host, n, states, parent_id, dim, flag, U, 1.0, w, 3.0, 3.0, 0.0, 0.5 if yaw else 0.0, goal)
        rows = [b"".join(np.ascontiguousarray(host[key][..., k * S:(k + 1) * S]).tobytes() for key in
                         ("action", "cost", "hash", "state", "heur", "flags", "iters")) + bytes([int(eligible[k])]) + host["count"][k].tobytes()
                for k in range(n)]
        return rows
    base = answer(pst)
    out = {}
    for name, lo in (("acc", 2 * dim),) + ((("jrk", 3 * dim),) if order >= 4 else ()):
        z = pst.copy()
        z[lo:lo + dim] = 0.0
        out[name] = sum(a != b for a, b in zip(base, answer(z)))
    return out


def eligible_of(pst, rows, dim, flag, U, yaw):
    """The pair's three conditions for the parents `rows` (a mask), from the model."""
    u0 = np.asarray(U)[WM.zero_action(U)]
    out = []
    for k in np.nonzero(rows)[0]:
        p = WM.pair_eval(dim, flag, pst[:, k], u0, 1.0, 3.0, 3.0, 0.0, 0.5 if yaw else 0.0)
        out.append(p["h_next"] == p["h_curr"] and p["valid"] and p["same_pos"])
    return np.array(out, dtype=bool)


def wait_case(m, dim, control, vals, yaw, nU, S, w=10.0):
    """The inputs of one case, without a device: (U, flag, order, F, goal, pst, kind, count, parent_id, a0)."""
    rng = np.random.default_rng(7 * dim + S + len(control))
    U = m.workloads.grid_controls(vals, dim, yaw_rates=[-0.3, 0.0, 0.3]) if yaw else m.workloads.grid_controls(vals, dim)
    assert len(U) == nU
    perm = rng.permutation(nU)  # a0 is wherever the shuffle put the zero row
    U = np.ascontiguousarray(np.asarray(U)[perm])
    flag = getattr(m, control)
    order = WM.order_of(flag)
    F = 4 * dim + 2
    goal_row = np.zeros(F)
    goal_row[:dim] = 4.0
    goal = dict(row=goal_row, hash=WM.lattice_hash(dim, flag, goal_row), w=w, v_max=3.0, tol_pos=1.5, tol_vel=-1.0, tol_acc=-1.0,
                tol_yaw=-1.0)
    added_case = (dim, control, yaw, nU, S) in CM.WAIT_ADDED  # (by the case, not the pair: JRK has old and added cases)
    pst, kind, count, parent_id = wait_inputs(rng, dim, order, yaw, F, nU, S, live_rows=added_case)
    pst[:dim, 0] = 4.0  # one wait inside the goal region, on the goal's own lattice state
    if yaw:
        pst[4 * dim, 0] = 0.0
    a0 = WM.zero_action(U)
    assert a0 == int(np.nonzero(np.all(U == 0, axis=1))[0][0])
    return U, flag, order, F, goal, pst, kind, count, parent_id, a0


def assert_wait_case_is_sensitive(dim, control, yaw, nU, S, U, flag, order, F, goal, pst, kind, count, parent_id, w=10.0):
    """The higher-order rows decide something: on the model alone (tests/test_control_matrix.py runs it without a device)."""
    moved = wait_sensitivity(pst, parent_id, count, dim, flag, U, w, yaw, goal, F, S)
    print("%dd %s: parents whose answer a zeroed row changes: %s" % (dim, control, moved))
    if (dim, control, yaw, nU, S) in CM.WAIT_ADDED:  # (the two old JRK cases keep their inputs and only print; the -live ones assert)
        assert all(v >= MIN_SENSITIVE for v in moved.values()), moved
        assert (kind == 5).sum() == 8 and not eligible_of(pst, kind == 5, dim, flag, U, yaw).any()
        if order >= 4:
            assert not eligible_of(pst, kind == 6, dim, flag, U, yaw).any() and eligible_of(pst, kind == 7, dim, flag, U, yaw).all()
    return moved


@pytest.mark.parametrize("dim,control,vals,yaw,nU,S", WAIT_CASES, ids=WAIT_IDS)
def test_add_wait_equals_the_model(engine, dim, control, vals, yaw, nU, S):
    m = engine
    U, flag, order, F, goal, pst, kind, count, parent_id, a0 = wait_case(m, dim, control, vals, yaw, nU, S)
    if order >= 3:  # asserted before the device runs
        assert_wait_case_is_sensitive(dim, control, yaw, nU, S, U, flag, order, F, goal, pst, kind, count, parent_id)
    env = plain_env(m, dim, flag, U)
    if yaw:
        env.set_yaw_max(0.5)
    assert F == env.n_fields and float(env._p.w) == goal["w"] and env.nU == nU
    env.set_goal(goal["row"], w=10.0, v_max=3.0, tol_pos=1.5)
    n, N = N_ROWS, N_ALLOC * S
    for full in (True, False):  # every row of the lists; then only count / action / cost
        host = {"stride": S, "count": count.copy(), "action": poison(np.int32, N), "cost": poison(np.float64, N)}
        if full:
            host.update(hash=poison(np.uint64, N), state=poison(np.float64, F * N).reshape(F, N), heur=poison(np.float64, N),
                        flags=poison(np.uint8, N), iters=poison(np.int32, N))
        L = m.Lists(env, N_ALLOC, nU, want_state=full, want_hash=full, want_iters=full, want_heur=full, want_flags=full, stride=S)
        L.count.upload(host["count"])
        L.action.upload(host["action"])
        L.cost.upload(host["cost"])
        if full:
            L.hash.upload(host["hash"])
            L.state.upload(host["state"])
            L.heur.upload(host["heur"])
            L.flags.upload(host["flags"])
            L.iters.upload(host["iters"])
        fr = m.TableFrontier(env, N_ALLOC)
        fr.id.upload(parent_id)
        fr.state.upload(pst)
        d_n = upload(env, m, np.array([5], np.int64))
        want_n, eligible = WM.add_wait(host, n, pst, parent_id, dim, flag, U, 1.0, float(env._p.w), 3.0, 3.0, 0.0,
                                       0.5 if yaw else 0.0, goal)
        s = L.c_struct()
        m._abi.check(env._ctx, m._abi.lib().mplx_lists_add_wait_device(env._ctx, C.byref(s), n, fr.ptr, fr.n_nodes, fr.id.ptr, d_n.ptr))
        env.synchronize()
        got = L.download()
        share = want_n / n
        print("%s full %d: eligible %d added %d (%.2f) kinds %s" % (control, full, eligible.sum(), want_n, share, np.bincount(kind, minlength=5)))
        assert np.array_equal(got["count"], host["count"]) and int(d_n.download(np.int64, (1,))[0]) == 5 + want_n
        assert np.array_equal(got["action"], host["action"])
        assert np.array_equal(bits(got["cost"]), bits(host["cost"]))
        if full:
            assert np.array_equal(got["hash"], host["hash"])
            assert np.array_equal(bits(got["state"]), bits(host["state"]))
            assert np.array_equal(bits(got["heur"]), bits(host["heur"])) and np.array_equal(got["flags"], host["flags"])
            assert np.array_equal(got["iters"], host["iters"])
            added = np.nonzero(host["action"][:n * S] != poison(np.int32, 1)[0])[0]
            assert len(added) == want_n and np.all(host["action"][added] == a0) and np.all(host["iters"][added] == 0)
            assert np.all(host["flags"][added] <= 3) and host["flags"][0 * S + count[0]] == 3  # the wait on the goal's own lattice state
        # the model alone: the share, and every kind of row
        assert 0.2 <= share <= 0.8, share
        if order >= 2:
            assert eligible[kind == 0].all() and eligible[kind == 3].all() and not eligible[kind == 1].any() and not eligible[kind == 2].any()
            assert 0.2 <= eligible.mean() <= 0.8
            if yaw:
                assert (kind == 4).any() and not eligible[kind == 4].any()
        else:
            assert eligible.all()  # a VEL state has no velocity: only parent_id and a full list keep a wait out
        for b in (d_n, fr, L):
            b.free()
    env.close()


def test_add_wait_errors_and_the_zero_rows_mask(engine):
    m = engine
    A = m._abi
    U = m.workloads.grid_controls(THREE, 2)
    env = plain_env(m, 2, m.ACC, U)
    env._flush()  # (parameters and controls reach the context with the next call of the EnvMap's own)
    F = env.n_fields
    n = 6
    L = m.Lists(env, n, 9, want_state=True, stride=9)
    assert L.zero_rows == (1 << F) - 1
    L.count.upload(np.full(n, 3, np.int32))
    fr = m.TableFrontier(env, n)
    fr.id.upload(np.arange(n, dtype=np.int32))
    st = np.zeros((F, n))
    st[:2] = [[1.5] * n, [2.5] * n]
    fr.state.upload(st)
    raw = lambda s, nn, ps, stride, pid, na: A.check(env._ctx, A.lib().mplx_lists_add_wait_device(env._ctx, s, nn, ps, stride, pid, na))
    s = L.c_struct()
    assert code(m, lambda: raw(None, n, fr.ptr, n, fr.id.ptr, None)) == A.ERR_ARG
    assert code(m, lambda: raw(C.byref(s), -1, fr.ptr, n, fr.id.ptr, None)) == A.ERR_ARG
    assert code(m, lambda: raw(C.byref(s), n, None, n, fr.id.ptr, None)) == A.ERR_ARG
    assert code(m, lambda: raw(C.byref(s), n, fr.ptr, n - 1, fr.id.ptr, None)) == A.ERR_ARG  # parent_stride < n_nodes
    no_cost = L.c_struct()
    no_cost.cost = None
    assert code(m, lambda: raw(C.byref(no_cost), n, fr.ptr, n, fr.id.ptr, None)) == A.ERR_ARG
    raw(C.byref(s), 0, fr.ptr, n, fr.id.ptr, None)  # n_nodes == 0
    # the mask: a chain standing somewhere gives a Reservations to call add_waits on
    res = env.alloc_reservations((st[:, :1], np.zeros((1, 1), np.int32)), STEP, n_steps=8, radius=0.1)
    mask = L.zero_rows
    res.add_waits(fr, L, n)  # parent_id given; all six at rest
    env.synchronize()
    got = L.download()
    assert L.zero_rows == mask and got["count"].tolist() == [4] * n
    const_rows = [f for f in range(F) if f >= 4 and f != F - 1]  # ACC in 2D: acc, jrk and yaw rows
    assert np.all(bits(got["state"][const_rows]) == 0)  # all +0.0, the wait entries included
    e = 3
    assert got["state"][:, e].tolist() == [1.5, 2.5, 0, 0, 0, 0, 0, 0, 0, 1.0] and got["action"][e] == 4
    # parent_id NULL: no row is skipped
    raw(C.byref(s), n, fr.ptr, n, None, None)
    env.synchronize()
    assert L.download()["count"].tolist() == [5] * n
    # heur / flags without a goal
    Lh = m.Lists(env, n, 9, want_state=False, want_heur=True, stride=9)
    Lh.count.upload(np.zeros(n, np.int32))
    sh = Lh.c_struct()
    assert code(m, lambda: raw(C.byref(sh), n, fr.ptr, n, fr.id.ptr, None)) == A.ERR_STATE
    # a control table without a zero row
    env.set_u(np.asarray(U)[[0, 1, 2, 3, 5, 6, 7, 8]])
    env._flush()
    assert code(m, lambda: raw(C.byref(s), n, fr.ptr, n, fr.id.ptr, None)) == A.ERR_STATE
    # arguments that need each other
    start = m.Waypoint(2, m.ACC, pos=[0.5, 0.5]).to_row()
    with pytest.raises(ValueError):
        env.search(start, start, wait=True)
    with pytest.raises(ValueError):
        env.search(start, start, park_goal=True, time_keys=True)
    with pytest.raises(ValueError):
        env.search_many(start.reshape(-1, 1), start.reshape(1, -1), wait=True, time_keys=False, avoid=res, radius=0.1)
    for b in (res, Lh, fr, L):
        b.free()
    env.close()


# ------------------------------------------------------------------------------------------------------ park
# (dim, B, n_steps, frontier rows, Q, park, step)
PARK_CASES = [
    (2, 1, 3, 1, 1, True, 0.25),
    (2, 70, 130, 64, 1, False, 0.3),
    (3, 257, 130, 200, 3, True, 0.25),
    (2, 257, 130, 65, 3, False, 0.25),
    (3, 70, 3, 65, 1, True, 0.3),
    (3, 1, 130, 64, 3, False, 0.3),
    (2, 70, 130, 200, 1, True, 0.25),
]
PARK_IDS = ["2d-B1-3steps-1row", "2d-B70-64rows-gone", "3d-B257-200rows-Q3", "2d-B257-65rows-Q3-gone", "3d-B70-3steps-65rows",
            "3d-B1-64rows-Q3-gone", "2d-B70-200rows"]


@pytest.mark.parametrize("dim,B,n_steps,rows,Q,park,step", PARK_CASES, ids=PARK_IDS)
def test_park_equals_the_model(engine, dim, B, n_steps, rows, Q, park, step):
    m = engine
    rng = np.random.default_rng(1000 + B + n_steps + rows + Q)
    U = m.workloads.grid_controls([-1.0, 0.0, 1.0], dim)
    nU = len(U)
    env = plain_env(m, dim, m.VEL, U)
    F = env.n_fields
    horizon = (n_steps - 1) * step
    # ---- the reservations: B - 1 short chains that roam [2, 6]^D, and the last one far off, moving for the whole
    # horizon (so that GONE keeps it to the last instant): the one the sole hits are made of
    H = max(int(math.ceil(horizon)) + 2, 6)
    r_starts = np.zeros((F, B))
    r_starts[:dim] = rng.uniform(2.0, 6.0, size=(dim, B))
    r_actions = np.full((H, B), -1, np.int32)
    for b in range(B):
        k = int(rng.integers(1, 6))
        r_actions[:k, b] = rng.integers(0, nU, size=k)
    far = B - 1
    r_starts[:dim, far] = 40.0
    r_actions[:, far] = int(np.nonzero(np.all(np.asarray(U) == ([1.0] + [0.0] * (dim - 1)), axis=1))[0][0])  # +x for ever
    r_t0 = rng.choice([0.0, 0.5, 1.3], size=B)
    r_t0[far] = 0.0
    vol = 16.0 if dim == 2 else 64.0
    rr = math.sqrt(0.22 * vol / max(B, 2) / math.pi) if dim == 2 else (0.22 * vol / max(B, 2) * 0.75 / math.pi) ** (1.0 / 3.0)
    r_rad = rr * rng.uniform(0.5, 1.0, size=B)
    group = (np.arange(B) // 2).astype(np.int32)
    group[far] = 5000
    res = env.alloc_reservations((r_starts, r_actions), step, n_steps=n_steps, t0=r_t0, radius=r_rad, group=group, park=park)
    table = res.positions()
    table["step"] = step
    q_t0, q_r, q_ign = [0.0, 0.3, 1.0][:Q], [0.5 * rr, 0.7 * rr, 0.3 * rr][:Q], [-1, 1, 0][:Q]
    res.set_queries(q_t0, q_r, q_ign)

    # ---- a table of n_nodes nodes, about half of them inside their query's goal region, pushed: the open set's flags
    n_nodes = rows + 10
    tab = env.alloc_table(1024, n_queries=Q)
    opn = env.alloc_open(tab)
    goal_rows = np.zeros((Q, F))
    goal_rows[:, :dim] = 4.0
    if Q > 1:
        opn.set_goals(goal_rows, tol_pos=2.0)
    else:
        env.set_goal(goal_rows[0], tol_pos=2.0)
    seeds = np.zeros((F, n_nodes))
    inside = rng.random(n_nodes) < 0.55
    inside[:4] = True
    seeds[:dim] = np.where(inside[None, :], 2.5 + 0.01 * np.arange(n_nodes)[None, :] + 0.5 * np.arange(dim)[:, None],
                           20.0 + 0.01 * np.arange(n_nodes)[None, :])  # distinct lattice states
    node_query = (np.arange(n_nodes) % Q).astype(np.int32)
    fr0 = m.TableFrontier(env, n_nodes)
    assert tab.seed(seeds, frontier=fr0, query=node_query if Q > 1 else None) == n_nodes  # node k = seed k
    opn.push(fr0, n_max=n_nodes)
    env.synchronize()
    before = opn.download()
    assert np.array_equal((before["flags"] & m.search.IS_GOAL) != 0, inside)

    # ---- the frontier handed to park: hand-made rows (park reads the row's state, not the table's)
    cap = rows + 3
    ids = rng.permutation(n_nodes)[:cap].astype(np.int32)
    st = np.zeros((F, cap))
    st[:dim] = rng.uniform(2.0, 6.0, size=(dim, cap))
    st[F - 1] = rng.choice([0.0, 1.0, 2.5, 7.0], size=cap)
    special = {}
    goal_nodes = [int(i) for i in np.nonzero(inside)[0]]

    def put(r, node, pos, t):
        ids[r] = node
        others = np.nonzero(ids == node)[0]
        for o in others[others != r]:  # a frontier holds every id once
            ids[o] = -1
        st[:dim, r], st[F - 1, r] = pos, t
    i_sp = min(7, n_steps - 2)
    if rows < 64:
        ids[:rows] = goal_nodes[:rows]
    if rows >= 64:
        qn = lambda k: q_t0[node_query[k]]
        last_i = n_steps - 1
        a, b_, c_, d_ = goal_nodes[:4]
        # a sole hit at (n_steps - 1, B - 1): on the far reservation's last position, arriving exactly at the last instant
        put(0, a, table["pos"][last_i, :, far], np.float64(last_i) * np.float64(step) - np.float64(qn(a)))
        special["last"] = 0
        # a sole hit at the row's first instant: on the far reservation at instant i_sp, arriving just before it
        t7 = np.float64(i_sp) * np.float64(step) - np.float64(qn(b_))
        put(rows - 1, b_, table["pos"][i_sp, :, far], np.nextafter(t7, -np.inf))
        special["first"] = rows - 1
        # past the horizon: no instants
        put(5, c_, table["pos"][0, :, far], horizon + 1.0)
        special["past"] = 5
        ids[9], ids[11], ids[12] = -1, n_nodes, n_nodes + 500  # ids out of range
    if Q > 1 and rows >= 64 and B > 4:
        # on a reservation of the group the query ignores, from t = 0 on (its partner of the same group stands elsewhere)
        node = next(k for k in goal_nodes[4:] if node_query[k] == 1)
        put(20, node, table["pos"][0, :, 2], 0.0)
        special["ignored"] = 20
    n_count = rows + 1      # one more row than n_max lets through
    fr = m.TableFrontier(env, cap)
    fr.id.upload(ids)
    fr.state.upload(st)
    fr.count.upload(np.array([n_count], np.int64))
    PAT = np.int64(0x5A5A5A5A5A5A5A5A)
    d_hit, d_nv = upload(env, m, np.full(cap, PAT, np.int64)), upload(env, m, np.array([3], np.int64))
    host_fr = {"count": n_count, "id": ids, "state": st}
    want_flags, want_hit, want_nv = WM.park(before["flags"], n_nodes, host_fr, rows, cap, table, (q_t0, q_r, q_ign), dim,
                                            node_query if Q > 1 else None)
    res.park(opn, fr, rows, hit=d_hit, n_vetoed=d_nv)
    env.synchronize()
    after = opn.download()
    got_hit = d_hit.download(np.int64, (cap,))
    looked = np.array([0 <= i < n_nodes and bool(before["flags"][i] & m.search.IS_GOAL) for i in ids[:rows]])
    print("B %d rows %d: goal rows %d vetoed %d kept %d" % (B, rows, looked.sum(), want_nv, looked.sum() - want_nv))
    assert np.array_equal(after["flags"], want_flags)
    assert np.array_equal(bits(after["f"]), bits(before["f"]))
    assert np.array_equal(got_hit[:rows], want_hit) and np.all(got_hit[rows:] == PAT)  # rows past n_max are not written
    assert int(d_nv.download(np.int64, (1,))[0]) == 3 + want_nv
    assert np.array_equal(after["flags"] | m.search.IS_GOAL, before["flags"] | m.search.IS_GOAL)  # no other bit moved
    if rows >= 64:  # on the model's answer: what the case is there for
        assert 0.2 <= looked.mean() <= 0.8, looked.mean()
        assert 0 < want_nv < looked.sum()
        assert want_hit[special["last"]] == ((n_steps - 1) << 32) | far
        assert want_hit[special["first"]] == (i_sp << 32) | far
        assert want_hit[special["past"]] == -1 and looked[special["past"]]
        if "ignored" in special:
            r = special["ignored"]
            assert looked[r] and (want_hit[r] == -1 or (want_hit[r] & 0xFFFFFFFF) not in (2, 3))
    else:
        assert looked.all()
    # a second call vetoes nothing new: the vetoed nodes have no goal bit any more
    res.park(opn, fr, rows, hit=d_hit, n_vetoed=d_nv)
    env.synchronize()
    assert int(d_nv.download(np.int64, (1,))[0]) == 3 + want_nv and np.array_equal(opn.download()["flags"], want_flags)
    for b in (d_hit, d_nv, fr, fr0, opn, tab, res):
        b.free()
    env.close()


def test_park_one_row_both_answers(engine):
    """The smallest frontier, vetoed and kept: one row on a reservation that stands for 2 s and is reached at t = 2.75.
    PARK: it is still there at the row's first instant, 11; GONE: it ended at t = 2."""
    m = engine
    U = m.workloads.grid_controls([-1.0, 0.0, 1.0], 2)
    env = plain_env(m, 2, m.VEL, U)
    F = env.n_fields
    st = np.zeros((F, 1))
    st[:2, 0] = [3.0, 3.0]
    env.set_goal(st[:, 0], tol_pos=0.5)
    for park_mode, want in ((True, 11 << 32), (False, -1)):
        res = env.alloc_reservations((st, np.full((2, 1), 4, np.int32)), STEP, n_steps=40, radius=0.2, park=park_mode)
        res.set_queries(0.0, 0.2)
        tab = env.alloc_table(64)
        opn = env.alloc_open(tab)
        fr = m.TableFrontier(env, 1)
        assert tab.seed(st, frontier=fr) == 1
        st_t = st.copy()
        st_t[F - 1] = 2.75
        fr.state.upload(st_t)
        opn.push(fr, n_max=1)
        d_hit = upload(env, m, np.zeros(1, np.int64))
        res.park(opn, fr, 1, hit=d_hit)
        env.synchronize()
        flags = opn.download()["flags"]
        assert d_hit.download(np.int64, (1,))[0] == want
        assert flags[0] == m.search.SEEN | m.search.IS_OPEN | (m.search.IS_GOAL if want == -1 else 0)
        for b in (d_hit, fr, opn, tab, res):
            b.free()
    env.close()


def test_park_errors_and_no_ops(engine):
    m = engine
    A = m._abi
    U = m.workloads.grid_controls([-1.0, 0.0, 1.0], 2)
    env = plain_env(m, 2, m.VEL, U)
    F = env.n_fields
    st = np.zeros((F, 1))
    res = env.alloc_reservations((st, np.zeros((1, 1), np.int32)), STEP, n_steps=8, radius=0.1)
    tab = env.alloc_table(64)
    opn = env.alloc_open(tab)
    fr = m.TableFrontier(env, 4)
    fr.count.upload(np.array([0], np.int64))
    assert code(m, lambda: res.park(opn, fr, 4)) == A.ERR_STATE                      # no queries yet
    res.set_queries([0.0, 1.0], 0.3)
    assert code(m, lambda: res.park(opn, fr, 4)) == A.ERR_ARG                        # two queries, a table of one
    res.set_queries(0.0, 0.3)
    assert code(m, lambda: res.park(opn, fr, -1)) == A.ERR_ARG
    raw = lambda *a: A.check(env._ctx, A.lib().mplx_reserve_park_device(*a))
    assert code(m, lambda: raw(res._res, None, C.byref(fr.c_struct()), 4, None, None)) == A.ERR_ARG
    assert code(m, lambda: raw(res._res, opn._open, None, 4, None, None)) == A.ERR_ARG
    other = m.EnvMap(2)
    tab_o = other.alloc_table(64)
    opn_o = other.alloc_open(tab_o)
    assert code(m, lambda: res.park(opn_o, fr, 4)) == A.ERR_ARG                      # an open set of another context
    opn_o.free()
    tab_o.free()
    other.close()
    res.park(opn, fr, 0)   # n_max == 0
    res.park(opn, fr, 4)   # an empty frontier
    env.synchronize()
    for b in (fr, opn, tab, res):
        b.free()
    env.close()


# ------------------------------------------------------------------------------------------------------ composition
def test_the_check_sees_a_wait_edge(engine):
    """A wait entry made by add_waits at a position a reservation sits on: the unchanged check blocks it, with the hit
    the model gives (a zero control from rest evaluates to a constant position)."""
    m = engine
    U = m.workloads.grid_controls(THREE, 2)
    env = plain_env(m, 2, m.ACC, U)
    F = env.n_fields
    n, S = 3, 9
    pst = np.zeros((F, n))
    pst[:2] = [[3.0, 3.0, 6.0], [3.0, 3.0, 6.0]]
    pst[F - 1] = [2.0, 30.0, 2.0]  # the second row's wait leaves the horizon
    sit = np.zeros((F, 1))
    sit[:2, 0] = [3.0, 3.25]
    n_steps = 41
    res = env.alloc_reservations((sit, np.full((3, 1), 4, np.int32)), 0.3, n_steps=n_steps, radius=0.2)  # parked at (3, 3.25)
    res.set_queries(0.1, 0.2)
    L = m.Lists(env, n, 9, want_state=True, stride=S)
    L.count.upload(np.zeros(n, np.int32))
    fr = m.TableFrontier(env, n)
    fr.id.upload(np.zeros(n, np.int32))
    fr.state.upload(pst)
    d_hit, d_na = upload(env, m, np.zeros(n * S, np.int64)), upload(env, m, np.zeros(1, np.int64))
    res.add_waits(fr, L, n, n_added=d_na)
    env.synchronize()
    got = L.download()
    assert got["count"].tolist() == [1, 1, 1] and int(d_na.download(np.int64, (1,))[0]) == 3
    cost_before = got["cost"].copy()
    want_cost, want_hit, want_nb, looked = RM.check(got["count"], got["action"], cost_before, S, np.zeros(n, np.int32), pst[F - 1], 1.0,
                                                    9, 0.3, n_steps, res.positions(), ([0.1], [0.2], [-1]),
                                                    lambda k, j, i, s: pst[:2, k])
    res.check(fr, L, n, hit=d_hit)
    env.synchronize()
    hit = d_hit.download(np.int64, (n * S,))
    assert np.array_equal(hit, want_hit) and want_nb == 2 and looked.sum() == 3
    first = int(RM.instants(0.3, n_steps, 0.1, 2.0, 3.0)[0])
    assert hit[0] == first << 32 and hit[S] == -2 and hit[2 * S] == -1
    after = L.download()["cost"]
    assert np.isinf(after[0]) and np.isinf(after[S]) and after[2 * S] == cost_before[2 * S] == float(env._p.w) * 1.0
    for b in (d_hit, d_na, fr, L, res):
        b.free()
    env.close()


# ------------------------------------------------------------------------------------------------------ scenarios
def lane_env(m, cells):
    env = m.EnvMap(2)
    env.setMap([0.0, 0.0], [cells.shape[1], cells.shape[0]], cells.ravel(), 1.0)
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls(THREE, 2))
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    return env


def n_waits(env, path):
    """Edges of a chain that leave the robot where it is (chain states with equal positions and zero velocity)."""
    info = env.traj_info(path[0], path[1].reshape(-1, 1), want_states=True)["seg_state"][:, :len(path[1]) + 1, 0]
    return int(np.sum(np.all(info[:4, 1:] == info[:4, :-1], axis=0)))


def test_scenario_parking(engine):
    """The crossing of tests/test_gpu_reserve.py (two one-cell lanes on a 33 x 33 map).  Robot 0 drives west to east as
    there; robot 1 starts at rest 4 m south of the crossing and its goal is the crossing cell; order [0, 1].

    Recorded on an MI355X.  Robot 0 alone: 290.5 over 29 primitives, at the crossing at t = 15.  With today's arguments
    robot 1 takes its solo plan (50.5, 5 primitives), stands on the crossing from t = 5 on and is charged at instant 58
    (distance 0).  With wait and park_goal both are found and nobody is charged: robot 0 keeps 290.5 and its actions;
    robot 1 pays 151.0 for 15 primitives, eight of them waits at its start, and ends at t = 15 in the corner (16, 16) of
    the goal region, 0.71 m from robot 0, which is closest to that corner at t = 14.5.  With park_goal alone and
    delays=(0,) it finds 151.5 over 15 primitives by creeping, nobody charged."""
    m = engine
    n = 33
    cells = np.full((n, n), 100, np.int8)  # [y][x]
    cells[16, :] = 0
    cells[:, 16] = 0
    env = lane_env(m, cells)
    wp = lambda p: m.Waypoint(2, m.ACC, pos=p).to_row()
    starts = np.stack([wp([2.5, 16.5]), wp([16.5, 12.5])], axis=1)
    goals = np.stack([wp([30.5, 16.5]), wp([16.5, 16.5])])
    R = 0.3
    kw = dict(capacity=1 << 17, max_frontier=4096, n_steps=int(120 / STEP))
    solo = env.search(starts[:, 0], goals[0], capacity=1 << 15, max_frontier=4096)
    a0 = 4
    # today's arguments: robot 1 parks on the crossing before robot 0 gets there, and only the final conflicts says so
    old = m.search.plan_prioritised(env, starts, goals, STEP, R, **kw)
    print("today:", old["status"], old["cost"], [len(p[1]) for p in old["paths"]], old["conflicts"].first_step, old["conflicts"].min_dist)
    assert old["status"] == [m.search.FOUND] * 2 and old["conflicts"].charged.tolist() == [False, True]
    new = m.search.plan_prioritised(env, starts, goals, STEP, R, wait=True, park_goal=True, **kw)
    p1 = new["paths"][1]
    print("wait + park_goal:", new["status"], new["cost"], [len(p[1]) for p in new["paths"]], p1[1].tolist(), "waits", n_waits(env, p1),
          new["conflicts"].first_step, new["conflicts"].min_dist)
    assert new["status"] == [m.search.FOUND] * 2 and not new["conflicts"].charged.any()
    assert new["cost"][0] == solo.cost and np.array_equal(new["paths"][0][1], solo.path()[1])
    assert a0 in p1[1].tolist()
    # robot 1 arrives after robot 0 has passed: robot 0's passage is the instant at which it is closest to the place
    # robot 1 ends at (the goal region is a square of 1 m, and robot 1 may end in a corner of it)
    p0 = new["paths"][0]
    ti = np.arange(int(len(p0[1]) / STEP) + 1) * np.float64(STEP)
    xy0 = env.traj_sample(p0[0], p0[1].reshape(-1, 1), times=ti)["samples"][:2, 0, :]
    end1 = env.traj_info(p1[0], p1[1].reshape(-1, 1), want_states=True)["seg_state"][:2, len(p1[1]), 0]
    passage = float(ti[np.argmin(np.linalg.norm(xy0 - end1[:, None], axis=0))])
    arrival = len(p1[1]) * 1.0
    print("robot 1 ends at", end1, "at t =", arrival, "; robot 0 is closest to it at t =", passage)
    assert arrival > passage and arrival > len(old["paths"][1][1]) * 1.0
    assert (old["cost"][1], new["cost"][1], len(p1[1]), n_waits(env, p1)) == (50.5, 151.0, 15, 8)
    # park_goal without waits and without delays: recorded; held only to "nobody is charged if a plan is found"
    alone = m.search.plan_prioritised(env, starts, goals, STEP, R, wait=False, park_goal=True, delays=(0,), **kw)
    print("park_goal only:", alone["status"], alone["cost"], None if alone["paths"][1] is None else alone["paths"][1][1].tolist(),
          alone["conflicts"].first_step)
    if alone["status"][1] == m.search.FOUND:
        assert not alone["conflicts"].charged.any()
    solo.free()
    env.close()


def test_scenario_waiting_mid_path(engine):
    """One east-west lane with a side pocket two cells deep (tests/test_wait_model.py has the same map on the models).
    Robot 1 starts at rest on the lane below the pocket, in robot 0's way; its goal is further along the lane.

    Recorded from the models on the CPU: robot 0 alone 150.5 (15 primitives); robot 1 with wait and park_goal 141.5 (14
    primitives, six waits on the lane, then into the pocket and out), with park_goal alone 142.0 (14 primitives).  The
    MI355X returned the same costs and, action for action, the same two chains; closest approach 1.0 m in both."""
    m = engine
    cells = np.full((7, 17), 100, np.int8)  # [y][x]
    cells[3, :] = 0
    cells[4:6, 9] = 0
    env = lane_env(m, cells)
    wp = lambda p: m.Waypoint(2, m.ACC, pos=p).to_row()
    starts = np.stack([wp([1.5, 3.5]), wp([9.5, 3.5])], axis=1)
    goals = np.stack([wp([15.5, 3.5]), wp([13.5, 3.5])])
    R = 0.3
    kw = dict(capacity=1 << 17, max_frontier=4096, n_steps=int(60 / STEP), sight=False)
    both = m.search.plan_prioritised(env, starts, goals, STEP, R, wait=True, park_goal=True, **kw)
    park_only = m.search.plan_prioritised(env, starts, goals, STEP, R, wait=False, park_goal=True, **kw)
    print("wait + park_goal:", both["status"], both["cost"], both["paths"][1][1].tolist(), "waits", n_waits(env, both["paths"][1]),
          both["conflicts"].min_dist)
    print("park_goal only:", park_only["status"], park_only["cost"],
          None if park_only["paths"][1] is None else park_only["paths"][1][1].tolist(), park_only["conflicts"].min_dist)
    assert both["status"] == [m.search.FOUND] * 2 and not both["conflicts"].charged.any()
    assert park_only["status"][1] != m.search.FOUND or both["cost"][1] < park_only["cost"][1]
    assert not park_only["conflicts"].charged.any()
    assert n_waits(env, both["paths"][1]) >= 1
    assert (both["cost"][0], both["cost"][1], park_only["cost"][1]) == (150.5, 141.5, 142.0)
    env.close()


# ------------------------------------------------------------------------------------------------------ unchanged
def test_search_with_avoid_and_both_flags_off_is_unchanged(engine):
    """The corridor search among reservations of tests/test_gpu_reserve.py with wait and park_goal off: what the parent
    commit returns (the two builds, run side by side on an MI355X, printed the same lines): status, cost, rounds,
    expansions, node counts and path."""
    from test_gpu_open import corridor_env
    from test_multi import corridor_queries
    m = engine
    env, start, goal = corridor_env(m)
    starts, goals = corridor_queries(m)
    a = env.search(start, goal, capacity=1 << 15, max_frontier=4096)
    p = a.path()
    res = env.alloc_reservations((p[0].reshape(-1, 1), p[1].reshape(-1, 1)), STEP, n_steps=400, radius=0.4)
    one = env.search(starts[:, 2], goals[2], capacity=1 << 18, max_frontier=4096, avoid=res, radius=0.4)
    many = env.search_many(starts[:, [2, 1]], goals[[2, 1]], capacity=1 << 18, max_frontier=4096, avoid=res, radius=0.4, t0=[0.0, 2.0])
    got = (one.status, one.cost, one.rounds, one.expanded, one.table.stats(), one.path()[1].tolist())
    got_many = (many.status, many.cost, many.rounds, many.expanded, many.total_rounds, many.table.stats(),
                [many.path(q)[1].tolist() for q in range(2)])
    print("UNCHANGED one:", got)
    print("UNCHANGED many:", got_many)
    assert got == PARENT_ONE
    assert got_many == PARENT_MANY
    for x in (a, one, many, res):
        x.free()
    env.close()


# printed by the parent build and by this one, run side by side on an MI355X
PATH_BACK = [1, 1, 4, 4, 4, 5, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 3, 4, 4, 4, 5, 5]
PATH_SHIFTED = [7, 7, 4, 4, 5, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 4, 4, 4, 4, 3, 4, 4]
PARENT_ONE = (1, 352.0, 35, 6562, (13124, 0), PATH_BACK)
PARENT_MANY = ([1, 1], [352.0, 351.75], [35, 35], [6562, 6622], 35, (26496, 0), [PATH_BACK, PATH_SHIFTED])
