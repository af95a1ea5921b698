"""The reservation table and its check (include/mplx_reserve.h, reserve_kernel.hip), the time keys of the node table
(include/mplx_table.h) and the search among moving robots built on both (search.Reservations, EnvMap.search(avoid=),
search.plan_prioritised), on the device, against tests/reserve_model.py, tests/table_model.py and conflicts()."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import control_matrix as CM
import reserve_model as RM
from table_model import TableModel, hand_case
from test_gpu_open import corridor_env
from test_gpu_table import assert_frontier_equal, bits, upload, upload_lists
from test_multi import corridor_queries

pytestmark = pytest.mark.gpu

PAT64 = np.int64(0x5A5A5A5A5A5A5A5A)


def plain_env(m, dim, control, U, dt=1.0, lanes=None):
    """Parameters and controls on an all-free map (the check and the trajectory calls read no map cell).  lanes: the
    context's MPLX_RESERVE_LANES (read when it is created): lanes of a wave over a row's entries, None = automatic."""
    if lanes:
        os.environ["MPLX_RESERVE_LANES"] = str(lanes)
    try:
        env = m.EnvMap(dim)
    finally:
        os.environ.pop("MPLX_RESERVE_LANES", None)
    env.setMap([0.0] * dim, [8] * dim, np.zeros(8 ** dim, np.int8), 1.0)
    env.set_control(control)
    env.set_u(U)
    env.set_v_max(3.0)
    env.set_a_max(3.0)
    env.set_dt(dt)
    return env


def reserved_chains(rng, dim, F, nU, B, H):
    """B random chains of up to H primitives in [2, 6]^D: among them empty chains, bad actions (excluded by their
    status) and, through the radii, bad inputs."""
    starts = np.zeros((F, B))
    starts[:dim] = rng.uniform(2.0, 6.0, size=(dim, B))
    actions = rng.integers(0, nU, size=(H, B)).astype(np.int32)
    for b in range(B):
        actions[rng.integers(1, H + 1):, b] = -1
    if B >= 15:
        actions[0, 3] = -1       # TRAJ_EMPTY
        actions[1, 7] = nU + 5   # TRAJ_BAD_ACTION
    return starts, actions


NINE = CM.NINE
# (dim, control, axis values, yaw, S, B, park, step, Q, lanes); lanes: another split of a wave between a row's entries and
# slices of the reservations than the automatic one -- the same bytes
CASES = [
    (2, "ACC", [-0.5, 0.0, 0.5], False, 9, 15, True, 0.25, 1, None),
    (2, "ACC", NINE, False, 96, 70, False, 0.3, 1, None),
    (3, "VEL", [-1.0, 0.0, 1.0], False, 27, 257, True, 0.3, 3, None),
    (2, "ACCxYAW", [-0.5, 0.0, 0.5], True, 32, 1, False, 0.25, 1, None),
    (3, "ACC", [-0.5, 0.0, 0.5], False, 32, 70, True, 0.25, 3, None),
    (2, "VEL", [-1.0, 0.0, 1.0], False, 9, 257, False, 0.25, 1, None),
    (2, "ACC", [-0.5, 0.0, 0.5], False, 9, 15, True, 0.25, 1, 64),
    (2, "ACC", NINE, False, 96, 70, False, 0.3, 1, 8),
]
IDS = ["2d-acc-S9-B15", "2d-acc-81of96-B70-gone", "3d-vel-B257-Q3", "2d-yaw-B1-gone", "3d-acc-B70-Q3", "2d-vel-S9-B257-gone",
       "S9-all-lanes-on-entries", "81of96-eight-lanes-on-entries"]
# K = 3, K = 4 and the yaw flags (tests/control_matrix.py): parents with live acc and jerk rows
CASES = CASES + CM.RESERVE_ADDED
IDS = IDS + CM.RESERVE_ADDED_IDS
MIN_SENSITIVE = 10  # looked-at entries whose hit a zeroed acc (K >= 3) or jerk (K = 4) row has to change


def exact_positions(pst, U, act, times, dim, order):
    """p + v s + a s^2/2 + j s^3/6 + u s^4/24 without the terms past the order (the control takes the place of the first
    row the order does not hold), in exact rationals from the same doubles.  pst [4D+2][E], act [E], times [E][C].
    Returns (positions [D][E][C] as Fractions, sum of the terms' magnitudes [D][E][C])."""
    E, Cn = times.shape
    fact = [1, 1, 2, 6, 24]
    pos = np.empty((dim, E, Cn), dtype=object)
    mag = np.empty((dim, E, Cn), dtype=object)
    for e in range(E):
        for d in range(dim):
            coef = [Fraction(float(pst[k * dim + d, e])) for k in range(order)] + [Fraction(float(U[act[e]][d]))]
            for c in range(Cn):
                sx = Fraction(float(times[e, c]))
                terms = [coef[k] * sx ** k / fact[k] for k in range(order + 1)]
                pos[d, e, c], mag[d, e, c] = sum(terms), sum(abs(t) for t in terms)
    return pos, mag


@pytest.mark.parametrize("dim,control,vals,yaw,S,B,park,step,Q,lanes", CASES, ids=IDS)
def test_check_equals_the_model(engine, dim, control, vals, yaw, S, B, park, step, Q, lanes):
    m = engine
    rng = np.random.default_rng(100 + B + 7 * dim + S)
    U = m.workloads.grid_controls(vals, dim, yaw_rates=[-0.3, 0.0, 0.3]) if yaw else m.workloads.grid_controls(vals, dim)
    nU, dt = len(U), 1.0
    env = plain_env(m, dim, getattr(m, control), U, dt, lanes)
    F = env.n_fields
    # ---- the reservations: n_steps covers t <= 6.3, so that the rows at tp = 6 leave the horizon
    n_steps = int(6.3 / step) + 1
    r_starts, r_actions = reserved_chains(rng, dim, F, nU, B, 5)
    r_t0 = rng.choice([0.0, 0.5, 1.3, -0.7], size=B)
    # radii sized so that about half of the entries are blocked: B * volume(rr) ~ 0.7 * volume of [2, 6]^D
    rr = math.sqrt(3.5 / B) if dim == 2 else (10.7 / B) ** (1.0 / 3.0)
    r_rad = rr * rng.uniform(0.4, 0.8, size=B)
    if B >= 15:
        r_rad[5], r_rad[11], r_t0[12] = -1.0, np.nan, np.inf  # CONFLICT_BAD_INPUT
    group = (np.arange(B) // 2).astype(np.int32)
    res = env.alloc_reservations((r_starts, r_actions), step, n_steps=n_steps, t0=r_t0, radius=r_rad, group=group, park=park)
    table = res.positions()
    if B >= 15:
        assert table["included"][[3, 5, 7, 11, 12]].tolist() == [0] * 5 and table["included"].sum() == B - 5
        assert table["status"][[5, 11, 12]].tolist() == [128] * 3
    assert np.array_equal(table["group"], group) and table["pos"].shape == (n_steps, dim, B)
    if not park:
        assert 0 < table["active"].sum() < table["active"].size

    # ---- the queries, and whose the rows are
    q_t0, q_r, q_ign = [0.0, 0.3, 1.0][:Q], [0.3 * rr, 0.45 * rr, 0.2 * rr][:Q], [-1, 2, 0][:Q]
    res.set_queries(q_t0, q_r, q_ign)
    n, n_alloc = 37, 40
    tab = row_query = None
    parent_id = np.arange(n, dtype=np.int32)
    if Q > 1:
        tab = env.alloc_table(256, n_queries=Q)
        seeds = np.zeros((F, n))
        seeds[:dim] = 0.5 + np.arange(n)[None, :] * 0.01 + np.arange(dim)[:, None]  # distinct lattice states
        row_query = (np.arange(n) % Q).astype(np.int32)
        fr0 = m.TableFrontier(env, n)
        assert tab.seed(seeds, frontier=fr0, query=row_query) == n  # node k = seed k
        fr0.free()
    parent_id[[4, 20]] = -1

    # ---- parents and lists
    pst = np.zeros((F, n_alloc))
    pst[:dim, :n] = rng.uniform(2.0, 6.0, size=(dim, n))
    order = CM.order_of(control)
    if order >= 2:
        pst[dim:2 * dim, :n] = rng.uniform(-0.5, 0.5, size=(dim, n))
    # (the check applies no dynamic limits: within dt = 1 an acc of 1.5 moves an edge by up to 0.75 m and a jerk of 3 by up
    # to 0.5 m, against pair radii of about 0.2 .. 0.8 m)
    if order >= 3:
        pst[2 * dim:3 * dim, :n] = rng.uniform(-1.5, 1.5, size=(dim, n))
    if order >= 4:
        pst[3 * dim:4 * dim, :n] = rng.uniform(-3.0, 3.0, size=(dim, n))
    pst[F - 1, :n] = (np.arange(n) % 7) * dt  # differing parent times; tp = 6: past the horizon
    count = rng.integers(0, min(S, nU) + 1, size=n_alloc).astype(np.int32)
    count[:3] = [min(S, nU), 0, 1]
    N = n_alloc * S
    live = (np.arange(S)[None, :] < count[:, None]).ravel()
    live[n * S:] = False
    action = np.frombuffer(b"\xab" * (4 * N), np.int32).copy()
    cost = np.frombuffer(b"\xab" * (8 * N), np.float64).copy()
    action[live] = rng.integers(0, nU, size=int(live.sum()))
    cost[live] = rng.choice([0.5, 1.0, 2.0, np.inf], p=[0.3, 0.3, 0.3, 0.1], size=int(live.sum()))
    L = m.Lists(env, n_alloc, nU, want_state=False, stride=S)
    L.count.upload(count)
    L.action.upload(action)
    L.cost.upload(cost)
    fr = m.TableFrontier(env, n_alloc)
    fr.id.upload(np.concatenate([parent_id, np.full(n_alloc - n, 0, np.int32)]))
    fr.state.upload(pst)
    d_hit = upload(env, m, np.full(N, PAT64, np.int64))
    d_nb = upload(env, m, np.array([5], np.int64))

    # ---- the edges' positions from the device's own sampler: one chain of one primitive per entry, sampled at the
    # s = tl_i - tp of its row's instants (tp is a multiple of dt = 1, so s <= dt exactly and the sampler's clamp is idle)
    inst, times = [], np.zeros((n * S, 8))
    for k in range(n):
        q = 0 if row_query is None else int(row_query[k])
        tp = np.float64(pst[F - 1, k])
        ii = RM.instants(step, n_steps, q_t0[q], tp, tp + np.float64(dt))
        inst.append(ii)
        assert len(ii) <= 8
        for j in range(S):
            times[k * S + j, :len(ii)] = (ii.astype(np.float64) * np.float64(step) - np.float64(q_t0[q])) - tp
    e_starts = np.repeat(pst[:, :n], S, axis=1)
    e_starts[F - 1] = 0.0
    e_act = np.where(live[:n * S] & (action[:n * S] >= 0) & (action[:n * S] < nU), action[:n * S], 0).astype(np.int32)
    smp = env.traj_sample(e_starts, e_act.reshape(1, -1), times=times)["samples"]

    def edge_pos(k, j, i, s):
        c = int(np.nonzero(inst[k] == i)[0][0])
        assert times[k * S + j, c] == s
        return smp[:dim, k * S + j, c]

    want_cost, want_hit, want_nb, looked = RM.check(count[:n], action[:n * S], cost[:n * S], S, parent_id, pst[F - 1, :n], dt, nU,
                                                    step, n_steps, table, (q_t0, q_r, q_ign), edge_pos, row_query)
    if order >= 3:
        # ---- the sampler at this order against the polynomial in exact rationals: 2^-50 * sum |term| (five terms of at
        # most four rounded operations each, four rounded additions)
        rows = np.nonzero(looked)[0]
        exact, mag = exact_positions(e_starts[:, rows], np.asarray(U), e_act[rows], times[rows], dim, order)
        worst = Fraction(0)
        for d in range(dim):
            for r, e in enumerate(rows):
                for c in range(times.shape[1]):
                    err = abs(Fraction(float(smp[d, e, c])) - exact[d, r, c])
                    assert err <= mag[d, r, c] / 2 ** 50, (d, e, c, float(err), float(mag[d, r, c]))
                    worst = max(worst, err / mag[d, r, c] if mag[d, r, c] else worst)
        print("sampler vs exact polynomial, order %d: %d entries, worst error %.3g of sum |term|" % (order, len(rows), float(worst)))
        # ---- the higher-order rows decide hits: with them zeroed in the sampler's parents, entries change their hit
        for name, lo in (("acc", 2 * dim),) + ((("jrk", 3 * dim),) if order >= 4 else ()):
            z_starts = e_starts.copy()
            z_starts[lo:lo + dim] = 0.0
            z_smp = env.traj_sample(z_starts, e_act.reshape(1, -1), times=times)["samples"]
            z_pos = lambda k, j, i, s_: z_smp[:dim, k * S + j, int(np.nonzero(inst[k] == i)[0][0])]
            _, z_hit, _, z_looked = RM.check(count[:n], action[:n * S], cost[:n * S], S, parent_id, pst[F - 1, :n], dt, nU,
                                             step, n_steps, table, (q_t0, q_r, q_ign), z_pos, row_query)
            changed = int((z_hit[looked] != want_hit[looked]).sum())
            print("%s rows zeroed: %d of %d looked-at entries change their hit" % (name, changed, looked.sum()))
            assert np.array_equal(z_looked, looked) and changed >= MIN_SENSITIVE, (name, changed)
    res.check(fr, L, n, table=tab, hit=d_hit, n_blocked=d_nb)
    env.synchronize()
    got_hit, got_cost = d_hit.download(np.int64, (N,)), L.cost.download(np.float64, (N,))
    frac = want_nb / max(int(looked.sum()), 1)
    kinds = {("real" if h >= 0 else int(h)) for h in want_hit[looked]}
    print("B %d S %d: looked %d blocked %d (%.2f) kinds %s" % (B, S, looked.sum(), want_nb, frac, sorted(map(str, kinds))))
    assert np.array_equal(got_hit[:n * S], want_hit), np.nonzero(got_hit[:n * S] != want_hit)[0][:8]
    assert np.all(got_hit[n * S:] == PAT64)                              # rows past n_nodes
    assert np.array_equal(bits(got_cost[:n * S]), bits(want_cost))       # +inf where blocked, every other byte kept
    assert np.array_equal(bits(got_cost[n * S:]), bits(cost[n * S:]))
    assert np.array_equal(L.action.download(np.int32, (N,)), action) and np.array_equal(L.count.download(np.int32, (n_alloc,)), count)
    assert int(d_nb.download(np.int64, (1,))[0]) == 5 + want_nb
    assert 0.10 <= frac <= 0.90, frac
    assert kinds == {"real", -1, -2}, kinds  # entries without a conflict, real hits and entries past the horizon
    # a second call: the blocked entries are +inf now and nothing new is blocked
    res.check(fr, L, n, table=tab, hit=d_hit, n_blocked=d_nb)
    env.synchronize()
    assert int(d_nb.download(np.int64, (1,))[0]) == 5 + want_nb and np.all(d_hit.download(np.int64, (N,))[:n * S] == -1)
    for b in (d_hit, d_nb, fr, L, res) + ((tab,) if tab is not None else ()):
        b.free()
    env.close()


def test_poly_fill_is_the_samplers_positions(engine):
    m = engine
    env = plain_env(m, 2, m.ACC, m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    rng = np.random.default_rng(3)
    K, w = 6, 4
    wp = rng.uniform(1.0, 7.0, size=(2, w, K))
    poly = env.solve_traj(wp, v=1.0)
    step, t0 = 0.3, np.array([0.0, 0.4, -0.2, 1.0, 0.0, 2.5])
    res = env.alloc_reservations(poly, step, t0=t0, radius=0.3, park=False)
    tab = res.positions()
    n = res.n_steps
    times = (np.arange(n)[None, :] * np.float64(step)) - t0[:, None]
    smp = poly.sample(times=times)["samples"]
    total = poly.info()["total_time"]
    assert n == int(np.ceil((t0 + total).max() / step)) + 1
    for b in range(K):
        assert np.array_equal(bits(tab["pos"][:, :, b]), bits(smp[:2, b, :].T)), b
        assert np.array_equal(tab["active"][:, b] != 0, (times[b] >= 0) & (times[b] <= total[b]))
    res.free()
    poly.free()
    env.close()


# ------------------------------------------------------------------------------------------------------ time keys
def folded(host, F):
    h = host["hash"].copy()
    t = host["state"][F - 1]
    cnt = np.repeat(host["count"], host["stride"])
    livee = (np.arange(len(h)) % host["stride"]) < cnt
    for e in np.nonzero(livee)[0]:
        h[e] = RM.time_key(h[e], t[e])
    return dict(host, hash=h)


@pytest.mark.parametrize("Q,slots_log2", [(1, 0), (1, 12), (3, 11)])
def test_time_keys_equal_the_prefolded_table(engine, Q, slots_log2):
    """relax on (hash, t) lists with time keys on == the plain table (and tests/table_model.py, one query) on lists whose
    hash row the host folded; slots_log2 leaves little room: long probe chains."""
    m = engine
    env, start, _ = corridor_env(m)
    F = env.n_fields
    rng, pool, host, parent_id, parent_g = hand_case(seed=23, n=120, S=40)
    n, S = 120, 40
    # few hashes, times on the 0.1 lattice and half-way between (the rounding half case), some negative
    live = (np.arange(S)[None, :] < host["count"][:, None]).ravel()
    host["hash"] = np.where(live, pool[:200][host["hash"] % np.uint64(200)], host["hash"])
    host["state"][F - 1] = np.where(live, rng.integers(-4, 12, size=n * S) * 0.05, np.nan)
    pre = folded(host, F)
    assert len(set(pre["hash"][live].tolist())) > 2 * len(set(host["hash"][live].tolist()))  # one state at many times
    cap = 4000
    if Q == 1:
        parent_id = np.where(parent_id >= 0, 0, -1).astype(np.int32)
    tabs = []
    for keys in (True, False):
        tab = env.alloc_table(cap, slots_log2=slots_log2, n_queries=Q)
        if keys:
            tab.set_time_keys(True)
        fr = m.TableFrontier(env, n * S)
        if Q > 1:
            seeds = np.zeros((F, Q))
            seeds[0] = np.arange(Q)
            assert tab.seed(seeds, frontier=fr, query=np.arange(Q, dtype=np.int32)) == Q
            pid = np.where(parent_id >= 0, np.arange(n) % Q, -1).astype(np.int32)
        else:
            assert tab.seed(np.zeros(F), frontier=fr) == 1
            pid = parent_id
        lists = upload_lists(m, env, host if keys else pre)
        d_pid, d_pg = upload(env, m, pid), upload(env, m, parent_g)
        cnt = tab.relax(lists, d_pid, d_pg, frontier=fr)
        tabs.append((tab.download(), fr.download(cnt)))
        if keys and Q == 1:
            model = TableModel(F)
            model.seed(np.zeros((F, 1)), np.array([tabs[0][0]["hash"][0]], np.uint64))
            want_fr, _ = model.relax(pre, pid, parent_g)
            assert_frontier_equal(tabs[0][1], want_fr, "model")
            # find compares keys
            some = np.nonzero(live)[0][:50]
            ids = tab.find(pre["hash"][some])
            assert (ids >= 0).sum() > 10 and np.array_equal(tabs[0][0]["hash"][ids[ids >= 0]], pre["hash"][some][ids >= 0])
            assert np.array_equal(m.search.time_key(host["hash"][some], host["state"][F - 1][some]), pre["hash"][some])
            # refused: the switch on a table with nodes, a rebase of a table with time keys
            with pytest.raises(m._abi.MplxError) as e:
                tab.set_time_keys(False)
            assert e.value.code == m._abi.ERR_STATE
            with pytest.raises(m._abi.MplxError) as e:
                tab.rebase(root=-1, check_edges=False, frontier=fr)
            assert e.value.code == m._abi.ERR_STATE
            tab.clear()
            tab.set_time_keys(False)
        for b in (lists, d_pid, d_pg, fr, tab):
            b.free()
    (a, fa), (b, fb) = tabs
    assert a["n_nodes"] == b["n_nodes"] > 500
    # the seeds' keys differ (a seed's key folds its own t = 0); everything from the relax on is the same
    for k in ("pred", "pred_action", "query"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["hash"][Q:], b["hash"][Q:]) and np.array_equal(bits(a["g"]), bits(b["g"]))
    assert_frontier_equal(fa, fb, "time keys on / pre-folded")
    env.close()


def test_seed_with_time_keys(engine):
    m = engine
    env, start, _ = corridor_env(m)
    F = env.n_fields
    st = np.zeros((F, 5))
    st[0] = [1.0, 1.0, 1.0, 2.0, 1.0]
    st[F - 1] = [0.0, 0.05, 0.3, 0.3, 0.04]  # 0.05 rounds away from zero: its own node; 0.04 rounds to t = 0's
    plain, keyed = env.alloc_table(64), env.alloc_table(64)
    keyed.set_time_keys(True)
    fp, fk = m.TableFrontier(env, 8), m.TableFrontier(env, 8)
    assert plain.seed(st, frontier=fp) == 2 and keyed.seed(st, frontier=fk) == 4
    hp, hk = plain.download()["hash"], keyed.download()["hash"]
    assert hk.tolist() == [RM.time_key(hp[0], 0.0), RM.time_key(hp[0], 0.05), RM.time_key(hp[0], 0.3), RM.time_key(hp[1], 0.3)]
    for b in (fp, fk, plain, keyed):
        b.free()
    env.close()


# ------------------------------------------------------------------------------------- the search among reservations
STEP, RADIUS = 0.25, 0.4


def test_search_avoids_what_conflicts_reports(engine):
    """Robot 1 plans the corridor's way back against robot 0's plan.  Put in one set with it, conflicts() at the same
    step, radii and t0 reports nothing for robot 1 within its own trajectory (GONE for it), and the positions conflicts
    samples along its path are the positions the check evaluated: an edge's one-primitive chain sampled at
    s = tl_i - tp gives the same bits as the whole chain sampled at tl_i."""
    m = engine
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    solo = env.search_many(starts[:, [0, 2]], goals[[0, 2]], capacity=1 << 15, max_frontier=4096)
    assert all(solo.found)
    before = solo.conflicts(STEP, radius=RADIUS, park=False)
    print("independent plans:", before.first_step, before.min_dist)
    assert (before.first_step >= 0).all()
    p0 = solo.path(0)
    res = env.alloc_reservations((p0[0].reshape(-1, 1), p0[1].reshape(-1, 1)), STEP, n_steps=int(120 / STEP), radius=RADIUS, park=False)
    r1 = env.search(starts[:, 2], goals[2], capacity=1 << 18, max_frontier=4096, avoid=res, t0=0.0, radius=RADIUS)
    print(r1, "solo cost", solo.cost)
    assert r1.found and r1.cost >= solo.cost[1]
    with pytest.raises(RuntimeError):
        r1.replan()
    p1 = r1.path()
    H = max(len(p0[1]), len(p1[1]))
    st = np.stack([p0[0], p1[0]], axis=1)
    ac = np.full((H, 2), -1, np.int32)
    ac[:len(p0[1]), 0], ac[:len(p1[1]), 1] = p0[1], p1[1]
    n1 = int(len(p1[1]) * 1.0 / STEP) + 1  # the instants within robot 1's trajectory
    after = env.traj_conflicts(st, ac, STEP, n_steps=n1, radius=RADIUS, park=False, want_pairs=True)
    assert after.first_step[1] == -1 and after.pairs[1, 0] == -1 and after.min_dist[1] >= 2 * RADIUS
    # the bits: whole chain at tl_i against the edge that holds tl_i at s = tl_i - tp
    info = env.traj_info(p1[0], p1[1].reshape(-1, 1), want_states=True)
    ti = np.arange(n1) * np.float64(STEP)
    whole = env.traj_sample(p1[0], p1[1].reshape(-1, 1), times=ti)["samples"][:2, 0, :]
    seg = np.minimum(np.maximum(np.ceil(ti).astype(int) - 1, 0), len(p1[1]) - 1)  # sample's segment: tau <= taus[id + 1] first
    e_st = info["seg_state"][:, seg, 0].copy()
    tp = e_st[-1].copy()
    e_st[-1] = 0.0
    edge = env.traj_sample(e_st, p1[1][seg].reshape(1, -1), times=(ti - tp).reshape(-1, 1))["samples"][:2, :, 0]
    assert np.array_equal(bits(whole), bits(edge))
    # ... and the check itself as the probe: robot 1's own path reserved on a clock of 0.3 with t0 = 0.05 (no instant
    # falls on a chain state), radii 1e-100 and 0.  Every edge of the path is then blocked AT ITS FIRST INSTANT iff the
    # position the check evaluates there has the bits of the position conflicts() samples: d2 == 0 < 1e-200, while one
    # ulp of difference gives d2 ~ 1e-32
    own = env.alloc_reservations((p1[0].reshape(-1, 1), p1[1].reshape(-1, 1)), 0.3, n_steps=400, t0=[0.05], radius=0.0)
    own.set_queries(0.05, 1e-100)
    ne = len(p1[1])
    L = m.Lists(env, ne, 9, want_state=False, stride=1)
    L.count.upload(np.ones(ne, np.int32))
    L.action.upload(p1[1].astype(np.int32))
    L.cost.upload(np.ones(ne))
    fr = m.TableFrontier(env, ne)
    fr.id.upload(np.zeros(ne, np.int32))
    fr.state.upload(np.ascontiguousarray(info["seg_state"][:, :ne, 0]))
    d_hit = upload(env, m, np.zeros(ne, np.int64))
    own.check(fr, L, ne, hit=d_hit)
    env.synchronize()
    first = [int(RM.instants(0.3, 400, 0.05, float(k), float(k) + 1.0)[0]) for k in range(ne)]
    assert d_hit.download(np.int64, (ne,)).tolist() == [i << 32 for i in first]
    assert all(np.float64(i) * 0.3 - 0.05 > k for k, i in enumerate(first))  # s > 0: not the chain state itself
    for b in (d_hit, fr, L, own):
        b.free()
    # a start with t != 0 together with avoid
    bad = starts[:, 2].copy()
    bad[-1] = 1.0
    with pytest.raises(ValueError):
        env.search(bad, goals[2], avoid=res, radius=RADIUS)
    for b in (r1, solo, res):
        b.free()
    env.close()


def test_two_robots_swap_ends(engine):
    m = engine
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    starts, goals = starts[:, [0, 2]], goals[[0, 2]]
    kw = dict(capacity=1 << 18, max_frontier=4096, n_steps=int(160 / STEP))
    solo = env.search_many(starts, goals, capacity=1 << 15, max_frontier=4096)
    assert (solo.conflicts(STEP, radius=RADIUS).first_step >= 0).all()
    out = m.search.plan_prioritised(env, starts, goals, STEP, RADIUS, delays=(0.0, 2.0, 4.0, 8.0), **kw)
    print(out["status"], out["t0"], out["cost"], out["conflicts"].first_step, out["conflicts"].min_dist)
    assert out["status"] == [m.search.FOUND] * 2
    assert not out["conflicts"].charged.any()
    # the first robot met no reservation: its solo plan
    assert out["cost"][0] == solo.cost[0] and out["t0"][0] == 0.0
    # without time keys and without delays: recorded, and only held to "time keys are no better off without"
    keyed = m.search.plan_prioritised(env, starts, goals, STEP, RADIUS, delays=(0.0,), **kw)
    p0 = solo.path(0)
    res = env.alloc_reservations((p0[0].reshape(-1, 1), p0[1].reshape(-1, 1)), STEP, n_steps=kw["n_steps"], radius=RADIUS)
    flat = env.search(starts[:, 1], goals[1], capacity=1 << 18, max_frontier=4096, avoid=res, radius=RADIUS, time_keys=False)
    print("delays=(0,): time keys %s cost %r; without %s cost %r" % (keyed["status"][1], keyed["cost"][1], flat.status, flat.cost))
    assert keyed["cost"][1] <= flat.cost
    for b in (flat, res, solo):
        b.free()
    env.close()


def crossing_env(m):
    """Two one-cell lanes that cross in the middle of a 33 x 33 map of 1 m cells, everything else occupied: robot 0 drives
    west to east, robot 1 south to north, both 14 m from the crossing -- there is no way round, only another time."""
    n = 33
    cells = np.full((n, n), 100, np.int8)  # [y][x]
    cells[16, :] = 0
    cells[:, 16] = 0
    env = m.EnvMap(2)
    env.setMap([0.0, 0.0], [n, n], cells.ravel(), 1.0)
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    wp = lambda p: m.Waypoint(2, m.ACC, pos=p).to_row()
    starts = np.stack([wp([2.5, 16.5]), wp([16.5, 2.5])], axis=1)
    goals = np.stack([wp([30.5, 16.5]), wp([16.5, 30.5])])
    return env, starts, goals


def test_crossing_needs_the_clock(engine):
    """The lanes leave no detour, so the robot that yields can only pass the crossing at another time: later through a
    start delay, or by another speed profile.  Recorded on an MI355X: alone both cost 290.5 over 29 primitives and meet
    at the crossing at instant 59 (distance 0); prioritised, the second robot keeps delay 0 and its 29 primitives and
    pays 291.0 for a profile that passes 0.71 m from the first.  With delays=(0,) it finds that same 291.0 with time keys
    and without: here the slower approach is already another lattice state (its velocity differs), so the time in the key
    is not what makes the difference on this map; the test holds time keys to "no worse", as far as it can be held."""
    m = engine
    env, starts, goals = crossing_env(m)
    R = 0.3
    solo = env.search_many(starts, goals, capacity=1 << 15, max_frontier=4096)
    assert all(solo.found) and solo.cost[0] == solo.cost[1]
    ind = solo.conflicts(STEP, radius=R)
    print("independent:", ind.first_step, ind.min_dist)
    assert (ind.first_step >= 0).all() and ind.min_dist[0] == 0.0  # both at the crossing at the same instant
    kw = dict(capacity=1 << 17, max_frontier=4096, n_steps=int(120 / STEP))
    out = m.search.plan_prioritised(env, starts, goals, STEP, R, delays=(0.0, 2.0, 4.0, 8.0), **kw)
    print("prioritised:", out["status"], out["t0"], out["cost"], out["conflicts"].first_step, out["conflicts"].min_dist)
    assert out["status"] == [m.search.FOUND] * 2 and not out["conflicts"].charged.any()
    assert out["conflicts"].min_dist[1] >= 2 * R
    assert out["cost"][0] == solo.cost[0] and out["t0"][0] == 0.0 and np.array_equal(out["paths"][0][1], solo.path(0)[1])
    end = lambda o, r: o["t0"][r] + len(o["paths"][r][1]) * 1.0
    yielded = lambda o, r: end(o, r) > len(solo.path(r)[1]) * 1.0 or o["cost"][r] > solo.cost[r]
    assert yielded(out, 1)  # robot 1 arrives later than it would alone, or pays for another speed profile
    # the other order: robot 0 yields
    rev = m.search.plan_prioritised(env, starts, goals, STEP, R, order=[1, 0], delays=(0.0, 2.0, 4.0, 8.0), **kw)
    assert not rev["conflicts"].charged.any() and rev["cost"][1] == solo.cost[1] and yielded(rev, 0)
    # no delays: with time keys against without.  Recorded; held only to "time keys are no worse"
    keyed = m.search.plan_prioritised(env, starts, goals, STEP, R, delays=(0.0,), **kw)
    p0 = solo.path(0)
    res = env.alloc_reservations((p0[0].reshape(-1, 1), p0[1].reshape(-1, 1)), STEP, n_steps=kw["n_steps"], radius=R)
    flat = env.search(starts[:, 1], goals[1], capacity=1 << 17, max_frontier=4096, avoid=res, radius=R, time_keys=False)
    print("delays=(0,): time keys %s cost %r conflicts %s; without %s cost %r" % (
        keyed["status"][1], keyed["cost"][1], keyed["conflicts"].first_step, flat.status, flat.cost))
    assert keyed["cost"][1] <= flat.cost
    for b in (flat, res, solo):
        b.free()
    env.close()


def test_search_without_avoid_is_unchanged(engine):
    """The corridor search of tests/test_gpu_open.py and the three queries of tests/test_gpu_multi.py without `avoid`: the
    status, cost, rounds, expansions, node count and path recorded from the parent commit on an MI355X (the two builds
    side by side printed the same lines), before and after a search among reservations on the same EnvMap."""
    # parent: search      FOUND 351.5 rounds 35 expanded 6073 nodes 10102, path 7 7 4 5 4 3 4 ... (35 primitives)
    #         search_many FOUND x 3, costs 351.5 351.75 352.0, rounds 35 35 35, expanded 6073 6117 5949, 35 relax calls, 30239 nodes
    path0 = [7, 7, 4, 5, 4, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4]
    m = engine
    env, start, goal = corridor_env(m)
    starts, goals = corridor_queries(m)
    a = env.search(start, goal, capacity=1 << 15, max_frontier=4096)
    ma = env.search_many(starts, goals, capacity=1 << 15, max_frontier=4096)
    assert (a.status, a.cost, a.rounds, a.expanded, a.table.stats()) == (m.search.FOUND, 351.5, 35, 6073, (10102, 0))
    assert a.path()[1].tolist() == path0 and ma.path(0)[1].tolist() == path0
    assert (ma.status, ma.cost, ma.rounds, ma.expanded) == ([m.search.FOUND] * 3, [351.5, 351.75, 352.0], [35] * 3, [6073, 6117, 5949])
    assert ma.total_rounds == 35 and ma.table.stats() == (30239, 0)
    p = a.path()
    res = env.alloc_reservations((p[0].reshape(-1, 1), p[1].reshape(-1, 1)), STEP, n_steps=400, radius=RADIUS)
    mid = env.search(starts[:, 2], goals[2], capacity=1 << 18, max_frontier=4096, avoid=res, radius=RADIUS)
    b = env.search(start, goal, capacity=1 << 15, max_frontier=4096)
    mb = env.search_many(starts, goals, capacity=1 << 15, max_frontier=4096)
    assert (a.status, a.cost, a.rounds, a.expanded) == (b.status, b.cost, b.rounds, b.expanded)
    assert np.array_equal(a.path()[1], b.path()[1]) and a.table.stats() == b.table.stats()
    assert (ma.status, ma.cost, ma.rounds, ma.expanded) == (mb.status, mb.cost, mb.rounds, mb.expanded) and ma.cost[0] == 351.5
    for x in (a, b, ma, mb, mid, res):
        x.free()
    env.close()


def test_errors_and_no_ops(engine):
    m = engine
    A = m._abi
    env, start, goal = corridor_env(m)
    F = env.n_fields

    def code(fn):
        with pytest.raises(A.MplxError) as e:
            fn()
        return e.value.code

    st = np.zeros((F, 2))
    st[0] = [1.0, 3.0]
    ac = np.zeros((3, 2), np.int32)
    for kw in (dict(step=0.0), dict(step=np.inf), dict(n_steps=0), dict(n_steps=1 << 30)):
        args = dict(step=0.25, n_steps=8, radius=0.3)
        args.update(kw)
        assert code(lambda: env.alloc_reservations((st, ac), **args)) == A.ERR_ARG, kw  # (2^30 instants: over the cap)
    res = env.alloc_reservations((st, ac), 0.25, n_steps=40, radius=0.3)
    L = m.Lists(env, 4, 9, want_state=False, stride=9)
    L.count.upload(np.zeros(4, np.int32))
    fr = m.TableFrontier(env, 4)
    fr.id.upload(np.zeros(4, np.int32))
    fr.state.upload(np.zeros((F, 4)))
    assert code(lambda: res.check(fr, L, 4)) == A.ERR_STATE                      # no queries yet
    for t0, r in ((-1.0, 0.3), (np.nan, 0.3), (0.0, -0.1), (0.0, np.inf)):
        assert code(lambda: res.set_queries(t0, r)) == A.ERR_ARG
    res.set_queries([0.0, 1.0], 0.3)
    assert code(lambda: res.check(fr, L, 4)) == A.ERR_ARG                        # two queries, no table
    tab3 = env.alloc_table(64, n_queries=3)
    assert code(lambda: res.check(fr, L, 4, table=tab3)) == A.ERR_ARG            # two queries, a table of three
    res.set_queries(0.0, 0.3)
    assert code(lambda: res.check(fr, L, -1)) == A.ERR_ARG
    assert code(lambda: res.check(fr, L, 5)) == A.ERR_ARG                        # parent_stride < n_nodes
    no_cost = L.c_struct()
    no_cost.cost = None
    raw = lambda *a: A.check(env._ctx, A.lib().mplx_reserve_check_device(*a))
    assert code(lambda: raw(res._res, None, C.byref(no_cost), 4, fr.id.ptr, fr.ptr, 4, None, None)) == A.ERR_ARG
    assert code(lambda: raw(res._res, None, None, 4, fr.id.ptr, fr.ptr, 4, None, None)) == A.ERR_ARG
    assert code(lambda: raw(res._res, None, C.byref(L.c_struct()), 4, None, fr.ptr, 4, None, None)) == A.ERR_ARG
    assert code(lambda: A.check(env._ctx, A.lib().mplx_reserve_set_queries(res._res, 0, None, None, None))) == A.ERR_ARG
    assert code(lambda: A.check(env._ctx, A.lib().mplx_reserve_fill_traj(res._res, env._ctx, None, None))) == A.ERR_ARG
    other = m.EnvMap(2)
    tab_other = other.alloc_table(64)
    assert code(lambda: res.check(fr, L, 4, table=tab_other)) == A.ERR_ARG        # a table of another context
    tab_other.free()
    other.close()
    res.check(fr, L, 0)                                                          # n_nodes == 0
    res.check(fr, L, 4)                                                          # empty rows
    empty = env.alloc_reservations((np.zeros((F, 0)), np.zeros((1, 0), np.int32)), 0.25, n_steps=40, radius=0.3)  # K == 0
    empty.set_queries(0.0, 0.3)
    L.count.upload(np.array([1, 0, 0, 0], np.int32))
    L.action.upload(np.zeros(36, np.int32))
    L.cost.upload(np.ones(36))
    d_hit = upload(env, m, np.full(36, 7, np.int64))
    empty.check(fr, L, 4, hit=d_hit)
    env.synchronize()
    assert np.all(d_hit.download(np.int64, (36,)) == -1) and np.all(L.cost.download(np.float64, (36,)) == 1.0)
    fresh = C_create(m, env)
    assert code(lambda: A.check(env._ctx, A.lib().mplx_reserve_positions(fresh, None, None, None, None, None, None))) == A.ERR_STATE
    s = L.c_struct()
    assert code(lambda: A.check(env._ctx, A.lib().mplx_reserve_check_device(fresh, None, C.byref(s), 4, fr.id.ptr, fr.ptr, 4, None, None))) == A.ERR_STATE
    A.lib().mplx_reserve_destroy(fresh)
    for b in (d_hit, empty, tab3, fr, L, res):
        b.free()
    env.close()


def C_create(m, env):
    r = C.c_void_p()
    m._abi.check(env._ctx, m._abi.lib().mplx_reserve_create(env._ctx, C.byref(r)))
    return r
