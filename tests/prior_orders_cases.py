"""The worlds and priors of tests/test_prior_orders.py (conditions on the model alone, no GPU) and of
tests/test_gpu_prior_orders.py (the device against the model): a non-cube map with a few per cent of occupied cells and a
hand-made potential map, and Q priors per call from a seeded generator with the hand-made ones planted among them.  Test
infrastructure: numpy and tests/prior_model.py, nothing shared with the engine."""
import itertools

import numpy as np

import prior_model as PM

VEL, ACC, JRK, SNP, YAW = 0x01, 0x03, 0x07, 0x0f, 0x10
CONTROLS = {"VEL": VEL, "ACC": ACC, "JRK": JRK, "SNP": SNP, "VELxYAW": VEL | YAW, "ACCxYAW": ACC | YAW, "JRKxYAW": JRK | YAW,
            "SNPxYAW": SNP | YAW}
DIMS = {2: [75, 43], 3: [53, 37, 29]}  # the non-cubes of tests/test_gpu_map_geometry.py
ORIGIN = {2: [-9.4, -5.3], 3: [-6.6, -4.7, -3.6]}
RES, VMAX, W = 0.25, 2.0, 10.0
POT_W, GRAD_W = 0.5, 0.25
SEARCHING = {2: JRK, 3: ACC}  # the searching control is fixed per dimension; yaw stays out of it
SEED = 20260  # the generator's seed: the conditions of check_table_case() hold with it on the model alone, for every case below
N_PLANTED = {2: 10, 3: 12}


def centre(D, cell):
    return [ORIGIN[D][i] + (cell[i] + 0.5) * RES for i in range(D)]


def index(D, cell):
    d = DIMS[D]
    return cell[0] + d[0] * cell[1] + (d[0] * d[1] * cell[2] if D == 3 else 0)


# the planted priors start at the centres of these cells; the cell two cells up the x axis of THROUGH is occupied
THROUGH = {2: (30, 20), 3: (20, 18, 14)}
LEAVE_LO = {2: [(1, 11), (40, 1)], 3: [(1, 9, 9), (30, 1, 20), (40, 30, 1)]}
LEAVE_HI = {2: [(73, 30), (12, 41)], 3: [(51, 25, 6), (11, 35, 11), (25, 12, 27)]}

_worlds = {}


def world(D):
    """(cells, pot): the int8 occupancy map (about 3 % at 100) and the potential map (0 on 40 % of the cells, 1 .. 99 on
    the rest, 100 on the obstacles); the lines the planted priors take are free but for the one cell THROUGH runs into."""
    if D not in _worlds:
        dims = DIMS[D]
        n = int(np.prod(dims))
        rng = np.random.default_rng(1000 + D)
        cells = np.zeros(n, np.int8)
        cells[rng.random(n) < 0.03] = 100
        for i in range(-1, 3):
            c = list(THROUGH[D])
            c[0] += i
            cells[index(D, c)] = 100 if i == 2 else 0
        for ax in range(D):
            for side, sign in ((LEAVE_LO, -1), (LEAVE_HI, 1)):
                for i in range(0, 2):
                    c = list(side[D][ax])
                    c[ax] += sign * i
                    cells[index(D, c)] = 0
        cells[index(D, [d // 2 for d in dims])] = 0  # (where the stationary prior stands)
        pot = rng.integers(1, 100, n).astype(np.int8)
        pot[rng.random(n) < 0.4] = 0
        pot[cells == 100] = 100
        _worlds[D] = (cells, pot)
    return _worlds[D]


def prior_u(D, control, scale=1.0):
    """The control table of the prior's planner: {-1, 0, 1}^D * scale, times {-0.5, 0, 0.5} in yaw with the yaw bit."""
    g = [np.array(u, dtype=np.float64) * scale for u in itertools.product([-1.0, 0.0, 1.0], repeat=D)]
    if control & YAW:
        g = [np.append(u, y) for u in g for y in (-0.5, 0.0, 0.5)]
    return np.array(g)


def u_index(U, D, vec, yaw=0.0):
    want = list(vec) + ([yaw] if U.shape[1] > D else [])
    for i, u in enumerate(U):
        if list(u) == want:
            return i
    raise KeyError(vec)


def make_priors(D, control, Q, H, seed=SEED, scale=1.0, planted=True):
    """(starts [4D+2][Q], actions [H][Q], U): random walks of 1 .. H actions from the middle third of the map with every
    derivative row, the yaw and (for every fifth) the time of the start state live, so that a row the order does not read
    is seen to be ignored; with planted=True (Q >= 12) the first queries are, in this order: an empty prior, a bad action
    in the middle, a prior that fills the horizon, one segment, a stationary prior, a prior through an occupied cell, one
    leaving across the low side of every axis, one leaving across the high side of every axis."""
    rng = np.random.default_rng(seed + 100 * D + control)
    U = prior_u(D, control, scale)
    nU, F = U.shape[0], 4 * D + 2
    starts, actions = np.zeros((F, Q)), np.full((H, Q), -1, np.int32)
    ext = [DIMS[D][i] * RES for i in range(D)]
    for q in range(Q):
        n = int(rng.integers(1, H + 1))
        actions[:n, q] = rng.integers(0, nU, n)
        for i in range(D):
            starts[i, q] = ORIGIN[D][i] + ext[i] * rng.uniform(1.0 / 3.0, 2.0 / 3.0)
        starts[D:2 * D, q] = rng.uniform(-0.8, 0.8, D)
        starts[2 * D:3 * D, q] = rng.uniform(-0.5, 0.5, D)
        starts[3 * D:4 * D, q] = rng.uniform(-0.3, 0.3, D)
        starts[4 * D, q] = rng.uniform(-3.0, 3.0)
        starts[4 * D + 1, q] = 1.7 if q % 5 == 4 else 0.0
    if not planted:
        return starts, actions, U
    assert Q >= N_PLANTED[D] and H >= 8
    zero = u_index(U, D, [0.0] * D)

    def still(q, cell):  # at rest in the centre of a cell
        starts[:4 * D, q] = 0.0
        starts[:D, q] = centre(D, cell)

    def unit(ax, sign):
        return u_index(U, D, [sign * scale if i == ax else 0.0 for i in range(D)])
    actions[0, 0] = -1                                   # 0: empty (the actions after the first -1 are never read)
    actions[1:4, 0] = 1
    actions[:, 1] = -1                                   # 1: a bad action in the middle
    actions[:8, 1] = rng.integers(0, nU, 8)
    actions[4, 1] = nU + 5
    actions[:, 2] = rng.integers(0, nU, H)               # 2: fills the horizon
    actions[1:, 3] = -1                                  # 3: one segment
    still(4, [d // 2 for d in DIMS[D]])                  # 4: stationary
    actions[:, 4] = zero
    still(5, THROUGH[D])                                 # 5: through the occupied cell two cells up the x axis
    actions[:, 5] = unit(0, 1.0)
    q = 6
    for side, sign in ((LEAVE_LO, -1.0), (LEAVE_HI, 1.0)):  # 6 ..: across the low, then the high side of every axis
        for ax in range(D):
            still(q, side[D][ax])
            actions[:, q] = unit(ax, sign)
            q += 1
    assert q == N_PLANTED[D]
    return starts, actions, U


def make_goals(D, Q, seed=SEED):
    """Goal rows [Q][4D+2] of the searching control: positions anywhere in the map, the other rows zero."""
    rng = np.random.default_rng(seed + 7 * D)
    rows = np.zeros((Q, 4 * D + 2))
    for i in range(D):
        rows[:, i] = ORIGIN[D][i] + DIMS[D][i] * RES * rng.uniform(0.05, 0.95, Q)
    return rows


def model_tables(D, control, pdt, dt, starts, actions, U, goals, v_max=VMAX, with_pot=True):
    cells, pot = world(D)
    out = []
    for q in range(actions.shape[1]):
        st = starts[:, q] if starts.shape[1] > 1 else starts[:, 0]
        out.append(PM.prior_table(D, control, U, pdt, st, actions[:, q], cells, DIMS[D], ORIGIN[D], RES, v_max, W, dt,
                                  pot=pot if with_pot else None, pot_w=POT_W, grad_w=GRAD_W, goal_row=goals[q],
                                  goal_hash=PM.lattice_hash(D, SEARCHING[D], goals[q])))
    return out


# ---- the table cases: every (D, prior control) with prior dt 0.3 under context dt 0.1, one with 0.5 under 0.3, two correcting --

Q_TABLE, H_TABLE = 65, 12
# find_segment guesses the segment of t_k as (int)(t_k / dt_prior) and corrects the guess against the accumulated segment ends.
# With 0.3 under 0.1 and 0.5 under 0.3 no guess of a step needs correcting (guess_low = guess_high = 0 in measure());
# these two pairs have guesses one too low (t_k has reached a segment end its quotient has not) and one too high.
CORRECTING = {(3, "JRK", 0.2, 0.2): "guess_low", (2, "ACC", 0.3, 0.2): "guess_high"}
TABLE_CASES = [(D, name, 0.3, 0.1) for D in (2, 3) for name in CONTROLS] + [(3, "ACCxYAW", 0.5, 0.3)] + sorted(CORRECTING)


def table_id(case):
    return "%dD-%s-%g-%g" % case


_tables = {}


def table_case(case):
    """(starts, actions, U, goals, want [Q]) of one table case; computed once."""
    if case not in _tables:
        D, name, pdt, dt = case
        starts, actions, U = make_priors(D, CONTROLS[name], Q_TABLE, H_TABLE)
        goals = make_goals(D, Q_TABLE)
        _tables[case] = (starts, actions, U, goals, model_tables(D, CONTROLS[name], pdt, dt, starts, actions, U, goals))
    return _tables[case]


def traverse_class(v_max, horizon, pdt, res):
    """The lane count mplx_open_set_priors_device picks for its traverse launch: B = ceil(v_max * horizon * pdt / res) + 1."""
    B = int(np.ceil(v_max * (horizon * pdt) / res)) + 1
    return (4 if B <= 64 else 16 if B <= 256 else 64), B


def measure(D, want, dt):
    """What the conditions are about, counted on the model's tables."""
    n_cells = int(np.prod(DIMS[D]))
    some = [w for w in want if w["n_steps"] > 0]
    m = {"non_empty": len(some),
         "finite": sum(1 for w in some if np.all(np.isfinite(w["togo"]))),
         "infinite": sum(1 for w in some if np.all(np.isinf(w["togo"])) and np.all(w["togo"] > 0)),
         "off_quotient": sum(1 for w in some for k, t in enumerate(w["steps_t"]) if int(t / dt) != k),
         "skipped": 0, "potential_terms": 0, "wrapped_inside": 0, "guess_low": 0, "guess_high": 0,
         "lengths": sorted({w["n_steps"] for w in want})}
    for w in some:
        taus = w["taus"]
        S, pdt = len(taus) - 1, taus[1]
        for t in w["steps_t"]:  # the guess of find_segment against the segment the model evaluates
            tau = min(t, w["T"])
            guess = min(int(tau / pdt), S - 1)
            seg = next(si for si in range(S) if taus[si] <= tau < taus[si + 1] or si == S - 1)
            m["guess_low"] += guess < seg
            m["guess_high"] += guess > seg
        prev = -1
        for (_, _, idx, outside, _, pv) in w["samples"]:
            if outside and 0 <= idx < n_cells:
                m["wrapped_inside"] += 1
            if idx == prev:
                m["skipped"] += 1
                continue
            prev = idx
            if pv != 0 and not outside:
                m["potential_terms"] += 1
    return m


def check_table_case(case):
    """The conditions on the inputs of a table case, on the model alone; returns the counts."""
    D, name, pdt, dt = case
    starts, actions, U, goals, want = table_case(case)
    m = measure(D, want, dt)
    assert 4 * m["finite"] >= m["non_empty"] and 10 * m["infinite"] >= m["non_empty"], (case, m)
    assert m["skipped"] >= 1 and m["potential_terms"] >= 1 and m["wrapped_inside"] >= 1, (case, m)
    if case in CORRECTING:
        assert m[CORRECTING[case]] >= 10, (case, m)
    else:
        assert m["off_quotient"] >= 100 and m["guess_low"] == m["guess_high"] == 0, (case, m)
    n_low = 6 + D
    assert want[0]["status"] == PM.EMPTY and want[0]["n_steps"] == 0
    assert want[1]["status"] == PM.BAD_ACTION and 3.5 * pdt < want[1]["T"] < 4.5 * pdt and want[1]["n_steps"] > 0
    assert len(want[2]["samples"]) > 0 and want[2]["status"] == 0 and actions[H_TABLE - 1, 2] >= 0
    assert want[3]["T"] == pdt and want[3]["n_steps"] == len([t for t in want[3]["steps_t"]]) >= 1
    # the stationary prior: every sample in one cell, so the skip carries the whole sum; finite unless that cell is occupied
    assert len({s[2] for s in want[4]["samples"]}) == 1 and len(want[4]["samples"]) > 2
    assert np.all(want[4]["pos"] == want[4]["pos"][0])
    # the prior through the wall: +inf, by an occupied sample that comes before any sample outside the map
    first = next(s for s in want[5]["samples"] if s[3] or s[4])
    assert np.all(np.isinf(want[5]["togo"])) and first[4] and not first[3]
    for q in range(6, N_PLANTED[D]):  # the leavers: +inf, by a sample outside that comes before any occupied one
        first = next(i for i, s in enumerate(want[q]["samples"]) if s[3] or s[4])
        assert want[q]["samples"][first][3] and np.all(np.isinf(want[q]["togo"])), (case, q)
        ax = (q - 6) % D
        p_end = want[q]["goal_row"][ax]
        assert (p_end < ORIGIN[D][ax]) if q < n_low else (p_end > ORIGIN[D][ax] + DIMS[D][ax] * RES), (case, q)
    assert traverse_class(VMAX, H_TABLE, pdt, RES)[0] == 4
    return m


# ---- further table cases: query counts, one shared start, the 16-lane traverse (all 3D with an ACC prior, 0.3 under 0.1) ------

QUERY_COUNTS = (1, 63, 64, 257)  # 257: one past a block of prior_build_kernel
LANES16_VMAX = 6.0               # B = ceil(6 * 12 * 0.3 / 0.25) + 1 = 88: in (64, 256]
_further = {}


def count_case(Q):
    """(starts, actions, U, goals, the query without a prior (-1: none), want [Q]) for a call of Q queries."""
    if Q not in _further:
        starts, actions, U = make_priors(3, ACC, Q, H_TABLE, seed=SEED + Q, planted=Q >= 12)
        goals = make_goals(3, Q, seed=SEED + Q)
        none = Q // 2 if Q > 1 else -1
        if none >= 0:
            actions[:, none] = -1
            starts[:, none] = 0.0  # (what set_prior_list sends for None)
        _further[Q] = (starts, actions, U, goals, none, model_tables(3, ACC, 0.3, 0.1, starts, actions, U, goals))
    return _further[Q]


def shared_start_case():
    """64 priors from one start state (n_starts == 1): (starts [14][1], actions, U, goals, want)."""
    if "shared" not in _further:
        starts, actions, U = make_priors(3, ACC, 64, H_TABLE, seed=SEED + 5, planted=False)
        starts = starts[:, 7:8].copy()
        goals = make_goals(3, 64, seed=SEED + 5)
        _further["shared"] = (starts, actions, U, goals, model_tables(3, ACC, 0.3, 0.1, starts, actions, U, goals))
    return _further["shared"]


def lanes16_case():
    """The priors of the 3D JRK table case under v_max = 6: 87 samples a prior at most, the 16-lane traverse."""
    if "lanes16" not in _further:
        starts, actions, U = make_priors(3, JRK, Q_TABLE, H_TABLE)
        goals = make_goals(3, Q_TABLE)
        _further["lanes16"] = (starts, actions, U, goals, model_tables(3, JRK, 0.3, 0.1, starts, actions, U, goals, v_max=LANES16_VMAX))
    return _further["lanes16"]


# ---- the push cases: 3D, an ACC prior under an ACC search (so a row can BE the prior's goal state), context dt 0.1 ------------

PUSH_PDT, PUSH_DT = 0.3, 0.1


def accumulated(dt, n):
    """t_0 = 0, t_{k+1} = t_k + dt: the times a search's nodes carry (0.7999999999999999 and its kin)."""
    out, t = [], 0.0
    for _ in range(n):
        out.append(t)
        t = t + dt
    return out


def _near(pri, k, j, rng):
    p = np.array(pri["pos"][min(max(k, 0), pri["n_steps"] - 1)], dtype=np.float64)
    return p + [0.3 + 0.01 * j, -0.2, 0.07 * (j % 5)] + rng.uniform(-0.02, 0.02, 3)


def push_case(which):
    """(goals [Q][14], starts, actions, U, pri [Q] (model tables or None), states [14][n], query [n], g [n]) of the push
    tests on the map without its potential map.  "three": query 0 a long prior, 1 none, 2 a short one; per query rows at
    t = 0, below and at a step boundary, at accumulated times whose quotient is not their step, at the last step of either
    prior, one step past either end, at k * dt (whose quotient may fall short of k), a negative and a NaN time, then the
    effective goal state itself and rows inside and outside the tolerance.  "many": 67 queries, every seventh without a
    prior, five rows each with the query ids interleaved: t = 0, the middle and the last step of the query's own prior,
    one step and six steps past its end."""
    D, control, dt = 3, ACC, PUSH_DT
    rng = np.random.default_rng(SEED + (1 if which == "three" else 2))
    acc = accumulated(dt, 64)
    if which == "three":
        s0, a0, U = make_priors(D, control, 48, H_TABLE, seed=SEED + 31, planted=False)
        g0 = make_goals(D, 48, seed=SEED + 31)
        t0 = model_tables(D, control, PUSH_PDT, dt, s0, a0, U, g0, with_pot=False)
        fin = [q for q in range(48) if t0[q]["n_steps"] and np.all(np.isfinite(t0[q]["togo"]))]
        long_q = max(fin, key=lambda q: (t0[q]["n_steps"], -q))
        short_q = next(q for q in fin if 9 <= t0[q]["n_steps"] <= 18)
        pick = [long_q, short_q, short_q]
        starts, actions, goals = s0[:, pick].copy(), a0[:, pick].copy(), g0[pick].copy()
        actions[:, 1] = -1
        pri = [t0[long_q], None, t0[short_q]]
        goals[2, :D] += 0.1  # (its own goal row: replaced by the prior's end all the same)
        pri[2] = dict(pri[2])
        ns0, ns2 = pri[0]["n_steps"], pri[2]["n_steps"]
        assert ns0 >= 24 and ns0 > ns2 + 3
        times = [0.0, 0.05, 0.1, acc[3], acc[8], 0.8, acc[ns2 - 1], acc[ns2], ns2 * dt, acc[ns0 - 1], acc[ns0], ns0 * dt, (ns0 + 1) * dt,
                 -1.0, float("nan")]
        assert int(acc[8] / dt) == 7 and acc[8] == 0.7999999999999999
        cols, query = [], []
        for q in range(3):
            for j, t in enumerate(times):
                s = np.zeros(14)
                s[:D] = _near(pri[0], int(t / dt) if t > 0 else 0, j, rng)
                s[13] = t
                cols.append(s)
                query.append(q)
            end = pri[q]["goal_row"] if pri[q] else goals[q]
            for j, d in enumerate([(0.0, 0.0, 0.0), (0.25, 0.0, 0.1), (0.0, -0.4, 0.0), (0.6, 0.0, 0.0)]):  # itself, in, in, out
                s = np.array(end, dtype=np.float64)
                s[:D] += d
                s[2 * D:] = 0.0
                s[13] = acc[5 + j]
                cols.append(s)
                query.append(q)
    else:
        Q = 67
        starts, actions, U = make_priors(D, control, Q, H_TABLE, seed=SEED + 67, planted=False)
        goals = make_goals(D, Q, seed=SEED + 67)
        for q in range(3, Q, 7):
            actions[:, q] = -1
        tabs = model_tables(D, control, PUSH_PDT, dt, starts, actions, U, goals, with_pot=False)
        pri = [t if t["n_steps"] else None for t in tabs]
        cols, query = [], []
        for j in range(5):
            for q in range(Q):
                ns = pri[q]["n_steps"] if pri[q] else 12
                k = (0, ns // 2, ns - 1, ns, ns + 5)[j]
                s = np.zeros(14)
                s[:D] = _near(pri[q], k, j, rng) if pri[q] else goals[q][:D] + rng.uniform(-2.0, 2.0, 3)
                s[D:2 * D] = rng.integers(-3, 4, 3) * 0.1
                s[13] = acc[k]
                cols.append(s)
                query.append(q)
    states = np.stack(cols, axis=1)
    query = np.array(query, dtype=np.int32)
    return goals, starts, actions, U, pri, states, query, 0.25 * np.arange(states.shape[1])


def push_models(O, case, MM):
    """(table, seeded frontier, guided open model, plain open model) of a push case on the models."""
    import open_model as OM
    goals, starts, actions, U, pri, states, query, g = case
    D, Q = 3, goals.shape[0]
    cells, _ = world(D)
    table = MM.MultiTableModel(14, Q)
    fr, _ = table.seed(states, [O.lattice_hash(D, SEARCHING[D], states[:, i]) for i in range(states.shape[1])], g, query=query)
    hashes = [O.lattice_hash(D, SEARCHING[D], r) for r in goals]
    eff = [pri[q]["goal_row"] if pri[q] else goals[q] for q in range(Q)]
    blocked = [OM.ray_blocked(cells, DIMS[D], ORIGIN[D], RES, eff[q][:D]) for q in range(Q)]
    model = PM.PriorMultiOpenModel(table, D, goals, hashes, W, VMAX, PUSH_DT, pri, tol_pos=0.5, blocked=blocked)
    plain = MM.MultiOpenModel(table, D, goals, hashes, W, VMAX, tol_pos=0.5,
                              blocked=[OM.ray_blocked(cells, DIMS[D], ORIGIN[D], RES, goals[q][:D]) for q in range(Q)])
    return table, fr, model, plain


def check_push_case(O, case, MM):
    """The prior moves at least a third of the keys, and only keys of guided queries; returns what push_models gave and
    the counts."""
    goals, starts, actions, U, pri, states, query, g = case
    table, fr, model, plain = push_models(O, case, MM)
    assert fr["count"] == states.shape[1] == table.n_nodes  # every row a node of its own
    model.push(fr, fr["count"], 1.0)
    plain.push(fr, fr["count"], 1.0)
    f, fl = model.arrays()
    f0, _ = plain.arrays()
    guided = np.array([pri[q] is not None for q in query])
    moved = f.view(np.uint64) != f0.view(np.uint64)
    assert 3 * int(moved.sum()) >= f.size and not np.any(moved[~guided]), (int(moved.sum()), f.size)
    n = {"rows": int(f.size), "moved": int(moved.sum()), "goal_bits": int(((fl & 2) > 0).sum()), "inf_keys": int(np.isinf(f).sum())}
    model.f, model.flags = {}, {}
    return table, fr, model, plain, n


# ---- the search cases ---------------------------------------------------------------------------------------------------------

S3_DIMS, S3_RES, S3_ORIGIN = [21, 17, 13], 0.5, [-5.25, -4.25, -3.25]
S3_STARTS = [(-4.0, 2.0, 0.0), (-4.0, 2.5, 0.5), (-3.5, 1.5, -0.5)]
S3_GOALS = [(4.0, 2.0, 0.0), (4.0, 1.5, -0.5), (3.5, 2.0, 1.0)]
S3_NONE = 1  # the query whose prior is replaced by None
S_W, S_VMAX, S3_GMAX = 10.0, 1.0, 150.0


def s3_cells():
    """A wall across the x axis with one window low in y: the straight line every heuristic follows is a dead end."""
    c = np.zeros(S3_DIMS[::-1], np.int8)  # [z][y][x]
    c[:, :, 10] = 100
    c[5:8, 2:5, 10] = 0
    return c.ravel()


def s3_u():
    return np.array(list(itertools.product([-1.0, 0.0, 1.0], repeat=3)))


def rows_of(points, F):
    r = np.zeros((len(points), F))
    for q, p in enumerate(points):
        r[q, :len(p)] = p
    return r


_s3 = {}


def s3_stage(O, MM, control, priors, delta, model_class=None, **kw):
    """One stage of the 3D two-stage search on the models: (table, open model, the output of MM.search_many, starts)."""
    key = (control, tuple(p is not None for p in priors), delta, model_class, tuple(sorted(kw.items())))
    if key not in _s3:
        from table_model import oracle_provider
        oenv = O.Env(3, control, s3_u(), s3_cells(), S3_DIMS, S3_ORIGIN, S3_RES, v_max=S_VMAX, a_max=1.0, dt=1.0)
        S, G = rows_of(S3_STARTS, 14).T.copy(), rows_of(S3_GOALS, 14)
        table = MM.MultiTableModel(14, 3)
        cls = model_class or PM.PriorMultiOpenModel
        model = cls(table, 3, G, [O.lattice_hash(3, control, g) for g in G], S_W, S_VMAX, 1.0, list(priors), tol_pos=0.5)
        for k, v in kw.items():
            setattr(model, k, v)
        out = MM.search_many(table, model, oracle_provider(O, oenv), S, [O.lattice_hash(3, control, S[:, q]) for q in range(3)],
                             1.0, delta, 1 << 16, g_max=S3_GMAX)
        _s3[key] = (table, model, out, S)
    return _s3[key]


def s3_priors(O, MM):
    """The VEL stage on the model and its paths as priors: (start rows [14][3], actions [3] lists, model tables [3] with
    S3_NONE's replaced by None, the stage's output)."""
    import replan_model as RM
    table, _, out, S = s3_stage(O, MM, VEL, [None] * 3, 0.0)
    acts, pri = [], []
    for q in range(3):
        ids = RM.path_ids(table, out["results"][q]["goal_id"])
        acts.append([int(table.pred_action[i]) for i in ids[1:]])
        pri.append(None if q == S3_NONE else PM.prior_table(3, VEL, s3_u(), 1.0, S[:, q], acts[q], s3_cells(), S3_DIMS, S3_ORIGIN,
                                                            S3_RES, S_VMAX, S_W, 1.0))
    return S, acts, pri, out


# 2D: an ACC prior (prior dt 0.5, made by hand: speed up along x, coast, drift up, brake) for a JRK search at dt 0.25
S2_DIMS, S2_RES, S2_ORIGIN = [21, 17], 0.5, [-5.25, -4.25]
S2_PDT, S2_DT = 0.5, 0.25


def s2_case():
    """(cells, U of the prior, U of the search, start, goal, actions, the model's table of the prior)."""
    cells = np.zeros(21 * 17, np.int8)
    U1 = np.array(list(itertools.product([-1.0, 0.0, 1.0], repeat=2)))
    start, goal = np.zeros(10), np.zeros(10)
    start[:2], goal[:2] = (-2.0, 0.0), (1.0, 0.5)
    acts = [u_index(U1, 2, v) for v in [(1.0, 0.0)] * 2 + [(0.0, 0.0)] * 3 + [(0.0, 1.0)] + [(-1.0, -1.0)] * 2]
    pri = PM.prior_table(2, ACC, U1, S2_PDT, start, acts, cells, S2_DIMS, S2_ORIGIN, S2_RES, S_VMAX, S_W, S2_DT)
    return cells, U1, 4.0 * U1, start, goal, np.array(acts, np.int32), pri
