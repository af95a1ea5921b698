"""Sequential model of include/mplx_wait.h (the zero control's entry appended to successor lists) and of the park veto of
include/mplx_reserve.h (mplx_reserve_park_device), and the loop of EnvMap.search_many with both on tests/multi_model.py
and tests/reserve_model.py.

The pair arithmetic (primitive, successor state, lattice hashes, limits) is restated for control orders 1 .. 4 in Python
floats: IEEE doubles, one operation per operator, nothing contracted, in the order csrc/mplx_pair_device.h writes it.
Test infrastructure: nothing shared with the engine."""
import math

import numpy as np

import multi_model as MM
import reserve_model as RM
from prior_model import lattice_hash

IS_OPEN, IS_GOAL, SEEN = MM.IS_OPEN, MM.IS_GOAL, MM.SEEN
F = np.float64


def order_of(control):
    return 4 if control & 8 else 3 if control & 4 else 2 if control & 2 else 1


def zero_action(U):
    """The smallest row of U whose every entry is == 0.0 (-0.0 counts), or -1."""
    for a, row in enumerate(np.asarray(U, dtype=F)):
        if all(float(x) == 0.0 for x in row):
            return a
    return -1


def wrap_angle(a):
    while a > math.pi:
        a -= 2.0 * math.pi
    while a < -math.pi:
        a += 2.0 * math.pi
    return a


class Axis:
    """dev::Ax<K> for K in 1 .. 4."""

    def __init__(self, K, p, v, a, u, j=0.0):
        self.K = K
        self.c1 = self.c2 = self.c3 = self.c4 = 0.0
        self.c5 = p
        if K == 1:
            self.c4 = u
        elif K == 2:
            self.c4, self.c3 = v, u
        elif K == 3:
            self.c4, self.c3, self.c2 = v, a, u
        elif K == 4:
            self.c4, self.c3, self.c2, self.c1 = v, a, j, u
        else:
            raise ValueError("the model covers VEL, ACC, JRK and SNP")
        self.c3_2, self.c2_6, self.c2_2 = self.c3 / 2, self.c2 / 6, self.c2 / 2
        self.c1_24, self.c1_6, self.c1_2 = self.c1 / 24, self.c1 / 6, self.c1 / 2
        self.u = u

    def pos(self, t):  # EXACT
        K = self.K
        if K == 1:
            return (0.0 + self.c4 * t) + self.c5
        if K == 2:
            return ((0.0 + (self.c3_2 * t) * t) + self.c4 * t) + self.c5
        if K == 3:
            return (((0.0 + self.c2_6 * ((t * t) * t)) + (self.c3_2 * t) * t) + self.c4 * t) + self.c5
        t3 = (t * t) * t
        return ((((0.0 + self.c1_24 * (t3 * t)) + self.c2_6 * t3) + (self.c3_2 * t) * t) + self.c4 * t) + self.c5

    def vel(self, t):  # EXACT (the forms without the leading 0.0 differ in the sign of a zero only)
        K = self.K
        if K == 1:
            return 0.0 + self.c4
        if K == 2:
            return (0.0 + self.c3 * t) + self.c4
        if K == 3:
            return ((0.0 + (self.c2_2 * t) * t) + self.c3 * t) + self.c4
        return (((0.0 + self.c1_6 * ((t * t) * t)) + (self.c2_2 * t) * t) + self.c3 * t) + self.c4

    def acc(self, t):
        K = self.K
        if K == 1:
            return 0.0
        if K == 2:
            return 0.0 + self.c3
        if K == 3:
            return (0.0 + self.c2 * t) + self.c3
        return ((0.0 + (self.c1_2 * t) * t) + self.c2 * t) + self.c3

    def jrk(self, t):
        if self.K <= 2:
            return 0.0
        return 0.0 + self.c2 if self.K == 3 else (0.0 + self.c1 * t) + self.c2

    def max_vel(self, T):
        m = max(abs(self.c4), abs(self.vel(T)))  # (v0 < vT ? vT : v0; NaNs do not occur in the tests)
        if self.K == 3 or (self.K == 4 and self.c1_2 == 0):
            if self.c2 != 0:
                r = -self.c3 / self.c2
                if 0 < r < T:
                    m = max(m, abs(self.vel(r)))
        elif self.K == 4:  # the roots of v'(t) = c1/2 t^2 + c2 t + c3 in solver order; the scan stops at a root >= T
            disc = self.c2 * self.c2 - 4 * self.c1_2 * self.c3
            if not disc < 0:
                sq = math.sqrt(disc)
                r1, r2 = (-self.c2 - sq) / (2 * self.c1_2), (-self.c2 + sq) / (2 * self.c1_2)
                go_on = True
                if 0 < r1 < T:
                    m = max(m, abs(self.vel(r1)))
                elif r1 >= T:
                    go_on = False
                if go_on and 0 < r2 < T:
                    m = max(m, abs(self.vel(r2)))
        return m

    def max_acc(self, T):
        m = max(abs(self.c3), abs(self.acc(T)))
        if self.K == 4 and self.c1 != 0:
            r = -self.c2 / self.c1
            if 0 < r < T:
                m = max(m, abs(self.acc(r)))
        return m

    def max_jrk(self, T):
        return max(abs(self.c2), abs(self.jrk(T)))

    def effort(self, T):
        return self.u * self.u * T


def pair_eval(dim, control, row, u, dt, v_max=0.0, a_max=0.0, j_max=0.0, yaw_max=0.0):
    """One (state row [4D+2], control row u) pair as pair::Pair evaluates it: a dict with the successor rows "next"
    [4D+2] (t = tp + dt), h_next, h_curr, valid (heading where it applies, then the limits), same_pos, J."""
    D, K, yaw = dim, order_of(control), bool(control & 16)
    row = [float(x) for x in row]
    g = lambda o, i: row[o * D + i]
    ax = [Axis(K, g(0, i), g(1, i) if K >= 2 else 0.0, g(2, i) if K >= 3 else 0.0, float(u[i]), g(3, i) if K >= 4 else 0.0)
          for i in range(D)]
    cyaw = row[4 * D] if yaw else 0.0
    uyaw = float(u[D]) if yaw else 0.0
    T = float(dt)
    nxt = [0.0] * (4 * D + 2)
    for i in range(D):
        nxt[i], nxt[D + i], nxt[2 * D + i], nxt[3 * D + i] = ax[i].pos(T), ax[i].vel(T), ax[i].acc(T), ax[i].jrk(T)
    nxt[4 * D] = wrap_angle((0.0 + uyaw * T) + cyaw) if yaw else 0.0
    nxt[4 * D + 1] = row[4 * D + 1] + T
    cur = list(row)
    for i in range(D):  # rows the control order does not read are 0.0 in the pair
        if K < 2:
            cur[D + i] = 0.0
        if K < 3:
            cur[2 * D + i] = 0.0
        if K < 4:
            cur[3 * D + i] = 0.0
    cur[4 * D] = cyaw
    valid = True
    if yaw and yaw_max > 0:
        cos_lim = math.cos(yaw_max)

        def heading_ok(vx, vy, y):
            if vx != 0 or vy != 0:
                s = math.sqrt(vx * vx + vy * vy)
                return not (vx / s * math.cos(y) + vy / s * math.sin(y) < cos_lim)
            return True
        y0 = wrap_angle((0.0 + uyaw * 0.0) + cyaw)
        ok0 = heading_ok(ax[0].vel(0.0), ax[1].vel(0.0), y0)
        okT = heading_ok(nxt[D], nxt[D + 1], nxt[4 * D])
        valid = ok0 and okT
    if K >= 2 and v_max > 0:
        valid = valid and all(not (a.max_vel(T) > v_max) for a in ax)
    if K >= 3 and a_max > 0:
        valid = valid and all(not (a.max_acc(T) > a_max) for a in ax)
    if K >= 4 and j_max > 0:
        valid = valid and all(not (a.max_jrk(T) > j_max) for a in ax)
    J = 0.0
    for a in ax:
        J += a.effort(T)
    return {"next": nxt, "h_next": lattice_hash(D, control, nxt), "h_curr": lattice_hash(D, control, cur), "valid": valid,
            "same_pos": all(row[i] == nxt[i] for i in range(D)), "J": J}


def post_eval(dim, goal, h, s):
    """heur / flags of mplx_post_lists_device for hash h and state rows s; goal: dict(row, hash, w, v_max, tol_pos,
    tol_vel, tol_acc, tol_yaw)."""
    D, g = dim, [float(x) for x in goal["row"]]
    linf = lambda o: max([0.0] + [abs(float(s[o + i]) - g[o + i]) for i in range(D)])
    is_goal_state = int(h) == int(goal["hash"])
    m = linf(0)
    w, v_max = float(goal["w"]), float(goal["v_max"])
    heur = 0.0 if is_goal_state else (w * m / v_max if v_max > 0 else w * m)
    ok = m <= goal["tol_pos"]
    if ok and goal["tol_vel"] >= 0:
        ok = linf(D) <= goal["tol_vel"]
    if ok and goal["tol_acc"] >= 0:
        ok = linf(2 * D) <= goal["tol_acc"]
    if ok and goal["tol_yaw"] >= 0:
        ok = abs(float(s[4 * D]) - g[4 * D]) <= goal["tol_yaw"]
    return heur, (1 if ok else 0) | (2 if is_goal_state else 0)


def add_wait(lists, n_nodes, parent_state, parent_id, dim, control, U, dt, w, v_max=0.0, a_max=0.0, j_max=0.0, yaw_max=0.0,
             goal=None):
    """mplx_lists_add_wait_device on lists in the dict layout of tests/table_model.py ("stride", "count", "action",
    "cost", and any of "hash", "state", "heur", "flags", "iters"): the arrays are modified in place.  parent_id None: no
    row is skipped.  Returns (n_added, eligible [n_nodes] bool -- the pair's three conditions, whatever count and
    parent_id say), or raises ValueError without a zero row."""
    a0 = zero_action(U)
    if a0 < 0:
        raise ValueError("no zero row in U")
    S = int(lists["stride"])
    u0 = np.asarray(U, dtype=F)[a0]
    eligible = np.zeros(n_nodes, dtype=bool)
    n_added = 0
    for k in range(n_nodes):
        p = pair_eval(dim, control, np.asarray(parent_state)[:, k], u0, dt, v_max, a_max, j_max, yaw_max)
        eligible[k] = p["h_next"] == p["h_curr"] and p["valid"] and p["same_pos"]
        if parent_id is not None and parent_id[k] < 0:
            continue
        cnt = int(lists["count"][k])
        if not eligible[k] or not 0 <= cnt < S:
            continue
        e = k * S + cnt
        lists["action"][e] = a0
        lists["cost"][e] = 0.0 + (p["J"] + float(w) * float(dt))
        if lists.get("hash") is not None:
            lists["hash"][e] = p["h_next"]
        if lists.get("state") is not None:
            lists["state"][:, e] = p["next"]
        if lists.get("iters") is not None:
            lists["iters"][e] = 0
        if lists.get("heur") is not None or lists.get("flags") is not None:
            heur, flags = post_eval(dim, goal, p["h_next"], p["next"])
            if lists.get("heur") is not None:
                lists["heur"][e] = heur
            if lists.get("flags") is not None:
                lists["flags"][e] = flags
        lists["count"][k] = cnt + 1
        n_added += 1
    return n_added, eligible


# ---- the park veto
def park_instants(step, n_steps, t0, t_node):
    """Every i in [0, n_steps) with tl_i = (double)i * step - t0 >= t_node."""
    tl = np.arange(n_steps).astype(F) * F(step) - F(t0)
    with np.errstate(invalid="ignore"):
        return np.nonzero(tl >= F(t_node))[0]


def park_first_scan(step, n_steps, t0, t_node, n_scan=4):
    """The kernel's way to the first of them: a guess from (t_node + t0) / step, then at most n_scan instants.  n_steps:
    none."""
    step, t0, tn = F(step), F(t0), F(t_node)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (tn + t0) / step
    g = 0
    if x >= 1.0:
        g = int(x) - 1 if x < 2147483647.0 else n_steps
    for s in range(n_scan):
        i = g + s
        if i >= n_steps:
            break
        if F(i) * step - t0 >= tn:
            return i
    return n_steps


def park(flags, n_nodes, fr, n_max, capacity, res, queries, dim, node_query=None):
    """mplx_reserve_park_device.  flags: [>= n_nodes] uint8 (a copy is changed); fr: dict(count, id, state [4D+2][.]);
    res: the dict of Reservations.positions(); queries: (t0 [Q], radius [Q], ignore [Q]); node_query: per node its query
    or None (one query).  Returns (flags_out, hit [walked rows] int64, n_vetoed)."""
    flags = np.array(flags, dtype=np.uint8)
    q_t0, q_r, q_ign = (np.asarray(x) for x in queries)
    Q = len(q_t0)
    pos, act = np.asarray(res["pos"], dtype=F), np.asarray(res["active"]) != 0
    inc, r_b, g_b = np.asarray(res["included"]) != 0, np.asarray(res["radius"], dtype=F), np.asarray(res["group"])
    n_steps = pos.shape[0]
    step = F(res["step"])
    n = max(0, min(int(fr["count"]), int(n_max), int(capacity)))
    hit = np.full(n, -1, np.int64)
    n_vetoed = 0
    F_t = 4 * dim + 1
    for r in range(n):
        i_d = int(fr["id"][r])
        if not 0 <= i_d < n_nodes or not flags[i_d] & IS_GOAL:
            continue
        q = 0 if node_query is None else int(node_query[i_d])
        if q < 0 or q >= Q:
            continue
        p, t_node = np.asarray(fr["state"], dtype=F)[:dim, r], F(fr["state"][F_t][r])
        on_q = inc & (g_b != q_ign[q])
        rr = F(q_r[q]) + r_b
        rr2 = rr * rr
        for i in park_instants(step, n_steps, q_t0[q], t_node):
            with np.errstate(invalid="ignore", over="ignore"):
                d2 = None
                for d in range(dim):
                    dx = p[d] - pos[i, d]
                    d2 = dx * dx if d2 is None else d2 + dx * dx
                conf = on_q & act[i] & (d2 < rr2)
            if conf.any():
                hit[r] = (int(i) << 32) | int(np.argmax(conf))
                flags[i_d] &= np.uint8(0xFF ^ IS_GOAL)
                n_vetoed += 1
                break
    return flags, hit, n_vetoed


# ---- reservations from chains, in closed form (the scenarios' tables; the GPU tests take the device's own table)
def chain_table(dim, control, U, dt, starts, actions, step, n_steps, t0, radius, mode=0):
    """The table of B action chains: starts [4D+2][B], actions [H][B] (-1 ends).  pos at the clamped local time, from the
    chain state of its segment (RM.primitive_pos); PARK (0): active everywhere, GONE (1): within [0, total]."""
    import conflict_model as cm
    K = order_of(control)
    starts, actions = np.asarray(starts, dtype=F), np.asarray(actions)
    B = starts.shape[1]
    t0 = np.broadcast_to(np.asarray(t0, dtype=F), (B,))
    tl = cm.local_times(step, n_steps, t0, B)
    pos = np.zeros((n_steps, dim, B))
    total = np.zeros(B)
    for b in range(B):
        states = [starts[:, b].copy()]
        acts = []
        for a in actions[:, b]:
            if a < 0:
                break
            nxt = np.array(pair_eval(dim, control, states[-1], np.asarray(U, dtype=F)[a], dt)["next"])
            states.append(nxt)
            acts.append(int(a))
        total[b] = len(acts) * float(dt)
        for i in range(n_steps):
            t = min(max(float(tl[b, i]), 0.0), total[b])
            k = min(int(t / float(dt)), len(acts) - 1) if acts else 0
            if not acts:
                pos[i, :, b] = states[0][:dim]
                continue
            s = states[k]
            v = s[dim:2 * dim] if K >= 2 else np.zeros(dim)
            a_ = s[2 * dim:3 * dim] if K >= 3 else np.zeros(dim)
            j_ = s[3 * dim:4 * dim] if K >= 4 else np.zeros(dim)
            pos[i, :, b] = RM.primitive_pos(s[:dim], v, a_, j_, np.asarray(U, dtype=F)[acts[k]][:dim], K, t - k * float(dt))
    return {"pos": pos, "active": cm.active_mask(tl, total, mode).astype(np.uint8), "included": np.ones(B, np.uint8),
            "radius": np.broadcast_to(np.asarray(radius, dtype=F), (B,)).copy(), "group": np.arange(B, dtype=np.int32),
            "step": float(step)}


# ---- the loop of EnvMap.search_many(avoid=, time_keys=True, wait=, park_goal=) on the models
class ParkOpenModel(MM.MultiOpenModel):
    """MultiOpenModel whose every push is followed by the park veto (park_goal) against `res` / `queries`."""

    def __init__(self, *a, res=None, queries=None, park_goal=False, **kw):
        super().__init__(*a, **kw)
        self.res, self.queries, self.park_goal = res, queries, park_goal
        self.n_vetoed = 0

    def push(self, fr, n_max, eps, sight=0, capacity=None):
        super().push(fr, n_max, eps, sight, capacity)
        if not self.park_goal:
            return
        n = self.table.n_nodes
        fl = np.zeros(n, np.uint8)
        for i, v in self.flags.items():
            fl[i] = v
        cap = len(fr["id"]) if capacity is None else capacity
        out, _, nv = park(fl, n, fr, n_max, cap, self.res, self.queries, self.dim, self.table.query)
        for i in self.flags:
            self.flags[i] = int(out[i])
        self.n_vetoed += nv


def search_many(provider, dim, control, U, dt, w, limits, starts, start_hashes, goal_rows, goal_hashes, res, queries, n_steps,
                wait, park_goal, eps=1.0, delta=None, capacity=1 << 16, v_max_heur=1.0, tol_pos=0.5, max_rounds=None):
    """Q searches among the reservations `res` with time keys.  provider: states [4D+2][n] -> lists (tests/table_model.py);
    its hashes are folded with the entries' t rows (RM.time_key), waits are appended (wait), the check of
    tests/reserve_model.py blocks entries, and every push is followed by the veto (park_goal).  Returns (out of
    MM.search_many, table, open model)."""
    Q = np.asarray(starts).shape[1]
    K = order_of(control)
    U = np.asarray(U, dtype=F)
    table = MM.MultiTableModel(4 * dim + 2, Q)
    opn = ParkOpenModel(table, dim, goal_rows, goal_hashes, w=w, v_max=v_max_heur, tol_pos=tol_pos, res=res,
                        queries=queries, park_goal=park_goal)
    # the goal's own lattice state is recognised by its hash; with time keys no key equals it, as on the device
    opn.goal_hashes = [-1] * Q
    step = res["step"]
    state_of = {}

    def wrapped(states):
        states = np.asarray(states, dtype=F)
        n = states.shape[1]
        lists = provider(states)
        S = int(lists["stride"])
        if wait:
            add_wait(lists, n, states, None, dim, control, U, dt, w, *limits)
        # whose the rows are: the table's node of (query, key) -- the rows come from a select, in id order
        row_q = np.array([state_of[tuple(states[:, k])] for k in range(n)], np.int32)

        def edge_pos(k, j, i, s):
            st = states[:, k]
            u = U[int(lists["action"][k * S + j])][:dim]
            z = np.zeros(dim)
            return RM.primitive_pos(st[:dim], st[dim:2 * dim] if K >= 2 else z, st[2 * dim:3 * dim] if K >= 3 else z,
                                    st[3 * dim:4 * dim] if K >= 4 else z, u, K, s)
        cost, _, _, _ = RM.check(lists["count"], lists["action"], lists["cost"], S, np.zeros(n, np.int32), states[-1], dt, len(U),
                                 step, n_steps, res, queries, edge_pos, row_q)
        lists["cost"] = cost
        for k in range(n):
            for j in range(int(lists["count"][k])):
                e = k * S + j
                lists["hash"][e] = RM.time_key(int(lists["hash"][e]), float(lists["state"][-1, e]))
                state_of[tuple(lists["state"][:, e])] = row_q[k]
        return lists
    for q in range(Q):
        state_of[tuple(np.asarray(starts, dtype=F)[:, q])] = q
    if delta is None:
        delta = float(w) * float(dt)
    keys = [RM.time_key(int(h), float(np.asarray(starts)[-1, q])) for q, h in enumerate(start_hashes)]
    out = MM.search_many(table, opn, wrapped, np.asarray(starts, dtype=F), keys, eps, delta, capacity, max_rounds=max_rounds)
    return out, table, opn


def path_of(table, goal_id):
    """(ids root first, actions) of the chain of best predecessors."""
    ids, acts = [int(goal_id)], []
    while table.pred[ids[-1]] >= 0:
        acts.append(int(table.pred_action[ids[-1]]))
        ids.append(int(table.pred[ids[-1]]))
    return ids[::-1], acts[::-1]
