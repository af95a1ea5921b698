"""Inputs shared by tests/test_reserve_poly_model.py (CPU) and tests/test_gpu_reserve_poly.py: loaded trajectory sets as
EnvMap.load_traj takes them, a host evaluation of their positions (the expression of traj::eval_segment on exactly
representable inputs, for the CPU tests; the GPU tests feed the model the device's own samples), and the table a fill
leaves, built on the host.

random_case: candidates and reservations as the fixture of tests/test_gpu_conflict.py builds them -- c5 on the quarter
grid in [0, R), c4 in sixteenths within +-1, c3 in sixteenths within +-0.5, segment times in quarters from 0.5 to 3 --
with S = 1 + k % 5 segments (every seventh candidate and every ninth reservation S = 0: a failed load, excluded), t_start
in quarters from -2 to 6, radii from {0.125, 0.25, 0.5}, groups b // 2 and ignored groups k % 4 - 1; step 0.25 and a
horizon of n_steps = 57 instants (14 time units) that the longest candidates leave.

hand_case: one-segment candidates on straight lines among stationary reservations, every number exactly representable,
each problem built for one rule of include/mplx_reserve_poly.h; its expected hits are written out.

long_hand_case, long_random_case, inexact_case, keep_case (the end of the file): windows of more than two blocks of 64
instants, steps that are no power of two, tables in which only partners past the kernel's register tiles are met."""
import numpy as np

import conflict_model as CM

F = np.float64
STEP = 0.25
WMAX = 6


def segs_position(c, dts, n_segs, k, tl):
    """Position [D] of trajectory k of (c [S][D + 1][6][K], dts [S][K], n_segs [K]) at local time tl in [0, total]:
    the first segment whose end admits tl, then ((((c0/120 t^5 + c1/24 t^4) + c2/6 t^3) + c3/2 t t) + c4 t) + c5."""
    D = c.shape[1] - 1
    tau, s = F(0.0), 0
    for s in range(int(n_segs[k])):
        if tl <= tau + dts[s, k] or s == n_segs[k] - 1:
            break
        tau = tau + dts[s, k]
    t = F(tl) - tau
    t3 = (t * t) * t
    t4 = t3 * t
    t5 = t4 * t
    a = c[s, :D, :, k]
    return ((((a[:, 0] / 120 * t5 + a[:, 1] / 24 * t4) + a[:, 2] / 6 * t3) + a[:, 3] / 2 * t * t) + a[:, 4] * t) + a[:, 5]


def totals(dts, n_segs):
    out = np.zeros(dts.shape[1])
    for k in range(dts.shape[1]):
        t = F(0.0)
        for s in range(int(n_segs[k])):
            t = t + dts[s, k]
        out[k] = t
    return out


def host_table(c, dts, n_segs, step, n_steps, t0, radius, group, park):
    """The dict of Reservations.positions() for a loaded set, on the host: the init and position rules of
    include/mplx_conflict.h (local time clamped to [0, total] under PARK)."""
    B, D = dts.shape[1], c.shape[1] - 1
    total = totals(dts, n_segs)
    ok = CM.inputs_ok(B, t0, radius)
    inc = (np.asarray(n_segs) > 0) & ok
    tl = CM.local_times(step, n_steps, t0, B)
    pos = np.zeros((n_steps, D, B))
    for b in np.nonzero(inc)[0]:
        for i in range(n_steps):
            pos[i, :, b] = segs_position(c, dts, n_segs, b, min(max(tl[b, i], 0.0), total[b]))
    act = CM.active_mask(tl, total, CM.PARK if park else CM.GONE) & inc[None, :]
    return {"pos": pos, "active": act.astype(np.uint8), "included": inc.astype(np.uint8),
            "radius": np.where(inc, np.broadcast_to(np.asarray(radius, dtype=F), (B,)), 0.0),
            "group": np.arange(B, dtype=np.int32) if group is None else np.asarray(group, dtype=np.int32)}


def random_set(rng, D, n, R, every_empty):
    c = np.zeros((WMAX - 1, D + 1, 6, n))
    c[:, :D, 5, :] = rng.integers(0, 4 * R, (WMAX - 1, D, n)) / 4.0
    c[:, :D, 4, :] = rng.integers(-16, 17, (WMAX - 1, D, n)) / 16.0
    c[:, :D, 3, :] = rng.integers(-8, 9, (WMAX - 1, D, n)) / 16.0
    dts = rng.integers(2, 13, (WMAX - 1, n)) / 4.0
    n_segs = (1 + np.arange(n) % (WMAX - 1)).astype(np.int32)
    n_segs[every_empty - 1::every_empty] = 0
    return c, dts, n_segs


def random_case(D, K, B, seed=0):
    """{"cand": (c, dts, n_segs), "t_start", "radius", "ignore" [K]; "res": (c, dts, n_segs), "t0", "r_b", "group" [B];
    "step", "n_steps"}.  R shrinks with B so that the share of problems with a hit stays in the middle."""
    rng = np.random.default_rng(4200 + 1000 * D + 10 * K + B + 100000 * seed)
    R = 6 if D == 3 else 16
    case = {"cand": random_set(rng, D, K, R, 7), "res": random_set(rng, D, B, R, 9), "step": STEP, "n_steps": 57}
    case["t_start"] = rng.integers(-8, 25, K) / 4.0
    case["radius"] = rng.choice([0.125, 0.25, 0.5], K)
    case["ignore"] = (np.arange(K) % 4 - 1).astype(np.int32)
    case["t0"] = rng.integers(-4, 9, B) / 4.0
    case["r_b"] = rng.choice([0.125, 0.25, 0.5], B)
    case["group"] = (np.arange(B) // 2).astype(np.int32)
    return case


def line(D, K):
    return np.zeros((1, D + 1, 6, K)), np.zeros((1, K)), np.ones(K, np.int32)


def hand_case(park):
    """D = 2, step 0.25, n_steps 81 (the last instant is t = 20).  Reservations, stationary for 8 time units from t0 = 0
    (PARK: for ever; GONE: until t = 8) unless said otherwise, radius 0.25:
      0 at (16, 0)      1 at (16.25, 1)    2 at (0, 2)      3 at (3.125, 3)   4 at (2, 4), group 7
      5 at (2, 5), S = 0 (excluded)      6 at (2, 6), radius -1 (excluded, BAD_INPUT)
      7 at (0.75, 7)    8 at (9, 8)      9 at (2, 9), stationary for 20
    Candidates move along x with speed 1 from (x0, y) unless said otherwise, radius 0.125:
      0  y = 0, t_start 0, total 15.75: 64 instants, the last exactly at tl = total, where it meets 0 (PARK; GONE: gone)
      1  y = 1, t_start 0, total 16: 65 instants, the last exactly at tl = total, where it meets 1 (PARK)
      2  y = 2, t_start 1, total 2: meets 2 at tl = 0 exactly, instant 4
      3  y = 3, x0 = 3.0625, t_start 0.0625, total 0.125: no instant falls into it; it would meet 3
      4  y = 3, x0 = 3, t_start 0.125, total 0.25: one instant (1, tl = 0.125), where it meets 3
      5  y = 4, t_start -0.5 (x = 0.5 at instant 0), total 4, ignores group 7: passes 4 unharmed
      6  y = 4, as 5 but ignoring nothing: meets 4 at instant 5 (x = 1.75: |dx| = 0.25 < 0.375)
      7  y = 5, total 4: passes the excluded 5       8  y = 6, total 4: passes the excluded 6
      9  stands at (0, 7), total 1, radius 0.5: touches 7 (d2 = 0.5625 = rr * rr): no conflict
      10 stands at (0.0625, 7), total 1, radius 0.5: inside 7, instant 0
      11 y = 8, t_start 4, total 16: ends exactly on the horizon, is checked, meets 8 at t = 12.75 (PARK: instant 51)
      12 y = 8, t_start 4, total 16.25: one instant past the horizon: -2
      13 t_start NaN      14 radius -0.5      15 S = 0 (a set status)
      16 y = 9, t_start 10, total 4: meets 9 (active under both modes) at instant 47 (x = 1.75)."""
    B, K = 10, 17
    rc, rd, rs = line(2, B)
    at = [(16, 0), (16.25, 1), (0, 2), (3.125, 3), (2, 4), (2, 5), (2, 6), (0.75, 7), (9, 8), (2, 9)]
    rc[0, :2, 5, :] = np.array(at).T
    rd[0, :] = 8.0
    rd[0, 9] = 20.0
    rs[5] = 0
    r_b = np.full(B, 0.25)
    r_b[6] = -1.0
    group = np.arange(B, dtype=np.int32)
    group[4] = 7
    c, d, s = line(2, K)
    rows = {0: (0, 0, 0, 15.75), 1: (0, 1, 0, 16), 2: (0, 2, 1, 2), 3: (3.0625, 3, 0.0625, 0.125), 4: (3, 3, 0.125, 0.25),
            5: (0, 4, -0.5, 4), 6: (0, 4, -0.5, 4), 7: (0, 5, 0, 4), 8: (0, 6, 0, 4), 9: (0, 7, 0, 1), 10: (0.0625, 7, 0, 1),
            11: (0, 8, 4, 16), 12: (0, 8, 4, 16.25), 13: (0, 0, np.nan, 1), 14: (0, 0, 0, 1), 15: (0, 0, 0, 1), 16: (0, 9, 10, 4)}
    t_start = np.zeros(K)
    for k, (x0, y, ts, tot) in rows.items():
        c[0, 0, 5, k], c[0, 1, 5, k], t_start[k], d[0, k] = x0, y, ts, tot
        c[0, 0, 4, k] = 0.0 if k in (9, 10) else 1.0
    s[15] = 0
    radius = np.full(K, 0.125)
    radius[[9, 10]] = 0.5
    radius[14] = -0.5
    ignore = np.full(K, -1, np.int32)
    ignore[5] = 7

    def key(i, b):
        return (i << 32) | b

    hit = np.full(K, -1, np.int64)
    hit[2], hit[4], hit[6], hit[10], hit[12], hit[16] = key(4, 2), key(1, 3), key(5, 4), key(0, 7), -2, key(47, 9)
    if park:
        hit[0], hit[1], hit[11] = key(63, 0), key(64, 1), key(51, 8)
    status = np.zeros(K, np.uint8)
    status[13] = status[14] = 128
    status[15] = 1  # SOLVE_EMPTY
    return {"cand": (c, d, s), "t_start": t_start, "radius": radius, "ignore": ignore, "res": (rc, rd, rs), "t0": np.zeros(B),
            "r_b": r_b, "group": group, "step": STEP, "n_steps": 81, "hit": hit, "status": status}


# ------------------------------------------------------------------ past one block, past an exact step, past kKeep
# (tests/test_reserve_poly_long_model.py on the CPU, tests/test_gpu_reserve_poly_long.py on the device)
def line_table(c, dts, n_segs, step, n_steps, t0, radius, group, park):
    """host_table for a set of one-segment CONSTANT trajectories (line(): only c5 set): the same dict without the
    position loop, which at thousands of instants is too slow."""
    B, D = dts.shape[1], c.shape[1] - 1
    assert c.shape[0] == 1 and not c[0, :, :5].any()
    inc = (np.asarray(n_segs) > 0) & CM.inputs_ok(B, t0, radius)
    tl = CM.local_times(step, n_steps, t0, B)
    pos = np.broadcast_to(np.where(inc[None, :], c[0, :D, 5, :], 0.0)[None], (n_steps, D, B)).copy()
    act = CM.active_mask(tl, totals(dts, n_segs), CM.PARK if park else CM.GONE) & inc[None, :]
    return {"pos": pos, "active": act.astype(np.uint8), "included": inc.astype(np.uint8),
            "radius": np.where(inc, np.broadcast_to(np.asarray(radius, dtype=F), (B,)), 0.0),
            "group": np.arange(B, dtype=np.int32) if group is None else np.asarray(group, dtype=np.int32)}


# long_hand_case: candidate k -> (t_start, instants of its window, [(b, offset of the meeting in the window)], the
# expected (offset, b) or None).  The kernel walks a window in blocks of 64 instants from its first one and a block in
# passes of 8.
LONG_ROWS = {
    0: (1.0, 128, [(0, 63)], (63, 0)),        # the last lane of block 0
    1: (1.25, 129, [(1, 64)], (64, 1)),       # the first lane of block 1
    2: (1.5, 192, [(2, 71)], (71, 2)),        # the last instant of a pass (block 1, pass 0)
    3: (1.75, 193, [(3, 72)], (72, 3)),       # the first instant of the next pass
    4: (2.0, 200, [(4, 127)], (127, 4)),      # the last lane of block 1
    5: (2.25, 200, [(6, 128)], (128, 6)),     # the first lane of block 2: the third block
    6: (2.5, 129, [(8, 128)], (128, 8)),      # ... where it is the window's only instant of that block, at tl = total
    7: (2.75, 200, [(9, 129)], (129, 9)),
    8: (3.0, 128, [(10, 127)], (127, 10)),    # the last instant of a window of exactly two blocks
    9: (3.25, 193, [(11, 192)], (192, 11)),   # the single instant of a fourth block
    10: (3.5, 200, [(12, 130), (13, 70)], (70, 13)),   # conflicts in two blocks: the earlier wins, whatever b
    11: (3.75, 200, [(5, 78), (40, 74)], (74, 40)),    # one pass (offsets 72 .. 79): lane 5 at 6, lane 40 at 2 of it
    12: (4.0, 200, [(41, 100), (7, 100)], (100, 7)),   # two partners at one instant: the smaller b
    13: (33.0, 129, [(64, 128)], (128, 64)),  # the window's last instant is the table's last; a partner of the second tile
    14: (4.25, 200, [], None),                # four blocks walked, nothing met
    15: (-2.0, 153, [(65, 130)], (130, 65)),  # started before the clock: the window begins at instant 0 with tl = 2
}
LONG_B, LONG_STEPS = 66, 261


def long_hand_case(D):
    """Step 0.25, n_steps 261 (the last instant is t = 65).  LONG_B = 66 stationary reservations of radius 0.0625 that
    stand from t0 = 0 for 65 (active at every instant under PARK and GONE alike); candidate k moves along x with speed 1
    from (0, 2 k) with radius 0.0625, so that it meets a reservation at (0.25 o (+ 2 for k = 15), 2 k) at window offset o
    and at no other instant: one instant further dx = 0.25 and rr = 0.125.  Reservations no row names stand far away.  In
    3-D everybody has z = 0.5.  The expected hits are LONG_ROWS's."""
    K, B = len(LONG_ROWS), LONG_B
    rc, rd, rs = line(D, B)
    rc[0, 0, 5, :], rc[0, 1, 5, :] = -1000.0, -1000.0 - np.arange(B)
    rd[0, :] = 65.0
    c, d, s = line(D, K)
    t_start, hit = np.zeros(K), np.full(K, -1, np.int64)
    for k, (ts, n, meets, want) in LONG_ROWS.items():
        first, tl0 = (0, -ts) if ts < 0 else (int(ts * 4), 0.0)
        c[0, 0, 4, k], c[0, 1, 5, k], t_start[k], d[0, k] = 1.0, 2.0 * k, ts, tl0 + 0.25 * (n - 1)
        for b, o in meets:
            rc[0, 0, 5, b], rc[0, 1, 5, b] = tl0 + 0.25 * o, 2.0 * k
        if want is not None:
            hit[k] = ((first + want[0]) << 32) | want[1]
    if D == 3:
        rc[0, 2, 5, :], c[0, 2, 5, :] = 0.5, 0.5
    return {"cand": (c, d, s), "t_start": t_start, "radius": np.full(K, 0.0625), "ignore": np.full(K, -1, np.int32), "res": (rc, rd, rs),
            "t0": np.zeros(B), "r_b": np.full(B, 0.0625), "group": np.arange(B, dtype=np.int32), "step": STEP, "n_steps": LONG_STEPS,
            "hit": hit, "status": np.zeros(K, np.uint8)}


LONG_STEP = 1.0 / 32


def long_random_case(D, K, B, seed=0):
    """random_case on a clock 8 times as fine: step 1/32 and 449 instants for the same 14 time units, so that a candidate
    of more than 4 time units has more than 128 instants."""
    case = random_case(D, K, B, seed)
    case["step"], case["n_steps"] = LONG_STEP, 8 * 56 + 1
    return case


INEXACT_STEPS = (0.1, 1.0 / 3.0)
INEXACT_I = (0, 1, 2, 3, 63, 64, 1000, 5000)
INEXACT_N = 5004


def inexact_case(D, step):
    """Steps that are no power of two: t_start / step is a rounded quotient and the kernel's guess of the first instant
    may be off by one either way.  Problem (i, n, j): a candidate standing at its own place (20 apart) for 2.5 steps from
    t_start = fl(i step) (n = 0), the double below it (n = -1) or above it (n = 1); a reservation standing on it that is
    active at the single instant i + j, j in {-1, 0, 1} (GONE, t0 = fl((i + j) step), total half a step).  The
    candidate's instants are i, i + 1, i + 2, without i where t_start lies above fl(i step): so the expected hit is
    (i + j, b) for j = 1, for j = 0 unless n = 1, and none for j = -1.  GONE only."""
    rows = [(i, n, j) for i in INEXACT_I for n in (-1, 0, 1) for j in (-1, 0, 1) if i + j >= 0]
    K = len(rows)
    c, d, s = line(D, K)
    rc, rd, rs = line(D, K)
    t_start, t0, hit = np.zeros(K), np.zeros(K), np.full(K, -1, np.int64)
    for k, (i, n, j) in enumerate(rows):
        at = F(i) * F(step)
        t_start[k] = at if n == 0 else np.nextafter(at, np.inf if n > 0 else -np.inf)
        t0[k] = F(i + j) * F(step)
        c[0, 0, 5, k] = rc[0, 0, 5, k] = 20.0 * k
        c[0, 1:D, 5, k] = rc[0, 1:D, 5, k] = 0.5
        if j == 1 or (j == 0 and n != 1):
            hit[k] = ((i + j) << 32) | k
    d[0, :], rd[0, :] = 2.5 * step, 0.5 * step
    return {"cand": (c, d, s), "t_start": t_start, "radius": np.full(K, 0.25), "ignore": np.full(K, -1, np.int32), "res": (rc, rd, rs),
            "t0": t0, "r_b": np.full(K, 0.25), "group": np.arange(K, dtype=np.int32), "step": step, "n_steps": INEXACT_N,
            "hit": hit, "status": np.zeros(K, np.uint8), "rows": rows}


KEEP_K = 130


def keep_case(D, B, seed=0):
    """Past the kKeep = 4 tiles whose radius sums the kernel keeps in registers: random_case(D, KEEP_K, B) with the
    reservations b < 256 moved to where no candidate comes (x + 1000), every eleventh radius (b % 11 == 5) -1 (excluded,
    BAD_INPUT) next to the S = 0 of every ninth, and ignore[k] (even k) = the group of the partner the model finds for
    problem k when nobody is ignored -- so that every rule the load path past kKeep re-derives per pass decides hits.
    Reservation B - 1 is the trajectory of candidate case["rider"] itself, on that candidate's clock.
    Also "nobody": the model's hits with nobody ignored."""
    import reserve_poly_model as RPM
    case = random_case(D, KEEP_K, B, seed)
    rc, rd, rs = case["res"]
    rc[:, 0, 5, :256] += 1000.0
    case["r_b"][5::11] = -1.0
    c, dts, n_segs = case["cand"]
    status = np.where(n_segs == 0, 1, 0).astype(np.uint8)
    own = lambda k, i, tl: segs_position(c, dts, n_segs, k, tl)

    def hits_of_nobody():
        table = host_table(rc, rd, rs, case["step"], case["n_steps"], case["t0"], case["r_b"], case["group"], False)
        return RPM.check(status, n_segs, totals(dts, n_segs), case["t_start"], case["radius"], None, case["step"], table, own)[0]

    # the last reservation -- at B = 513 the only lane of the last tile -- rides along with the first odd candidate
    # (odd: it ignores nobody) that is checked and meets nobody else, so that it is that candidate's answer, at its
    # first instant
    first = hits_of_nobody()
    k0 = next(k for k in range(1, KEEP_K, 2) if n_segs[k] > 0 and first[k] == -1)
    rc[:, :, :, B - 1], rd[:, B - 1], rs[B - 1] = c[:, :, :, k0], dts[:, k0], n_segs[k0]
    case["t0"][B - 1], case["r_b"][B - 1], case["rider"] = case["t_start"][k0], 0.25, k0
    nobody = hits_of_nobody()
    ignore = np.full(KEEP_K, -1, np.int32)
    for k in range(0, KEEP_K, 2):
        if nobody[k] >= 0:
            ignore[k] = case["group"][nobody[k] & 0xffffffff]
    case["ignore"], case["nobody"] = ignore, nobody
    return case
