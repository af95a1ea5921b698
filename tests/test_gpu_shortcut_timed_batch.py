"""The timed shortcut (mplx_shortcut_timed[_device], include/mplx_reserve_poly.h) at many queries: the batch of
tests/test_gpu_shortcut.py -- Q = 67, w_max = 6, max_hop = 3, 1005 pairs, n_wp = k % 8, eight configurations -- against the
tables and per-query rows of tests/shortcut_timed_cases.py (B = 65 PARK, B = 300 GONE; t0, radius and ignored group vary
with k; a horizon that some hops and some chains leave).  tests/test_shortcut_timed_cases.py asserts on the CPU that the
reference alone blocks, reroutes and reports enough for the comparisons here to mean something.

Per case (configuration, B, max_hop) the device runs EnvMap.shortcut once without and once with the table (run()); the
tests read it, everything bit for bit:
  (a) test_batch_hits_and_costs  the timed call's pair set is the untimed one's (status, durations, coefficients); with
        the pair rows built on the host (t0[k] + t_i, one IEEE add) check_poly of the pair set equals
        reserve_poly_model.check fed the device's own samples of the pairs and the table's own positions; and
        edge_cost == admit(untimed edge_cost, hit) for all 1005 pairs, against the device's own untimed costs.
  (b) test_batch_programme       status, keep, n_keep, cost, chain_cost are shortcut_model.dp on the masked matrix, chain_hit
        is reserve_poly_model.chain_hit of the query's own pairs; EMPTY queries report -1, BAD_CHAIN keeps the identity.
  (c) test_batch_result          the result set's n_segs and 25 samples are those of EnvMap.load_traj of the chosen pairs.
max_hop = 1 (nothing non-adjacent to mask, chain_hit still reported) and max_hop = 5 run on ACC 2-D, B = 65.
Raw ABI (ACC, 2-D): the host twin with stride 71, keep_stride 73, poisoned outputs and a chain_hit row five entries
longer than Q against the device form with the same strides, with and without n_wp; every optional output NULL; two calls
on one pair of polys with different Q and hop, then the first again.  Search layer: MultiSearchResult.shortcut(avoid=) and
smooth(timed=True, avoid=) with three delay candidates against EnvMap.shortcut / check_poly of each query's own chain."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import reserve_poly_model as RPM
import shortcut_model as XM
import shortcut_timed_cases as TC
from test_gpu_shortcut import CONFIGS, N_SAMPLES, POISON, HeldPairs, batch_env, chosen_segments, poison, same_bytes
from test_gpu_solve import same_bits

pytestmark = pytest.mark.gpu

Q, WMAX, HOP = XM.Q, XM.WMAX, XM.HOP
CASES = [(name, B, HOP) for name in CONFIGS for B in TC.BS] + [("acc-2d", 65, 1), ("acc-2d", 65, 5)]
IDS = ["%s-B%d-hop%d" % c for c in CASES]
ROWS = ("status", "n_keep", "keep_rows", "cost", "chain_cost", "edge_cost", "chain_hit")
_RUNS = {}


def make_table(m, env, D, B, control):
    """(Reservations, the PolyTrajSet it was filled from) of shortcut_timed_cases.reservations(D, B)."""
    r = TC.reservations(D, B)
    c, dts, n_segs = r["res"]
    rp = env.load_traj(c, dts, n_segs=n_segs, control=control)
    assert (rp.status[n_segs == 0] == m.SOLVE_EMPTY).all() and (rp.status[n_segs > 0] == 0).all()
    return env.alloc_reservations(rp, TC.STEP, n_steps=TC.N_STEPS[D], t0=r["t0"], radius=r["r_b"], group=r["group"], park=r["park"]), rp


def model_hits(pairs, table, D, rows):
    """reserve_poly_model.check of a device pair set from its own samples and the table's own positions: hit [P]."""
    ts, rad, ign = rows
    info = pairs.info()
    tl = np.arange(table.n_steps)[None, :] * np.float64(TC.STEP) - ts[:, None]
    pos = pairs.sample(times=np.ascontiguousarray(tl))["samples"][:D]
    hit, _, _ = RPM.check(info["status"], info["n_segs"], info["total_time"], ts, rad, ign, TC.STEP, table.positions(),
                          lambda k, i, t: pos[:, k, i])
    return hit


def run(m, name, B, hop):
    """Both shortcuts of one case, everything the tests read brought to the host, the device objects freed."""
    key = (name, B, hop)
    if key not in _RUNS:
        D, control = CONFIGS[name]
        b = XM.batch(D, control)
        env = batch_env(m, D, control)
        table, rp = make_table(m, env, D, B, control)
        t0, radius, ignore = TC.query_rows(D, B)
        plain = env.shortcut(b["states"], n_wp=b["n_wp"], control=control, max_hop=hop)
        timed = env.shortcut(b["states"], n_wp=b["n_wp"], control=control, max_hop=hop, avoid=table, t0=t0, radius=radius,
                             ignore_group=ignore)
        out = {k: getattr(timed, k) for k in ROWS}
        out["keep"] = [k.tolist() for k in timed.keep]
        out["pairs"], out["plain_pairs"] = HeldPairs(timed.pairs), HeldPairs(plain.pairs)
        out["plain"] = {k: getattr(plain, k) for k in ROWS[:-1]}
        assert plain.chain_hit is None
        rows = TC.pair_rows(b["states"][4 * D + 1], t0, radius, ignore, hop)
        out["hit"] = table.check_poly(timed.pairs, *rows)["hit"]
        out["model_hit"] = model_hits(timed.pairs, table, D, rows)
        out["poly"] = {"status": timed.poly.status.copy(), "n_segs": timed.poly.n_segs.copy(),
                       "samples": timed.poly.sample(N=N_SAMPLES)["samples"]}
        coeff, durs, n_segs = chosen_segments(D, out["keep"], out["pairs"], WMAX, hop)
        twin = env.load_traj(coeff, durs, n_segs=n_segs, control=control)
        out["twin"] = {"status": twin.status.copy(), "n_segs": n_segs, "samples": twin.sample(N=N_SAMPLES)["samples"]}
        for x in (twin, plain, timed, table, rp):
            x.free()
        env.close()
        _RUNS[key] = out
    return _RUNS[key]


@pytest.mark.parametrize("name,B,hop", CASES, ids=IDS)
def test_batch_hits_and_costs(engine, name, B, hop):
    """(a) of the module's docstring."""
    r = run(engine, name, B, hop)
    NP = Q * (WMAX - 1) * hop
    a, p = r["pairs"], r["plain_pairs"]
    assert a.n == NP and np.array_equal(a.status, p.status)
    same_bits(a.dts(), p.dts(), "pair durations")
    same_bits(a.coefficients(), p.coefficients(), "pair coefficients")
    same_bits(a.yaw_coefficients(), p.yaw_coefficients(), "pair yaw coefficients")
    assert np.array_equal(r["hit"], r["model_hit"]), np.nonzero(r["hit"] != r["model_hit"])[0]
    hit = r["hit"].reshape(Q, WMAX - 1, hop)
    plain = r["plain"]["edge_cost"]
    assert r["edge_cost"].shape == plain.shape == (Q, WMAX - 1, hop)
    for k in range(Q):
        same_bits(r["edge_cost"][k], RPM.admit(plain[k], hit[k]), "masked edge costs of query %d" % k)
    admitted = np.isfinite(plain) & (a.status == 0).reshape(plain.shape)
    admitted[:, :, 0] = False
    blocked, horizon = int((admitted & (hit != -1)).sum()), int((admitted & (hit == -2)).sum())
    big = int(((hit >= 0) & ((hit & 0xffffffff) >= 256)).sum())
    print("%s B=%d hop=%d: %d admitted non-adjacent hops, %d blocked, %d of them by the horizon; %d hits with a partner >= 256" % (
        name, B, hop, admitted.sum(), blocked, horizon, big))
    if hop == HOP:  # (the conditions tests/test_shortcut_timed_cases.py holds the reference to, on the device's own hits)
        assert 0.15 * admitted.sum() <= blocked <= 0.70 * admitted.sum() and horizon >= 2
        assert B < 256 or big >= 10


@pytest.mark.parametrize("name,B,hop", CASES, ids=IDS)
def test_batch_programme(engine, name, B, hop):
    """(b) of the module's docstring."""
    m = engine
    D, control = CONFIGS[name]
    b, r = XM.batch(D, control), run(engine, name, B, hop)
    n_wp, c = b["n_wp"], r["edge_cost"]
    hit = r["hit"].reshape(Q, WMAX - 1, hop)
    live, changed, kinds = 0, 0, {"hit": 0, "horizon": 0, "clear": 0}
    for k in range(Q):
        W = XM.w_of(n_wp, k)
        status, keep, cost, chain = XM.dp(c[k], W, hop)
        assert r["status"][k] == status and r["keep"][k] == keep and r["n_keep"][k] == len(keep), (k, r["keep"][k], keep)
        assert r["keep_rows"][:len(keep), k].tolist() == keep and (r["keep_rows"][len(keep):, k] == -1).all(), k
        same_bits([r["cost"][k], r["chain_cost"][k]], [cost, chain], "cost and chain_cost of query %d" % k)
        assert r["chain_hit"][k] == RPM.chain_hit(hit[k], W), (k, r["chain_hit"][k], hit[k, :, 0])
        if k % 8 < 2:
            assert status == m.SOLVE_EMPTY and r["chain_hit"][k] == -1 and r["n_keep"][k] == 0 and np.isnan(r["cost"][k])
        elif k in XM.REPEAT_T:
            assert status == m.SHORTCUT_BAD_CHAIN and keep == list(range(W)) and np.isnan(r["cost"][k]) and np.isnan(r["chain_cost"][k])
        else:
            assert status == 0 and keep[0] == 0 and keep[-1] == W - 1 and r["cost"][k] <= r["chain_cost"][k], k
            assert r["cost"][k] >= r["plain"]["cost"][k], k
            live += 1
            changed += keep != [i for i in r["plain"]["keep_rows"][:, k].tolist() if i >= 0]
            kinds["hit" if r["chain_hit"][k] >= 0 else "horizon" if r["chain_hit"][k] == -2 else "clear"] += 1
    same_bits(r["chain_cost"], r["plain"]["chain_cost"], "chain_cost with and without the table")
    print("%s B=%d hop=%d: %d live queries, %d keep other states than without the table; chain_hit %s" % (name, B, hop, live, changed, kinds))
    assert live == 48 and kinds["hit"] >= 5 and kinds["horizon"] >= 1 and kinds["clear"] >= 5
    if hop == 1:
        assert changed == 0 and all(r["keep"][k] == list(range(XM.w_of(n_wp, k))) for k in range(Q) if k % 8 >= 2)
    else:
        assert 5 * changed >= live


@pytest.mark.parametrize("name,B,hop", CASES, ids=IDS)
def test_batch_result(engine, name, B, hop):
    """(c) of the module's docstring."""
    m = engine
    r = run(engine, name, B, hop)
    poly, twin = r["poly"], r["twin"]
    kept = 0
    for k in range(Q):
        if r["status"][k]:
            assert poly["status"][k] == m.SOLVE_EMPTY and poly["n_segs"][k] == 0 and not poly["samples"][:, k].any(), k
            continue
        S = len(r["keep"][k]) - 1
        assert poly["status"][k] == 0 and twin["status"][k] == 0 and poly["n_segs"][k] == S == twin["n_segs"][k], k
        same_bits(poly["samples"][:, k], twin["samples"][:, k], "samples of query %d" % k)
        kept += 1
    assert kept == 48


# ------------------------------------------------------------------------------------------------------ the raw ABI
RAW = ("status", "n_keep", "keep", "cost", "chain_cost", "edge_cost", "chain_hit")


def raw_timed(m, env, table, pairs, res, st, n_wp, control, hop, device, stride, keep_stride, outputs=True):
    """mplx_shortcut_timed (device=False) or mplx_shortcut_timed_device on outputs filled with the byte POISON; states
    padded to `stride` with NaN columns, the [Q] rows and the columns of keep `keep_stride` long, edge_cost eight entries
    and chain_hit five entries longer than what is written.  Returns (rows or None, the result poly's samples)."""
    A, L = m._abi, m._abi.lib()
    env._flush()
    Fd, W, n = st.shape
    P = n * (W - 1) * hop
    padded = np.full((Fd, W, stride), np.nan)
    padded[:, :, :n] = st
    ks = keep_stride
    shapes = {"status": ((ks,), np.uint8), "n_keep": ((ks,), np.int32), "keep": ((W, ks), np.int32), "cost": ((ks,), np.float64),
              "chain_cost": ((ks,), np.float64), "edge_cost": ((P + 8,), np.float64), "chain_hit": ((n + 5,), np.int64)}
    host = {key: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, POISON, np.uint8).view(dt).reshape(shape)
            for key, (shape, dt) in shapes.items()}
    i, o = A.ShortcutIn(), A.ShortcutOut()
    i.n_query, i.w_max, i.control, i.stride, i.max_hop = n, W, control, stride, hop
    o.keep_stride = ks if outputs else 0
    bufs = {}
    try:
        if device:
            for key, arr in [("states", padded)] + ([("n_wp", np.ascontiguousarray(n_wp, np.int32))] if n_wp is not None else []):
                bufs[key] = m.DeviceArray(env, arr.nbytes)
                bufs[key].upload(arr)
                setattr(i, key, bufs[key].ptr)
            for key in RAW if outputs else ():
                bufs[key] = m.DeviceArray(env, host[key].nbytes)
                A.check(env._ctx, L.mplx_memset(env._ctx, bufs[key].ptr, POISON, host[key].nbytes))
                if key != "chain_hit":
                    setattr(o, key, bufs[key].ptr)
            A.check(env._ctx, L.mplx_shortcut_timed_device(pairs._h, res._h, C.byref(i), C.byref(o), table._res,
                                                           bufs["chain_hit"].ptr if outputs else None))
            env.synchronize()
            for key in RAW if outputs else ():
                host[key] = bufs[key].download(shapes[key][1], shapes[key][0])
        else:
            i.states = padded.ctypes.data
            if n_wp is not None:
                n_wp = np.ascontiguousarray(n_wp, np.int32)
                i.n_wp = n_wp.ctypes.data
            for key in RAW[:-1] if outputs else ():
                setattr(o, key, host[key].ctypes.data)
            A.check(env._ctx, L.mplx_shortcut_timed(pairs._h, res._h, C.byref(i), C.byref(o), table._res,
                                                    host["chain_hit"].ctypes.data if outputs else None))
    finally:
        for buf in bufs.values():
            buf.free()
    res.n, res.n_wmax, res.control = n, W, control
    return (host if outputs else None), res.sample(N=N_SAMPLES)["samples"]


def assert_raw_equal(rows, want, n, P, what):
    """rows: raw_timed's, with strides; want: dict of compact rows ([n], keep [W][n], edge_cost [P]) or raw rows."""
    for key in RAW:
        got = rows[key]
        cut = P if key == "edge_cost" else n
        body, tail = (got[:cut], got[cut:]) if got.ndim == 1 else (got[:, :n], got[:, n:])
        w = want[key]
        w = (w[:cut] if w.ndim == 1 else w[:, :n])
        assert same_bytes(body, w), (what, key)
        assert tail.size > 0 and poison(tail), (what, key, "the padding was written")


def test_raw_strides_and_untouched_memory(engine):
    """The host twin of the timed shortcut (on the staging arena) and the device form on the ACC 2-D batch, B = 65, with
    stride 71, keep_stride 73, poisoned outputs and a chain_hit row five entries longer than Q: with n_wp both are bit
    for bit what EnvMap.shortcut(avoid=) returned (run()); without n_wp (every query W = 6) the twin is the device form;
    the padding is untouched; with every optional output NULL both give the same result trajectories."""
    m = engine
    D, control = CONFIGS["acc-2d"]
    b, want = XM.batch(D, control), run(engine, "acc-2d", 65, HOP)
    NP = Q * (WMAX - 1) * HOP
    compact = {"status": want["status"], "n_keep": want["n_keep"], "keep": want["keep_rows"], "cost": want["cost"],
               "chain_cost": want["chain_cost"], "edge_cost": want["edge_cost"].reshape(-1), "chain_hit": want["chain_hit"]}
    env = batch_env(m, D, control)
    table, rp = make_table(m, env, D, 65, control)
    table.set_queries(*TC.query_rows(D, 65))
    pairs, res = env.alloc_poly(NP, 2), env.alloc_poly(Q, WMAX)
    got = {}
    for device in (True, False):
        for n_wp in (b["n_wp"], None):
            rows, samples = raw_timed(m, env, table, pairs, res, b["states"], n_wp, control, HOP, device, 71, 73)
            got[(device, n_wp is None)] = (rows, samples)
        none, samples = raw_timed(m, env, table, pairs, res, b["states"], b["n_wp"], control, HOP, device, 71, 73, outputs=False)
        assert none is None and same_bytes(samples, got[(device, False)][1]), "every optional output NULL, device=%s" % device
    for device in (True, False):
        assert_raw_equal(got[(device, False)][0], compact, Q, NP, "with n_wp, device=%s" % device)
        assert same_bytes(got[(device, False)][1], want["poly"]["samples"])
    full = got[(True, True)][0]
    assert full["status"][:Q].tolist() == [m.SHORTCUT_BAD_CHAIN if k in XM.REPEAT_T else 0 for k in range(Q)] and (full["n_keep"][:Q] >= 2).all()
    assert (full["chain_hit"][:Q] >= 0).sum() >= 10 and (full["chain_hit"][:Q] == -2).any() and (full["chain_hit"][:Q] == -1).any()
    assert_raw_equal(got[(False, True)][0], full, Q, NP, "without n_wp: the host twin against the device form")
    assert same_bytes(got[(False, True)][1], got[(True, True)][1])
    for x in (pairs, res, table, rp):
        x.free()
    env.close()


def test_raw_reuse_of_the_polys(engine):
    """One pair poly and one result poly through the batch (Q = 67, max_hop 3), then queries 2 .. 6 with max_hop = 5 and
    five queries set on the table, then the batch again: call 3 is call 1 bit for bit, call 2 is the same call on fresh
    polys, and call 1 is EnvMap.shortcut(avoid=)."""
    m = engine
    D, control = CONFIGS["acc-2d"]
    b, want = XM.batch(D, control), run(engine, "acc-2d", 65, HOP)
    st, n_wp = b["states"], b["n_wp"]
    st2, n_wp2 = np.ascontiguousarray(st[:, :, 2:7]), n_wp[2:7]
    t0, radius, ignore = TC.query_rows(D, 65)
    env = batch_env(m, D, control)
    table, rp = make_table(m, env, D, 65, control)
    pairs, res = env.alloc_poly(Q * (WMAX - 1) * HOP, 2), env.alloc_poly(Q, WMAX)

    def big():
        table.set_queries(t0, radius, ignore)
        return raw_timed(m, env, table, pairs, res, st, n_wp, control, HOP, True, 71, 73)

    def small(ps, rs):
        table.set_queries(t0[2:7], radius[2:7], ignore[2:7])
        return raw_timed(m, env, table, ps, rs, st2, n_wp2, control, 5, True, 7, 9)

    one, two, three = big(), small(pairs, res), big()
    fresh_pairs, fresh_res = env.alloc_poly(125, 2), env.alloc_poly(5, WMAX)
    fresh = small(fresh_pairs, fresh_res)
    for got, ref, what in ((three, one, "the batch again"), (two, fresh, "the small call")):
        for key in RAW:
            assert same_bytes(got[0][key], ref[0][key]), (what, key)
        assert same_bytes(got[1], ref[1]), (what, "samples")
    assert same_bytes(one[0]["chain_hit"][:Q], want["chain_hit"]) and same_bytes(one[0]["edge_cost"][:want["edge_cost"].size], want["edge_cost"].reshape(-1))
    # the small call is queries 2 .. 6 of the hop-5 case: the same chains, their own t0 / radius / ignored group
    hop5 = run(engine, "acc-2d", 65, 5)
    rows = two[0]
    assert same_bytes(rows["chain_hit"][:5], hop5["chain_hit"][2:7])
    assert same_bytes(rows["edge_cost"][:125].reshape(5, 5, 5), hop5["edge_cost"][2:7])
    assert np.array_equal(rows["keep"][:, :5], hop5["keep_rows"][:, 2:7])
    for x in (pairs, res, fresh_pairs, fresh_res, table, rp):
        x.free()
    env.close()


# --------------------------------------------------------------------------------------------------- the search layer
def compare_queries(m, env, T1, multi, table, delays, what):
    """MultiSearchResult.shortcut(avoid=table) and smooth(timed=True, avoid=table) of `multi`, whose queries started at
    `delays`, per query against EnvMap.shortcut of the query's own chain with its own delay and against check_poly of
    its own solve; a query without a path is SOLVE_EMPTY with chain_hit -1.  Returns how many of the queries with a
    delay other than query 0's give another timed shortcut (edge costs or chain_hit) when started at query 0's delay:
    the queries that show that t0 is read per query."""
    n = len(delays)
    found = list(multi.found)
    lengths = [len(multi.full_path(q)[1]) + 1 if found[q] else 0 for q in range(n)]
    hop = max(lengths) - 1  # (one max_hop for the batch and for each query alone: the default is the call's own w_max - 1)
    sc = multi.shortcut(max_hop=hop, avoid=table)
    sm = multi.smooth(timed=True, avoid=table)
    assert sc.edge_cost.shape == (n, hop, hop)
    all_samples = sc.poly.sample(N=N_SAMPLES)["samples"]
    sensitive = 0
    for q in range(n):
        if not found[q]:
            assert sc.status[q] == m.SOLVE_EMPTY and sc.chain_hit[q] == -1 and sc.n_keep[q] == 0, (what, q)
            assert sm.status[q] == m.SOLVE_EMPTY and sm.reserve_hit["hit"][q] == -1, (what, q)
            continue
        states = T1.chain_states(env, multi.full_path(q))
        W = lengths[q]
        assert states.shape[1] == W
        one = env.shortcut(states, max_hop=hop, avoid=table, t0=delays[q], radius=T1.R)
        assert one.status[0] == 0 and sc.status[q] == 0 and sc.keep[q].tolist() == one.keep[0].tolist(), (what, q)
        assert sc.chain_hit[q] == one.chain_hit[0], (what, q, sc.chain_hit[q], one.chain_hit[0])
        same_bits([sc.cost[q], sc.chain_cost[q]], [one.cost[0], one.chain_cost[0]], "%s: costs of query %d" % (what, q))
        same_bits(sc.edge_cost[q, :W - 1], one.edge_cost[0], "%s: edge costs of query %d" % (what, q))
        assert sc.poly.n_segs[q] == one.poly.n_segs[0]
        same_bits(all_samples[:, q], one.poly.sample(N=N_SAMPLES)["samples"][:, 0], "%s: samples of query %d" % (what, q))
        if delays[q] != delays[0]:
            other = env.shortcut(states, max_hop=hop, avoid=table, t0=delays[0], radius=T1.R)
            sensitive += int(other.chain_hit[0] != one.chain_hit[0] or not same_bytes(other.edge_cost, one.edge_cost))
            other.free()
        one.free()
        t = states[-1, :, 0]
        same_bits(sm.dts()[:W - 1, q], t[1:] - t[:-1], "%s: segment times of query %d" % (what, q))
        # smooth(timed=True, avoid=): the hit of this query is check_poly of its own solve at its own delay
        alone = m.search._smooth_timed(env, [multi.full_path(q)], None, table, delays[q], T1.R, -1)
        assert alone.reserve_hit["hit"][0] == sm.reserve_hit["hit"][q], (what, q)
        alone.free()
    again = table.check_poly(sm, np.asarray(delays), T1.R, -1)
    assert np.array_equal(sm.reserve_hit["hit"], again["hit"]) and sm.reserve_hit["n_hit"] == again["n_hit"]
    print("%s: found %s, chain_hit %s, smooth hit %s, %d queries turn on their own t0" % (
        what, found, sc.chain_hit.tolist(), sm.reserve_hit["hit"].tolist(), sensitive))
    sc.free()
    sm.free()
    return sensitive


def test_multi_search_result_with_three_delays(engine):
    """The pocket lane of tests/test_gpu_shortcut_timed.py planned with delays (0, 1, 2) and keep=True: every robot's
    MultiSearchResult has three queries with their own t0.  Robots 1 and 2 against robot 0's reservation as planned and
    against robot 0 delayed (a stale table: a chain of robot 1 is hit); then a search_many on the lower lane whose second query
    runs out of rounds: a query without a path between two with one.  Across all of them at least two queries must turn
    on their own t0 (compare_queries), or the comparisons would hold with every query on query 0's clock."""
    import test_gpu_shortcut_timed as T1
    m = engine
    delays = (0.0, 1.0, 2.0)
    cells = np.full((9, 25), 100, np.int8)  # [y][x]: the scenario of test_gpu_shortcut_timed.scenario
    cells[3, :17] = 0
    cells[4:6, 9] = 0
    cells[7, :] = 0
    env = T1.lane_env(m, cells)
    wp = lambda p: m.Waypoint(2, m.ACC, pos=p).to_row()
    starts = np.stack([wp([1.5, 3.5]), wp([9.5, 3.5]), wp([23.5, 7.5])], axis=1)
    goals = np.stack([wp([15.5, 3.5]), wp([13.5, 3.5]), wp([1.5, 7.5])])
    kw = dict(wait=True, park_goal=True, capacity=1 << 17, max_frontier=4096, sight=False)
    plan = m.search.plan_prioritised(env, starts, goals, T1.STEP, T1.R, delays=delays, keep=True, n_steps=int(60 / T1.STEP), **kw)
    assert plan["status"] == [m.search.FOUND] * 3
    table = T1.table_of(env, plan, [0])
    stale = None
    for late in (2.0, 1.0, 3.0, 4.0, 5.0, 6.0):  # robot 0 delayed: the first delay at which a chain of robot 1 no longer holds
        stale = T1.table_of(env, plan, [0], t0=np.array([late]))
        sc = plan["results"][1].shortcut(avoid=stale)
        hits = sc.chain_hit.copy()
        sc.free()
        if (hits >= 0).any():
            break
        stale.free()
        stale = None
    assert stale is not None, "no delay of robot 0 makes a chain of robot 1 stale"
    print("robot 0 delayed by %.1f: chain_hit of robot 1's candidates %s" % (late, hits.tolist()))
    sensitive, checked = 0, 0
    for r in (1, 2):
        multi = plan["results"][r]
        if sum(multi.found) < 2:
            continue
        checked += 1
        sensitive += compare_queries(m, env, T1, multi, table, delays, "robot %d" % r)
        sensitive += compare_queries(m, env, T1, multi, stale, delays, "robot %d, robot 0 delayed" % r)
    assert checked >= 1, "no robot has two found delay candidates"
    # the lower lane: a goal two cells away, the far end (more than 16 rounds away), the near goal again
    near = wp([21.5, 7.5])
    multi = env.search_many(np.repeat(starts[:, 2:3], 3, axis=1), np.stack([near, goals[2], near]), avoid=table, t0=delays, radius=T1.R,
                            max_rounds=16, **kw)
    assert list(multi.found) == [True, False, True], multi
    sensitive += compare_queries(m, env, T1, multi, table, delays, "lower lane")
    multi.free()
    assert sensitive >= 2
    for x in (table, stale):
        x.free()
    for res in plan["results"]:
        res.free()
    env.close()
