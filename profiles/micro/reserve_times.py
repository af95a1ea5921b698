"""Time of one reservation check (include/mplx_reserve.h) next to the expansion and the relax of the round it joins, and
of a corridor search with and without `avoid`.

    python profiles/micro/reserve_times.py measure [OUT.json]   # GPU box; default profiles/reserve_times.json

Workload: 2-D, ACC, 81 controls (nine values per axis in [-1, 1]), dt = 1, an all-free 256 x 256 map of 0.25 m cells; a
frontier of 4096 distinct states with velocities in quarters within +-1 and t = (k mod 8) dt; lists of stride 96.
Reservations: B chains of 8 random primitives from random starts on the map, t0 in quarters from 0 to 2, PARK, step
0.25 (dt / step = 4: five instants per row), n_steps = 128.  Radii 0: nothing is blocked, so every call does the same,
full work -- every looked-at entry meets every included reservation at every one of its instants; pair_instants counts
exactly those.  (With radii that block, an entry stops at its first conflict and later calls find the blocked entries
already +inf: less work, and not the same work from call to call.)

A timed window is CALLS = 5 back-to-back device calls between mplx_timer_begin / _end (events on the context's stream)
after one untimed call; the figure is the window divided by CALLS, the median of REPS = 5 windows.  relax is timed on a
table that already holds the round's nodes (the first, untimed call created them).
Lanes: with 9 controls (stride 9) the default gives 16 lanes to a row's entries and four slices of the reservations;
MPLX_RESERVE_LANES=64 gives all 64 lanes to the entries (9 of them busy).  Both are timed.
The search: EnvMap.search on the corridor of tests/golden, robot 1 on the way back against robot 0's plan, by a host
clock, median of 3."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, REPS, CALLS, STEP, N_STEPS = 4096, 5, 5, 0.25, 128


def median(xs):
    return float(np.median(np.asarray(xs)))


def windows(env, call):
    call()
    env.synchronize()
    out = []
    for _ in range(REPS):
        env.timer_begin()
        for _ in range(CALLS):
            call()
        out.append(env.timer_end() / CALLS)
        env.synchronize()
    return out


def round_times(m, vals, stride, Bs, lanes_env=None):
    rng = np.random.default_rng(77)
    U = m.workloads.grid_controls(vals, 2)
    if lanes_env:  # (read once, when the context is created)
        os.environ["MPLX_RESERVE_LANES"] = lanes_env
    env = m.EnvMap(2)
    os.environ.pop("MPLX_RESERVE_LANES", None)
    env.setMap([0.0, 0.0], [256, 256], np.zeros(256 * 256, np.int8), 0.25)
    env.set_control(m.ACC)
    env.set_u(U)
    env.set_v_max(2.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    F = env.n_fields
    st = np.zeros((F, N))
    cells = rng.permutation(200 * 200)[:N]
    st[0], st[1] = 7.0 + (cells % 200) * 0.25, 7.0 + (cells // 200) * 0.25
    st[2:4] = rng.integers(-4, 5, (2, N)) / 4.0
    tab = env.alloc_table(N * stride + N)
    fr, imp = m.TableFrontier(env, N), m.TableFrontier(env, N * stride)
    n = tab.seed(st, frontier=fr)  # (a few of the 4096 states share a lattice hash: hash_combine is what it is)
    tt = fr.download(n)["state"]
    tt[F - 1] = (np.arange(n) % 8) * 1.0
    up = np.zeros((F, N))
    up[:, :n] = tt
    fr.state.upload(up)  # (the parents' times: the table keeps t = 0, which nothing below reads)
    lists = env.alloc_lists(N, want_state=True, stride=stride)
    out = {"controls": len(U), "stride": stride, "rows": n}
    out["expand_ms_all"] = windows(env, lambda: env.expand_lists_resident(fr, lists, n_nodes=n))
    out["expand_ms"] = median(out["expand_ms_all"])
    entries = int(lists.download()["count"][:n].sum())
    out["entries"] = entries
    for B in Bs:
        r_st = np.zeros((F, B))
        r_st[:2] = rng.uniform(7.0, 57.0, (2, B))
        r_ac = rng.integers(0, len(U), (8, B)).astype(np.int32)
        res = env.alloc_reservations((r_st, r_ac), STEP, n_steps=N_STEPS, t0=rng.integers(0, 9, B) / 4.0, radius=0.0)
        res.set_queries(0.0, 0.0)
        d_nb = m.DeviceArray(env, 8)
        d_nb.upload(np.zeros(1, np.int64))
        w = windows(env, lambda: res.check(fr, lists, n, n_blocked=d_nb))
        assert int(d_nb.download(np.int64, (1,))[0]) == 0
        pi = entries * 5 * B
        out["check_B%d" % B] = {"ms": median(w), "ms_all": w, "pair_instants": pi, "pair_instants_per_s": pi / (median(w) * 1e-3)}
        d_nb.free()
        res.free()
    out["relax_ms_all"] = windows(env, lambda: tab.relax(lists, fr.id, fr.g, frontier=imp, n_nodes=n, want_count=False))
    out["relax_ms"] = median(out["relax_ms_all"])
    for b in (lists, fr, imp, tab):
        b.free()
    env.close()
    return out


def corridor_search(m):
    from test_gpu_open import corridor_env
    from test_multi import corridor_queries
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    r0 = env.search(starts[:, 0], goals[0], capacity=1 << 15, max_frontier=4096)
    p = r0.path()
    res = env.alloc_reservations((p[0].reshape(-1, 1), p[1].reshape(-1, 1)), STEP, n_steps=640, radius=0.4)
    out = {}
    for name, kw in (("plain", {}), ("time_keys_only", dict(time_keys=True)), ("avoid", dict(avoid=res, radius=0.4))):
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            r = env.search(starts[:, 2], goals[2], capacity=1 << 18, max_frontier=4096, **kw)
            ts.append((time.perf_counter() - t) * 1e3)
            rec = {"status": r.status, "cost": r.cost, "rounds": r.rounds, "expanded": r.expanded, "nodes": r.table.stats()[0]}
            r.free()
        out[name] = dict(rec, wall_ms=median(ts), wall_ms_all=ts)
    res.free()
    r0.free()
    env.close()
    return out


def measure(path):
    import motion_primitive_library_amd as m
    nine = [-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0]
    res = {"repetitions": REPS, "calls_per_window": CALLS, "step": STEP, "n_steps": N_STEPS, "instants_per_row": 5}
    res["round_81"] = round_times(m, nine, 96, (1024, 64))
    res["round_9_lanes16x4"] = round_times(m, [-1.0, 0.0, 1.0], 9, (1024, 64))
    res["round_9_lanes64"] = round_times(m, [-1.0, 0.0, 1.0], 9, (1024, 64), lanes_env="64")
    res["corridor"] = corridor_search(m)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "measure":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reserve_times.json"))
    else:
        raise SystemExit(__doc__)
