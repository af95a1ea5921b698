"""What the body checks cost (include/mplx_body.h).

    python profiles/micro/body_times.py measure [OUT.json]   # GPU box; default profiles/body_times.json

(a) the grid build (mplx_body_fill_device: box, grid, count, scan, scatter) for 10^3, 10^5 and 10^6 points, uniform in a
    cube whose side keeps about 0.04 points per cell of the body r = 0.3, h = 0.1 (the 10^3 cloud: a 10 m cube).  A
    timed window is CALLS = 20 back-to-back fills between timer_begin / timer_end after one untimed fill; the figure is
    the window over CALLS, the median of REPS = 5 windows.
(b) the list check of 4093 rows x 81 entries (3-D ACCxYAW, {-1, 0, 1}^3 x three yaw rates, every entry live, parents
    uniform in the cloud's cube) at n_samp = 4 and 8 against those clouds, beside the expansion of the same 4093 parents.
    A check turns the entries it blocks to +inf, which a second check would skip: the cost row is uploaded again before
    every timed call and a window is ONE call (so the figure carries one launch's fixed cost); the median of REPS = 5.
    profiles/reserve_times.json has the relax (0.076 ms) and the reservation check (0.10 ms at 64 reservations) of a
    round of this size.
(c) the set check of K = 64 and K = 4096 solved five-waypoint trajectories at step = 0.05 against the 10^5 cloud (a
    stand-in for the pair set of a 64-query shortcut, which is 64 x (w_max - 1) x max_hop short problems).
(d) the slit search of tests/body_cases.py (flat body) and the corridor search with the map's occupied cells as the
    cloud (r = h = 0.2), beside the same searches with body=None, which issue the calls of the parent commit; status,
    cost, rounds and expansions of each are recorded.  Host clock around each search, the median of REPS = 5 after one untimed run.
Nothing here asserts a time.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, CALLS = 5, 20
ROWS = 4093
R, H = 0.3, 0.1


def med(xs):
    return float(np.median(xs))


def windows(env, fn, calls=CALLS, before=None):
    fn()
    env.synchronize()
    out = []
    for _ in range(REPS):
        if before:
            before()
            env.synchronize()
        env.timer_begin()
        for _ in range(calls):
            fn()
        out.append(env.timer_end() / calls)
    return out


def host_clock(env, fn):
    fn()
    out = []
    for _ in range(REPS):
        env.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def lists_and_clouds(m):
    U = m.workloads.grid_controls([-1.0, 0.0, 1.0], 3, yaw_rates=[-0.3, 0.0, 0.3])
    env = m.EnvMap(3)
    env.setMap([0.0] * 3, [128] * 3, np.zeros(128 ** 3, np.int8), 1.0)
    env.set_control(m.ACCxYAW)
    env.set_u(U)
    env.set_v_max(3.0)
    env.set_a_max(3.0)
    env.set_dt(1.0)
    rng = np.random.default_rng(5)
    out = {"rows": ROWS, "controls": len(U), "r": R, "h": H}
    body = env.alloc_body(R, H)
    for n in (1000, 100000, 1000000):
        side = max(10.0, (n / 0.04) ** (1.0 / 3.0) * 0.3)
        pts = rng.uniform(1.0, 1.0 + side, size=(n, 3))
        d_pts = m.DeviceArray(env, pts.nbytes)
        d_pts.upload(pts)
        build = windows(env, lambda: body.fill_resident(d_pts, n))
        sh = body.shape()
        rec = {"side_m": side, "cells": sh["cells"].tolist(), "edge": sh["edge"], "build_ms": med(build), "build_ms_all": build}
        F = env.n_fields
        pst = np.zeros((F, ROWS))
        pst[:3] = rng.uniform(2.0, side, size=(3, ROWS))
        pst[3:6] = rng.uniform(-0.5, 0.5, size=(3, ROWS))
        fr = m.TableFrontier(env, ROWS)
        fr.id.upload(np.zeros(ROWS, np.int32))
        fr.state.upload(pst)
        L = m.Lists(env, ROWS, len(U), want_state=True)
        ex = windows(env, lambda: env.expand_lists_resident(fr, L, n_nodes=ROWS))
        rec["expand_ms"], rec["expand_ms_all"] = med(ex), ex
        count, action = np.full(ROWS, len(U), np.int32), np.tile(np.arange(len(U), dtype=np.int32), ROWS)
        cost = np.ones(ROWS * len(U))
        L.count.upload(count)
        L.action.upload(action)
        d_nb = m.DeviceArray(env, 8)
        for n_samp in (4, 8):
            d_nb.upload(np.zeros(1, np.int64))
            ms = windows(env, lambda: body.check(fr, L, ROWS, n_samp, n_blocked=d_nb), calls=1, before=lambda: L.cost.upload(cost))
            L.cost.upload(cost)
            d_nb.upload(np.zeros(1, np.int64))
            body.check(fr, L, ROWS, n_samp, n_blocked=d_nb)
            env.synchronize()
            rec["check_n_samp_%d" % n_samp] = {"ms": med(ms), "ms_all": ms, "entries": int(ROWS * len(U)),
                                               "blocked": int(d_nb.download(np.int64, (1,))[0])}
        if n == 100000:
            for K in (64, 4096):
                wp = rng.uniform(2.0, side, size=(3, 5, K))
                poly = env.solve_traj(wp, v=1.5, control=m.ACC)
                d_hit, d_n = m.DeviceArray(env, 8 * K), m.DeviceArray(env, 8)
                d_n.upload(np.zeros(1, np.int64))
                ms = windows(env, lambda: body.check_poly_resident(poly, 0.05, hit=d_hit, n_hit=d_n))
                hits = int((d_hit.download(np.int64, (K,)) != -1).sum())
                rec["check_poly_K%d" % K] = {"ms": med(ms), "ms_all": ms, "step": 0.05, "hit": hits,
                                             "mean_total_s": float(poly.info()["total_time"].mean())}
                for b in (d_hit, d_n, poly):
                    b.free()
        out["points_%d" % n] = rec
        for b in (d_pts, fr, L, d_nb):
            b.free()
    body.free()
    env.close()
    return out


def searches(m):
    import body_cases as BC
    from test_gpu_open import corridor_env
    out = {}
    sc = BC.slit(m)
    env = BC.slit_env(m, sc)
    flat = env.alloc_body(*BC.FLAT)
    flat.fill(sc["cloud"])
    kw = dict(capacity=1 << 14, max_frontier=BC.CAP, sight=False, tol_pos=sc["tol_pos"])

    def run(e, a, b, keep, **k):
        r = e.search(a, b, **k)
        keep[:] = [m.search.STATUS_NAMES[r.status], r.cost, r.rounds, r.expanded]
        r.free()
    for name, body in (("body", flat), ("plain", None)):
        keep = []
        ms = host_clock(env, lambda: run(env, sc["start"], sc["goal"], keep, body=body, body_samples=BC.N_SAMP, **kw))
        out["slit_" + name] = {"ms": med(ms), "ms_all": ms, "status": keep[0], "cost": keep[1], "rounds": keep[2], "expanded": keep[3]}
    flat.free()
    env.close()
    env, start, goal = corridor_env(m)
    body = env.alloc_body(0.2, 0.2)
    body.fill_map()
    out["corridor_cloud_points"] = body.shape()["n"]
    for name, b in (("body", body), ("plain", None)):
        keep = []
        ms = host_clock(env, lambda: run(env, start, goal, keep, body=b, capacity=1 << 15, max_frontier=4096))
        out["corridor_" + name] = {"ms": med(ms), "ms_all": ms, "status": keep[0], "cost": keep[1], "rounds": keep[2], "expanded": keep[3]}
    body.free()
    env.close()
    return out


def main():
    import motion_primitive_library_amd as m
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "body_times.json")
    out = {"repetitions": REPS, "calls_per_window": CALLS, "lists": lists_and_clouds(m), "searches": searches(m)}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "measure":
    main()
