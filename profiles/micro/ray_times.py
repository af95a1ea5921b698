"""Times of the device ray trace (include/mplx_ray.h) at user size.

    python profiles/micro/ray_times.py measure OUT.json    # device-event times (GPU box); writes profiles/ray_times.json by default
    python profiles/micro/ray_times.py trace [query|goal]  # a few calls per case, for a kernel trace or a counter run of its own:
        rocprofv3 --kernel-trace --stats -d DIR -o r -- python profiles/micro/ray_times.py trace
        rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU -d DIR -o c -- python profiles/micro/ray_times.py trace query

Query: 65 536 rays on C4's map (512^3, res 0.1), `short` rays (p2 within 0.5 m of p1 on every axis: the regime of the
goal test) and `cross` rays (both ends uniform in the map), for lanes 4 / 16 / 64 and the automatic rule, with and
without the cell lists.  rays/s and steps/s: the steps are counted by the numpy restatement (tests/ray_model.py), which
the results are also compared with.  The reference's own rayTrace on one host thread over the same rays:
tests/golden/make_ray_golden.py --time.

Goal pass: C4's frontier and lists (65 536 nodes x 729 controls), the goal at a frontier node's position, flags from
the expansion launch; mplx_goal_sight_device against the expansion launch itself and against what the commit before
could do: copy the position rows and the flag row to the host (`host_copy_ms`, wall clock of the downloads) and trace
there (`host_model_ms`: the numpy restatement over the candidates, NOT host_planner.hpp's loop -- a stand-in).

measure: one warm-up + 7 repetitions, median; mplx_timer_begin / _end (events on the context's stream).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_RAYS, REPS = 65536, 7
MD, ORG, RES = [512] * 3, [0.0] * 3, 0.1


def query_rays(kind, n=N_RAYS):
    rng = np.random.default_rng(515 + (kind == "cross"))
    p1 = rng.uniform(0.0, 51.2, size=(n, 3))
    p2 = rng.uniform(0.0, 51.2, size=(n, 3)) if kind == "cross" else p1 + rng.uniform(-0.5, 0.5, size=(n, 3))
    return p1, p2


def c4_map():
    import motion_primitive_library_amd.workloads as W
    return W.box_map(MD, RES, 0.15, 1004)  # C4's map (workloads.make("C4"))


def timed(env, fn, reps=REPS):
    ms = []
    for r in range(reps + 1):  # the first is the warm-up
        env.timer_begin()
        fn()
        t = env.timer_end()
        env.synchronize()
        if r:
            ms.append(t)
    return float(np.median(ms)), ms


def measure_query(res):
    import motion_primitive_library_amd as m
    import ray_model as R
    from motion_primitive_library_amd.env import DeviceArray
    grid = c4_map().ravel()
    env = m.EnvMap(3, 0)
    env.setMap(ORG, MD, grid, RES)
    res["device"] = env.device_info()[0]
    for kind in ("short", "cross"):
        p1, p2 = query_rays(kind)
        model = R.ray_trace(grid, MD, ORG, RES, p1, p2)
        steps, cap = int(model["steps"].sum()), int(model["n_cells"].max())
        d1, d2 = DeviceArray(env, p1.nbytes), DeviceArray(env, p2.nbytes)
        d1.upload(np.ascontiguousarray(p1.T))
        d2.upload(np.ascontiguousarray(p2.T))
        rec = {"rays": N_RAYS, "steps": steps, "cells": int(model["n_cells"].sum()), "longest_list": cap,
               "hit_share": float(((model["status"] & R.HIT) > 0).mean()), "lanes": {}}
        for with_cells in (False, True):
            out = env.alloc_rays(N_RAYS, cap if with_cells else 0)
            for lanes in (4, 16, 64, 0):
                med, all_ms = timed(env, lambda: env.ray_trace_resident(d1, d2, out, lanes=lanes))
                got = out.download()
                ok = bool(np.array_equal(got["n_cells"], model["n_cells"]) and np.array_equal(got["first_hit"], model["first_hit"])
                          and np.array_equal(got["status"] & 7, model["status"]))
                if with_cells:
                    ok = ok and bool(np.array_equal(got["cells"], R.cells_matrix(model, cap, 0)[0]))
                rec["lanes"]["%s%s" % ("auto" if lanes == 0 else lanes, "+cells" if with_cells else "")] = {
                    "ms": med, "ms_all": all_ms, "rays_per_s": N_RAYS / (med * 1e-3), "steps_per_s": steps / (med * 1e-3),
                    "equals_model": ok}
            out.free()
        res["query"][kind] = rec
        print(kind, json.dumps(rec), flush=True)
    env.close()


def goal_setup():
    import motion_primitive_library_amd as m
    wl = m.workloads.make("C4")
    env = m.EnvMap(wl.dim, 0)
    wl.apply(env)
    fr = env.upload_frontier(wl.nodes)
    goal = np.zeros(4 * wl.dim + 2)
    goal[:wl.dim] = wl.nodes[:wl.dim, wl.n_nodes // 2]  # inside the frontier
    env.set_goal(goal, tol_pos=0.5)
    lists = env.alloc_lists(wl.n_nodes, want_state=True, want_flags=True)
    return m, wl, env, fr, goal, lists


def measure_goal(res):
    import ray_model as R
    m, wl, env, fr, goal, lists = goal_setup()
    D = wl.dim
    expand_ms, _ = timed(env, lambda: env.expand_lists_resident(fr, lists), reps=3)
    sight_ms, sight_all = timed(env, lambda: env.goal_sight(lists))
    t0 = time.perf_counter()
    flags = lists.flags.download(np.uint8, (lists.n_slots,))
    pos = np.stack([lists.state.download(np.float64, (lists.n_slots,), r * lists.state_stride * 8) for r in range(D)])
    count = lists.count.download(np.int32, (lists.n_nodes,))
    copy_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    live = (np.arange(lists.stride)[None, :] < count[:, None]).ravel()
    cand = np.nonzero(live & ((flags & 1) > 0))[0]
    p1 = np.ascontiguousarray(pos[:, cand].T)
    model = R.ray_trace(np.asarray(wl.grid).ravel(), wl.map_dim, wl.origin, wl.res, p1, np.broadcast_to(goal[:D], p1.shape))
    model_ms = (time.perf_counter() - t0) * 1e3
    blocked = (model["status"] & R.HIT) > 0
    ok = bool(np.array_equal((flags[cand] & 8) > 0, blocked) and not (flags[np.setdiff1d(np.arange(flags.size), cand)] & 8).any())
    res["goal"] = {"nodes": int(wl.n_nodes), "slots": int(lists.n_slots), "emitted": int(count.sum()), "candidates": int(cand.size),
                   "blocked": int(blocked.sum()), "goal_sight_ms": sight_ms, "goal_sight_ms_all": sight_all, "expand_lists_ms": expand_ms,
                   "share_of_expansion": sight_ms / expand_ms, "host_copy_ms": copy_ms, "host_model_ms": model_ms,
                   "equals_model": ok}
    print("goal", json.dumps(res["goal"]), flush=True)
    env.close()


def measure(path):
    res = {"repetitions": REPS, "query": {}}
    measure_query(res)
    measure_goal(res)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def trace(which):
    import motion_primitive_library_amd as m
    from motion_primitive_library_amd.env import DeviceArray
    if "query" in which:
        env = m.EnvMap(3, 0)
        env.setMap(ORG, MD, c4_map().ravel(), RES)
        for kind in ("short", "cross"):
            p1, p2 = query_rays(kind)
            d1, d2 = DeviceArray(env, p1.nbytes), DeviceArray(env, p2.nbytes)
            d1.upload(np.ascontiguousarray(p1.T))
            d2.upload(np.ascontiguousarray(p2.T))
            out = env.alloc_rays(N_RAYS, 0)
            for lanes in (4, 16, 64):
                for _ in range(3):
                    env.ray_trace_resident(d1, d2, out, lanes=lanes)
                    env.synchronize()
            print("trace ok: query", kind, "mean cells %.2f" % out.download()["n_cells"].mean(), flush=True)
        env.close()
    if "goal" in which:
        m, wl, env, fr, goal, lists = goal_setup()
        env.expand_lists_resident(fr, lists)
        for _ in range(3):
            env.goal_sight(lists)
            env.synchronize()
        print("trace ok: goal", flush=True)
        env.close()


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "measure"
    if cmd == "measure":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ray_times.json"))
    elif cmd == "trace":
        trace(sys.argv[2:] or ["query", "goal"])
    else:
        raise SystemExit(__doc__)
