"""Times of the open set of a node table (include/mplx_open.h), in one process:

    python profiles/micro/open_times.py measure OUT.json

For two problems -- the corridor of tests/golden (2D ACC, 9 controls) and the 3D plan problem of the bench (120^3 cells,
ACC, 729 controls; profiles/micro/plan3d_timing.py and table_times.py use the same one) --

  search       EnvMap.search end to end for delta in {0, w dt, 4 w dt} (eps 1, the ray trace on): wall clock around a
               call that ends in its last select's synchronise, with rounds, expansions and nodes beside it.
  push/select  one mplx_open_push_device over all nodes of the table that search left, and one select with delta = +inf
               into a frontier that takes them all: event times (mplx_timer_begin / _end on the context's stream).
  sweep        EnvMap.cost_to_come bounded by the cost the search found (the label-correcting sweep of the node table).
  plan         the host A* (MapPlanner.plan, bench.engine_plan) on the same problem.

One warm-up and REPS repetitions of everything, alternating the legs inside a repetition; medians and all samples are
reported.  Tables, frontiers and lists are allocated inside the timed search and sweep calls, as a user's call does.
Searches stop after 20 000 rounds at the latest (the status says so if one does)."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS = 5


def med(xs):
    return float(np.median(xs))


def corridor_problem(m):
    from test_plan_known_answer import corridor
    c = corridor()
    U = m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    return {"name": "corridor", "dim": 2, "origin": c["origin"], "md": c["dim"], "cells": np.asarray(c["cells"], np.int8), "res": c["res"],
            "U": U, "start": m.Waypoint(2, m.ACC, pos=c["start"]), "goal": m.Waypoint(2, m.ACC, pos=c["goal"]), "v_max": 1.0,
            "a_max": 1.0, "batch": 16, "capacity": 1 << 15, "max_frontier": 4096}


def plan3d_problem(m, edge=120):
    W = m.workloads
    r_ = 0.1
    flat = W.box_map([edge] * 3, r_, 0.08, 4242, side_m=(0.5, 2.5)).ravel()
    U3 = W.grid_controls(np.linspace(-2.0, 2.0, 9), 3)

    def free_near(p):
        cc = np.array([int(x / r_) for x in p])
        for r in range(0, 30):
            for d in np.ndindex(2 * r + 1, 2 * r + 1, 2 * r + 1):
                q = cc + np.array(d) - r
                if np.all(q >= 0) and np.all(q < edge) and flat[q[0] + edge * (q[1] + edge * q[2])] == 0:
                    return [(q[i] + 0.5) * r_ for i in range(3)]
        raise RuntimeError("no free cell")

    s3 = m.Waypoint(3, m.ACC, pos=free_near([1.0, 1.0, 1.0]))
    g3 = m.Waypoint(3, m.ACC, pos=free_near([edge * r_ - 1.0, edge * r_ - 1.2, edge * r_ - 1.5]))
    return {"name": "plan3d_%d" % edge, "dim": 3, "origin": [0.0] * 3, "md": [edge] * 3, "cells": flat, "res": r_, "U": U3, "start": s3,
            "goal": g3, "v_max": 2.0, "a_max": 2.0, "batch": 64, "capacity": 1 << 23, "max_frontier": 1 << 13}


def make_env(m, p):
    env = m.EnvMap(p["dim"])
    env.setMap(p["origin"], p["md"], p["cells"], p["res"])
    env.set_control(m.ACC)
    env.set_u(p["U"])
    env.set_v_max(p["v_max"])
    env.set_a_max(p["a_max"])
    env.set_dt(1.0)
    return env


def one_problem(m, p, res):
    import bench
    env = make_env(m, p)
    start, goal = p["start"].to_row(), p["goal"].to_row()
    wdt = float(env._p.w) * float(env._p.dt)
    deltas = [0.0, wdt, 4.0 * wdt]
    kw = {"capacity": p["capacity"], "max_frontier": p["max_frontier"]}
    skw = dict(kw, max_rounds=20000)  # (a bound on the run, reported through the status if it is ever met)
    out = {"deltas": deltas, "search": {str(d): {"wall_ms_all": []} for d in deltas}, "sweep": {"wall_ms_all": []},
           "push_ms_all": [], "select_ms_all": []}
    cost = None
    for rep in range(REPS + 1):
        for d in deltas:
            t0 = time.perf_counter()
            rec = out["search"][str(d)]
            try:
                r = env.search(start, goal, delta=d, **skw)
            except RuntimeError as e:  # the table ran full: recorded, the other legs go on
                rec["error"] = str(e)
                continue
            ms = (time.perf_counter() - t0) * 1e3
            rec.update({"status": m.search.STATUS_NAMES[r.status], "cost": r.cost, "rounds": r.rounds, "expanded": r.expanded,
                        "nodes": r.table.stats()[0]})
            if rep:
                rec["wall_ms_all"].append(ms)
            if d == wdt:
                cost = r.cost
                # one push of every node and one select of every node, on the table this search left
                n = rec["nodes"]
                every = m.TableFrontier(env, n)
                r.open.clear()
                first = r.open.select(math.inf, every)  # (EMPTY: writes the count)
                assert first["status"] == m.search.EMPTY
                tab = r.table.download()
                every.id.upload(np.arange(n, dtype=np.int32))
                every.g.upload(tab["g"])
                st = np.zeros((every.n_fields, every.state_stride))
                st[:, :n] = tab["state"]
                every.state.upload(st)
                every.count.upload(np.array([n], np.int64))
                env.synchronize()
                env.timer_begin()
                r.open.push(every, n_max=n, eps=1.0, sight=True)
                push_ms = env.timer_end()
                env.timer_begin()
                r.open.select(math.inf, every, want_result=False)
                select_ms = env.timer_end()
                if rep:
                    out["push_ms_all"].append(push_ms)
                    out["select_ms_all"].append(select_ms)
                out["push_select_nodes"] = n
                every.free()
            r.free()
        if cost is not None and math.isfinite(cost):
            t0 = time.perf_counter()
            try:
                tab, rounds = env.cost_to_come(start, g_max=cost, **kw)
            except RuntimeError as e:  # the table or the frontier ran full: recorded, the other legs go on
                out["sweep"]["error"] = str(e)
                continue
            ms = (time.perf_counter() - t0) * 1e3
            out["sweep"].update({"g_max": cost, "rounds": rounds, "nodes": tab.stats()[0]})
            tab.free()
            if rep:
                out["sweep"]["wall_ms_all"].append(ms)
    for rec in list(out["search"].values()) + [out["sweep"]]:
        if rec["wall_ms_all"]:
            rec["wall_ms"] = med(rec["wall_ms_all"])
    if out["push_ms_all"]:
        out["push_ms"], out["select_ms"] = med(out["push_ms_all"]), med(out["select_ms_all"])
    env.close()
    r = bench.engine_plan(m, p["dim"], p["origin"], p["md"], p["cells"], p["res"], p["U"], p["start"], p["goal"], p["v_max"], p["a_max"],
                          p["batch"], reps=REPS)
    out["plan"] = {k: r[k] for k in ("wall_ms", "ok", "cost", "expansions", "nodes", "launches")}
    out["plan"]["what"] = "best of %d (bench.engine_plan), batch %d" % (REPS, p["batch"])
    res[p["name"]] = out
    print(p["name"], json.dumps(out), flush=True)


def measure(path):
    import motion_primitive_library_amd as m
    res = {"repetitions": REPS}
    for p in (corridor_problem(m), plan3d_problem(m)):
        one_problem(m, p, res)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "measure":
        measure(sys.argv[2])
    else:
        raise SystemExit(__doc__)
