"""Times of the k-best select of an open set (include/mplx_best.h) next to the plain select, in one process:

    python profiles/micro/open_best_times.py measure OUT.json [COMMIT]

  select    one plain select (delta = +inf) against one best-select with k = 16 and with k = the node count (no radix
            pass has work: the candidates are no more than k), all three over the same freshly pushed nodes: event times
            (mplx_timer_begin / _end on the context's stream).  Once over the table the default search leaves on the
            corridor of tests/golden (10 102 nodes), once over 2^20 nodes at rest with keys from 64 values and once with
            2^20 distinct keys.
  search    EnvMap.search on the corridor (eps 1, the ray trace on): the defaults, delta = 0, and best in {16, 64} with
            delta = +inf; and on the 3D problem of the bench (120^3 cells, ACC, 729 controls) with heur="robust":
            delta = 0 against best = 64 with delta = +inf.  Wall clock around a call that ends in its last select's
            synchronise, with cost, rounds, expansions and nodes beside it.
  plan      the host A* (MapPlanner.plan, bench.engine_plan) on the same two problems.

One warm-up and REPS repetitions of everything, alternating the legs inside a repetition; medians and all samples are
reported.  COMMIT: what the numbers were taken on (the caller says: the script does not ask git)."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from open_times import corridor_problem, make_env, med, plan3d_problem  # noqa: E402

REPS = 5
INF = math.inf


def time_selects(m, env, opn, every, n, out):
    """Plain, k = 16 and k = n over the same n open nodes; `every` holds the rows that open them (pushed with eps 0)."""
    legs = (("plain", None), ("best_16", 16), ("best_all", n))
    for name, _ in legs:
        out.setdefault(name + "_ms_all", [])
    sel = m.TableFrontier(env, n)
    for rep in range(REPS + 1):
        for name, k in legs:
            opn.push(every, n_max=n, eps=0.0)
            env.synchronize()
            env.timer_begin()
            opn.select(INF, sel, want_result=False, best=k)
            ms = env.timer_end()
            if rep:
                out[name + "_ms_all"].append(ms)
    for name, _ in legs:
        out[name + "_ms"] = med(out[name + "_ms_all"])
    out["nodes"] = n
    sel.free()


def corridor_selects(m, p, res):
    env = make_env(m, p)
    r = env.search(p["start"].to_row(), p["goal"].to_row(), capacity=p["capacity"], max_frontier=p["max_frontier"])
    n = r.table.stats()[0]
    tab = r.table.download()
    every = m.TableFrontier(env, n)
    every.id.upload(np.arange(n, dtype=np.int32))
    every.g.upload(r.open.download()["f"][:n])  # the keys the search left, planted again with eps = 0
    st = np.zeros((every.n_fields, every.state_stride))
    st[:, :n] = tab["state"]
    every.state.upload(st)
    every.count.upload(np.array([n], np.int64))
    r.open.clear()
    out = {}
    time_selects(m, env, r.open, every, n, out)
    every.free()
    r.free()
    env.close()
    res["select_corridor"] = out
    print("select_corridor", json.dumps(out), flush=True)


def big_selects(m, res, n=1 << 20):
    env = m.EnvMap(2)
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls([-1.0, 0.0, 1.0], 2))
    env.set_v_max(1.0)
    env.set_dt(1.0)
    goal = np.zeros(10)
    goal[:2] = 1e6
    env.set_goal(goal)
    states = np.zeros((10, n))
    i = np.arange(n)
    states[0], states[1] = (i % 1024) * 0.1, (i // 1024) * 0.1
    tab = env.alloc_table(n + 4096)
    every = m.TableFrontier(env, n)
    got = tab.seed(states, frontier=every)
    opn = env.alloc_open(tab)
    rng = np.random.default_rng(1)
    for name, keys in (("select_1m_64_values", rng.integers(0, 64, size=got) * 0.5),
                       ("select_1m_distinct", rng.permutation(got) * 0.25)):
        every.g.upload(keys.astype(np.float64))
        out = {}
        time_selects(m, env, opn, every, got, out)
        res[name] = out
        print(name, json.dumps(out), flush=True)
    every.free()
    opn.free()
    tab.free()
    env.close()


def searches(m, p, legs, res, **common):
    import bench
    env = make_env(m, p)
    start, goal = p["start"].to_row(), p["goal"].to_row()
    out = {name: {"args": {k: (str(v) if v == INF else v) for k, v in kw.items()}, "wall_ms_all": []} for name, kw in legs}
    for rep in range(REPS + 1):
        for name, kw in legs:
            rec = out[name]
            t0 = time.perf_counter()
            try:
                r = env.search(start, goal, capacity=p["capacity"], max_rounds=20000, **dict(common, **kw))
            except RuntimeError as e:  # the table ran full: recorded, the other legs go on
                rec["error"] = str(e)
                continue
            ms = (time.perf_counter() - t0) * 1e3
            rec.update({"status": m.search.STATUS_NAMES[r.status], "cost": r.cost, "rounds": r.rounds, "expanded": r.expanded,
                        "nodes": r.table.stats()[0]})
            if rep:
                rec["wall_ms_all"].append(ms)
            r.free()
    for rec in out.values():
        if rec["wall_ms_all"]:
            rec["wall_ms"] = med(rec["wall_ms_all"])
    env.close()
    r = bench.engine_plan(m, p["dim"], p["origin"], p["md"], p["cells"], p["res"], p["U"], p["start"], p["goal"], p["v_max"], p["a_max"],
                          p["batch"], reps=REPS)
    out["plan"] = {k: r[k] for k in ("wall_ms", "ok", "cost", "expansions", "nodes", "launches")}
    out["plan"]["what"] = "best of %d (bench.engine_plan), batch %d" % (REPS, p["batch"])
    res["search_" + p["name"]] = out
    print("search_" + p["name"], json.dumps(out), flush=True)


def measure(path, commit):
    import motion_primitive_library_amd as m
    res = {"repetitions": REPS, "commit": commit}

    def save():
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
    c = corridor_problem(m)
    corridor_selects(m, c, res)
    save()
    big_selects(m, res)
    save()
    searches(m, c, (("default", {"max_frontier": c["max_frontier"]}), ("delta_0", {"delta": 0.0, "max_frontier": c["max_frontier"]}),
                    ("best_16", {"delta": INF, "best": 16}), ("best_64", {"delta": INF, "best": 64})), res)
    save()
    p = plan3d_problem(m)
    searches(m, p, (("delta_0", {"delta": 0.0, "max_frontier": p["max_frontier"]}), ("best_64", {"delta": INF, "best": 64})), res,
             heur="robust")
    save()


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "measure":
        measure(sys.argv[2], sys.argv[3] if len(sys.argv) == 4 else "unknown")
    else:
        raise SystemExit(__doc__)
