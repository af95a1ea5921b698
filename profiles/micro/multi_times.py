"""Times of the batched device search (include/mplx_multi.h, EnvMap.search_many) on the corridor of tests/golden (2D ACC,
9 controls), next to the same queries run one by one:

    python profiles/micro/multi_times.py measure OUT.json      every step below, each in a process of its own
    python profiles/micro/multi_times.py step NAME OUT.json    one step: many_1, many_8, many_64, guard

  many_Q   for Q in {1, 8, 64} (delta = w dt = 10, eps 1, the ray trace on; 2^15 nodes and 4 096 frontier rows for a
           single search, Q times the nodes and min(Q, 16) times the rows for the batch):
             search_many   EnvMap.search_many of the Q queries: wall clock around the call, rounds, expansions, nodes
             sequential    Q EnvMap.search calls, one query after the other, each with a single search's sizes
             plan          Q host A* plans (MapPlanner.plan), one planner per query, its warm-up plan not timed
           Query 0 is the corridor's own start and goal.  Query q > 0 moves the start by (+0.1 (q % 8), +0.1 (q // 8)) m
           and the goal by (-0.1 (q % 8), -0.1 (q // 8)) m: two cells per step, every one checked to be free.
  guard    EnvMap.search of query 0 with delta 0 and 10: the single-query path, for the comparison with the parent
           commit (run the same step there: it needs nothing of this change).

The protocol of open_times.py: one warm-up and REPS = 5 repetitions of everything, the legs alternating inside a
repetition; medians and all samples are reported.  `measure` runs the steps in order, each under its own time limit,
and stops at the first that fails or runs out of time; the steps before it stay in OUT.json."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REPS = 5
STEPS = [("guard", 240), ("many_1", 240), ("many_8", 300), ("many_64", 420)]  # name, time limit in seconds


def med(xs):
    return float(np.median(xs))


def queries(m, p, Q):
    """(starts [10][Q], goals [Q][10]) as the docstring says; raises if a shifted point is not in a free cell."""
    md, cells = p["md"], np.asarray(p["cells"]).reshape(p["md"][1], p["md"][0])
    s0, g0 = np.asarray(p["start"].to_row()[:2]), np.asarray(p["goal"].to_row()[:2])
    starts, goals = np.zeros((10, Q)), np.zeros((Q, 10))
    for q in range(Q):
        d = np.array([0.1 * (q % 8), 0.1 * (q // 8)])
        for pos in (s0 + d, g0 - d):
            c = np.floor((pos - np.asarray(p["origin"])) / p["res"]).astype(int)
            if not (0 <= c[0] < md[0] and 0 <= c[1] < md[1]) or cells[c[1], c[0]] != 0:
                raise RuntimeError("query %d: %r is not in a free cell" % (q, pos))
        starts[:, q] = m.Waypoint(2, m.ACC, pos=s0 + d).to_row()
        goals[q] = m.Waypoint(2, m.ACC, pos=g0 - d).to_row()
    return starts, goals


def step_many(m, Q):
    from open_times import corridor_problem, make_env
    p = corridor_problem(m)
    env = make_env(m, p)
    starts, goals = queries(m, p, Q)
    # one query gets what open_times.py gives it; Q queries share Q times the nodes (at least) and up to 16 times the rows
    one = {"delta": 10.0, "capacity": p["capacity"], "max_frontier": p["max_frontier"]}
    kw = {"delta": 10.0, "capacity": p["capacity"] * Q, "max_frontier": p["max_frontier"] * min(Q, 16)}
    out = {"Q": Q, "search_many": {"wall_ms_all": []}, "sequential": {"wall_ms_all": []}, "plan": {"wall_ms_all": []}}
    planners = []
    for q in range(Q):
        pl = m.MapPlanner(2, device=0)
        mu = m.MapUtil(2)
        mu.setMap(p["origin"], p["md"], p["cells"], p["res"])
        pl.setMapUtil(mu)
        pl.setVmax(p["v_max"])
        pl.setAmax(p["a_max"])
        pl.setDt(1.0)
        pl.setU(p["U"])
        pl.setBatch(p["batch"])
        sq, gq = m.Waypoint(2, m.ACC, pos=starts[:2, q]), m.Waypoint(2, m.ACC, pos=goals[q, :2])
        pl.plan(sq, gq)  # warm-up
        planners.append((pl, sq, gq))
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        r = env.search_many(starts, goals, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        rec = out["search_many"]
        rec.update({"found": int(sum(r.found)), "rounds": r.total_rounds, "expanded": int(sum(r.expanded)), "nodes": r.table.stats()[0],
                    "cost_q0": r.cost[0], "costs": [float(c) for c in r.cost]})
        r.free()
        if rep:
            rec["wall_ms_all"].append(ms)
        t0 = time.perf_counter()
        rounds = expanded = nodes = found = 0
        costs = []
        for q in range(Q):
            s = env.search(starts[:, q], goals[q], **one)
            rounds, expanded, nodes, found = rounds + s.rounds, expanded + s.expanded, nodes + s.table.stats()[0], found + int(s.found)
            costs.append(float(s.cost))
            s.free()
        ms = (time.perf_counter() - t0) * 1e3
        out["sequential"].update({"found": found, "rounds": rounds, "expanded": expanded, "nodes": nodes, "costs": costs})
        if rep:
            out["sequential"]["wall_ms_all"].append(ms)
        t0 = time.perf_counter()
        ok = sum(1 for pl, sq, gq in planners if pl.plan(sq, gq))
        ms = (time.perf_counter() - t0) * 1e3
        out["plan"].update({"ok": ok, "costs": [float(pl.summary()["cost"]) for pl, _, _ in planners],
                            "expansions": int(sum(pl.summary()["expansions"] for pl, _, _ in planners))})
        if rep:
            out["plan"]["wall_ms_all"].append(ms)
    for pl, _, _ in planners:
        pl.close()
    env.close()
    for rec in (out["search_many"], out["sequential"], out["plan"]):
        rec["wall_ms"] = med(rec["wall_ms_all"])
    out["same_costs"] = out["search_many"]["costs"] == out["sequential"]["costs"]
    return out


def step_guard(m):
    from open_times import corridor_problem, make_env
    p = corridor_problem(m)
    env = make_env(m, p)
    start, goal = p["start"].to_row(), p["goal"].to_row()
    out = {str(d): {"wall_ms_all": []} for d in (0.0, 10.0)}
    for rep in range(REPS + 1):
        for d in (0.0, 10.0):
            t0 = time.perf_counter()
            r = env.search(start, goal, delta=d, capacity=p["capacity"], max_frontier=p["max_frontier"])
            ms = (time.perf_counter() - t0) * 1e3
            out[str(d)].update({"cost": r.cost, "rounds": r.rounds, "expanded": r.expanded})
            r.free()
            if rep:
                out[str(d)]["wall_ms_all"].append(ms)
    env.close()
    for rec in out.values():
        rec["wall_ms"] = med(rec["wall_ms_all"])
        rec["spread_ms"] = max(rec["wall_ms_all"]) - min(rec["wall_ms_all"])
    return out


def load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {"repetitions": REPS}


def step(name, path):
    import motion_primitive_library_amd as m
    out = step_guard(m) if name == "guard" else step_many(m, int(name.split("_")[1]))
    res = load(path)
    res[name] = out
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(name, json.dumps(out), flush=True)


def measure(path):
    for name, limit in STEPS:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "step", name, path], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            raise SystemExit("multi_times: step %s ended with %d: stopping" % (name, rc))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "measure":
        measure(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "step":
        step(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
