"""Times of device replanning (include/mplx_replan.h, SearchResult.replan / MultiSearchResult.replan) on the corridor of
tests/golden (2D ACC, 9 controls), next to a fresh search from the same root on the edited map and the host A* plan:

    python profiles/micro/replan_times.py measure OUT.json      every step below, each in a process of its own
    python profiles/micro/replan_times.py step NAME OUT.json    one step: scenarios, many_1, many_8, many_64, rebase

  scenarios  the corridor scenarios of tests/test_replan.py (eps 1, delta 10, no ray trace): per repetition a first search
             on the first map (not timed) and the map edit, then, timed:
               replan   result.replan(...) -- rebase, closed push, the forced round, the rounds after it
               fresh    EnvMap.search(root_state, goal, start_g=g_root) on the edited map
               plan     the host A* (MapPlanner.plan) from the root's state on the edited map, its warm-up plan not timed
             and the map is put back.
  many_Q     for Q in {1, 8, 64}: the queries of multi_times.py, the wall across query 0's middle edge, advance = 5:
             replan of the search_many result against a fresh search_many from the Q roots, and Q host plans.
  rebase     NodeTable.rebase alone (root = the seeds, edges checked on the unedited map: everything is kept, so the call
             can be repeated on the same table), with the result read back, on the table of one corridor search (10 102
             nodes) and on that of the 64 queries; the number of resolve passes is ceil(log2(bound of n_nodes)) + 1.

One warm-up and REPS = 5 repetitions of everything, the legs alternating inside a repetition; medians, minima and maxima
are reported.  `measure` runs the steps in order, each under its own time limit, and stops at the first that fails or
runs out of time; the steps before it stay in OUT.json."""
import json
import math
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
STEPS = [("scenarios", 420), ("many_1", 240), ("many_8", 300), ("many_64", 420), ("rebase", 300)]  # name, time limit in seconds
EPS, DELTA = 1.0, 10.0


def finish(rec):
    xs = rec["wall_ms_all"]
    rec["wall_ms"], rec["min_ms"], rec["max_ms"] = float(np.median(xs)), float(min(xs)), float(max(xs))


def planner_on(m, p, cells):
    pl = m.MapPlanner(2, device=0)
    mu = m.MapUtil(2)
    mu.setMap(p["origin"], p["md"], cells, p["res"])
    pl.setMapUtil(mu)
    pl.setVmax(p["v_max"])
    pl.setAmax(p["a_max"])
    pl.setDt(1.0)
    pl.setU(p["U"])
    pl.setBatch(p["batch"])
    return pl


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def step_scenarios(m):
    from open_times import corridor_problem, make_env
    from test_replan import SCENARIOS, world
    w, p = world(m), corridor_problem(m)
    goal_wp = lambda row: m.Waypoint(2, m.ACC, pos=row[:2])
    out = {}
    for name in sorted(SCENARIOS):
        sc = SCENARIOS[name]
        first, new = w.map_of(sc["first"]), w.cells(sc["wall"])
        changed = np.nonzero(new != first)[0]
        goal = w.goal_of(sc)
        p1 = dict(p, cells=first)
        env = make_env(m, p1)
        kw = dict(eps=EPS, delta=DELTA, capacity=p["capacity"], sight=False)
        rec = {k: {"wall_ms_all": []} for k in ("replan", "fresh", "plan")}
        pl = planner_on(m, p, new)
        root_wp = None
        for rep in range(REPS + 1):
            r0 = env.search(w.start, w.goal, max_frontier=sc.get("cap"), **kw)
            root = int(r0.table.path(r0.goal_id)[0][sc["advance"]])
            s_root, g_root = r0.table.state_of(root), float(r0.table.download()["g"][root])
            if changed.size:
                env.editMap(changed, new[changed])
            n0 = r0.table.stats()[0]
            r1, ms = timed(lambda: r0.replan(root=root if sc["advance"] else None, goal_row=goal if "goal" in sc else None))
            rec["replan"].update({"cost": r1.cost, "rounds": r1.rounds, "expanded": r1.expanded, "kept": r1.rebase_info["n_kept"],
                                  "bad_edges": r1.rebase_info["n_bad_edges"], "nodes_before": n0})
            r1.free()
            if rep:
                rec["replan"]["wall_ms_all"].append(ms)
            f, ms = timed(lambda: env.search(s_root, goal, start_g=g_root, **kw))
            rec["fresh"].update({"cost": f.cost, "rounds": f.rounds, "expanded": f.expanded})
            f.free()
            if rep:
                rec["fresh"]["wall_ms_all"].append(ms)
            if root_wp is None:
                root_wp = m.Waypoint(2, m.ACC, pos=s_root[0:2], vel=s_root[2:4], acc=s_root[4:6])
                pl.plan(root_wp, goal_wp(goal))  # warm-up
            ok, ms = timed(lambda: pl.plan(root_wp, goal_wp(goal)))
            rec["plan"].update({"ok": bool(ok), "cost_from_root": float(pl.summary()["cost"]), "g_root": g_root,
                                "expansions": int(pl.summary()["expansions"])})
            if rep:
                rec["plan"]["wall_ms_all"].append(ms)
            if changed.size:
                env.editMap(changed, first[changed])
        pl.close()
        env.close()
        for r in rec.values():
            finish(r)
        rec["same_cost"] = rec["replan"]["cost"] == rec["fresh"]["cost"]
        out[name] = rec
    return out


def step_many(m, Q):
    from multi_times import queries
    from open_times import corridor_problem, make_env
    from test_replan import world
    w, p = world(m), corridor_problem(m)
    env = make_env(m, p)
    starts, goals = queries(m, p, Q)
    wall = np.asarray(w.walls["mid"])
    new = w.cells("mid")
    kw = dict(eps=EPS, delta=DELTA, capacity=p["capacity"] * Q, max_frontier=p["max_frontier"] * min(Q, 16), sight=False)
    rec = {k: {"wall_ms_all": []} for k in ("replan", "fresh", "plan")}
    planners = None
    for rep in range(REPS + 1):
        r0 = env.search_many(starts, goals, **kw)
        roots = [int(r0.table.path(r0.goal_id[q])[0][5]) for q in range(Q)]
        d = r0.table.download()
        s_root, g_root = np.ascontiguousarray(d["state"][:, roots]), d["g"][roots].copy()
        env.editMap(wall, 100)
        r1, ms = timed(lambda: r0.replan(roots=roots))
        rec["replan"].update({"found": int(sum(r1.found)), "rounds": r1.total_rounds, "expanded": int(sum(r1.expanded)),
                              "kept": r1.rebase_info["n_kept"], "bad_edges": r1.rebase_info["n_bad_edges"], "nodes": r1.table.stats()[0],
                              "costs": [float(c) for c in r1.cost]})
        r1.free()
        if rep:
            rec["replan"]["wall_ms_all"].append(ms)
        f, ms = timed(lambda: env.search_many(s_root, goals, start_g=g_root, **kw))
        rec["fresh"].update({"found": int(sum(f.found)), "rounds": f.total_rounds, "expanded": int(sum(f.expanded)),
                             "costs": [float(c) for c in f.cost]})
        f.free()
        if rep:
            rec["fresh"]["wall_ms_all"].append(ms)
        if planners is None:
            planners = []
            for q in range(Q):
                pl = planner_on(m, p, new)
                sq = m.Waypoint(2, m.ACC, pos=s_root[0:2, q], vel=s_root[2:4, q], acc=s_root[4:6, q])
                gq = m.Waypoint(2, m.ACC, pos=goals[q, :2])
                pl.plan(sq, gq)  # warm-up
                planners.append((pl, sq, gq))
        ok, ms = timed(lambda: sum(1 for pl, sq, gq in planners if pl.plan(sq, gq)))
        rec["plan"].update({"ok": ok, "expansions": int(sum(pl.summary()["expansions"] for pl, _, _ in planners))})
        if rep:
            rec["plan"]["wall_ms_all"].append(ms)
        env.editMap(wall, w.grid[wall])
    for pl, _, _ in planners:
        pl.close()
    env.close()
    for r in rec.values():
        finish(r)
    rec["Q"] = Q
    rec["same_costs"] = rec["replan"]["costs"] == rec["fresh"]["costs"]
    return rec


def step_rebase(m):
    from multi_times import queries
    from open_times import corridor_problem, make_env
    p = corridor_problem(m)
    env = make_env(m, p)
    out = {}
    for Q in (1, 64):
        starts, goals = queries(m, p, Q)
        r = env.search_many(starts, goals, eps=EPS, delta=DELTA, capacity=p["capacity"] * Q, max_frontier=p["max_frontier"] * min(Q, 16),
                            sight=False)
        n = r.table.stats()[0]
        fr = m.table.TableFrontier(env, n)
        rec = {"nodes": n, "resolve_passes": int(math.ceil(math.log2(max(n, 2)))) + 1, "wall_ms_all": []}
        for check in (True, False):
            key = "wall_ms_all" if check else "no_edges_wall_ms_all"
            rec[key] = []
            for rep in range(REPS + 1):
                info, ms = timed(lambda: r.table.rebase(roots=[-1] * Q, check_edges=check, frontier=fr))
                assert info["n_kept"] == n and info["n_bad_edges"] == 0
                if rep:
                    rec[key].append(ms)
        finish(rec)
        rec["no_edges_wall_ms"] = float(np.median(rec["no_edges_wall_ms_all"]))
        out["Q%d" % Q] = rec
        fr.free()
        r.free()
    env.close()
    return out


def load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {"repetitions": REPS}


def step(name, path):
    import motion_primitive_library_amd as m
    out = step_scenarios(m) if name == "scenarios" else step_rebase(m) if name == "rebase" else step_many(m, int(name.split("_")[1]))
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
            raise SystemExit("replan_times: step %s ended with %d: stopping" % (name, rc))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "measure":
        measure(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "step":
        step(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
