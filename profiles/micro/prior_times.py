"""Times of prior-trajectory guidance on the device (include/mplx_prior.h) on the corridor of tests/golden:

    python profiles/micro/prior_times.py measure OUT.json      every step below, each in a process of its own
    python profiles/micro/prior_times.py step NAME OUT.json    one step: set_1, set_8, set_64, pipe_1, pipe_8, pipe_64, host

  set_Q    one OpenSet.set_priors of Q priors (the 34-segment VEL path of query q), the info read back: wall clock
           around the call (uploads of starts, actions and the control table included).
  pipe_Q   coarse to fine for Q queries (the queries of multi_times.py): stage 1 = EnvMap.search_many with VEL controls
           {-1, 0, 1}^2, as_priors(), stage 2 = search_many with the state (pos, vel, acc), jerk controls {-0.5, 0, 0.5}^2,
           priors=...; next to it the plain stage 2 of the same queries (no priors: it runs on the parent commit as well).
           eps 1, delta = w dt = 10, the ray trace on; 2^17 nodes per query, 8 192 min(Q, 16) frontier rows.
           rounds x rows: total rounds and expansions are reported beside the times.
  host     the host planner's two-stage scenario (test_planner_2d_with_prior_traj.cpp): a VEL plan, setPriorTrajectory, the
           guided plan; and the plain plan of the second planner.

The project's protocol: one warm-up and REPS = 7 repetitions, the legs alternating inside a repetition; medians and all
samples are reported.  `measure` runs the steps in order, each under its own time limit, and stops at the first that fails
or runs out of time; the steps before it stay in OUT.json."""
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

REPS = 7
STEPS = [("set_1", 120), ("set_8", 120), ("set_64", 120), ("pipe_1", 240), ("pipe_8", 300), ("pipe_64", 420), ("host", 240)]


def med(xs):
    return float(np.median(xs))


def make_env(m, p, control, U):
    env = m.EnvMap(2)
    env.setMap(p["origin"], p["md"], p["cells"], p["res"])
    env.set_control(control)
    env.set_u(U)
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    return env


def rows(m, control, pts):
    return np.stack([m.Waypoint(2, control, pos=x).to_row() for x in pts])


def problem(m, Q):
    from multi_times import queries
    from open_times import corridor_problem
    p = corridor_problem(m)
    starts, goals = queries(m, p, Q)
    return p, starts[:2].T.copy(), goals[:, :2].copy()


def stage1(m, env1, s, g):
    return env1.search_many(rows(m, m.VEL, s).T.copy(), rows(m, m.VEL, g), delta=10.0, capacity=(1 << 12) * len(s))


def step_set(m, Q):
    p, s, g = problem(m, Q)
    env1, env = make_env(m, p, m.VEL, 2.0 * p["U"]), make_env(m, p, m.JRK, p["U"])
    r1 = stage1(m, env1, s, g)
    priors = r1.as_priors()
    tab = env.alloc_table(64 * Q, n_queries=Q)
    opn = env.alloc_open(tab)
    opn.set_goals(rows(m, m.JRK, g))
    out = {"Q": Q, "wall_ms_all": []}
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        info = opn.set_prior_list(priors)
        ms = (time.perf_counter() - t0) * 1e3
        if rep:
            out["wall_ms_all"].append(ms)
    out.update({"wall_ms": med(out["wall_ms_all"]), "n_steps": [int(x) for x in info["n_steps"]]})
    opn.free()
    tab.free()
    r1.free()
    env1.close()
    env.close()
    return out


def step_pipe(m, Q):
    p, s, g = problem(m, Q)
    env1, env = make_env(m, p, m.VEL, 2.0 * p["U"]), make_env(m, p, m.JRK, p["U"])
    starts, goals = rows(m, m.JRK, s).T.copy(), rows(m, m.JRK, g)
    kw = {"delta": 10.0, "capacity": (1 << 17) * Q, "max_frontier": 8192 * min(Q, 16)}
    out = {"Q": Q, "stage1": {"wall_ms_all": []}, "guided": {"wall_ms_all": []}, "pipeline": {"wall_ms_all": []}, "plain": {"wall_ms_all": []}}

    def record(rec, r, ms, rep):
        rec.update({"found": int(sum(r.found)), "rounds": r.total_rounds, "expanded": int(sum(r.expanded)), "nodes": r.table.stats()[0],
                    "costs": [float(c) for c in r.cost]})
        if rep:
            rec["wall_ms_all"].append(ms)
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        r1 = stage1(m, env1, s, g)
        t1 = time.perf_counter()
        priors = r1.as_priors()
        r2 = env.search_many(starts, goals, priors=priors, **kw)
        t2 = time.perf_counter()
        record(out["stage1"], r1, (t1 - t0) * 1e3, rep)
        record(out["guided"], r2, (t2 - t1) * 1e3, rep)  # (as_priors and set_priors included)
        if rep:
            out["pipeline"]["wall_ms_all"].append((t2 - t0) * 1e3)
        r1.free()
        r2.free()
        t0 = time.perf_counter()
        r3 = env.search_many(starts, goals, **kw)
        record(out["plain"], r3, (time.perf_counter() - t0) * 1e3, rep)
        r3.free()
    for rec in out.values():
        if isinstance(rec, dict):
            rec["wall_ms"] = med(rec["wall_ms_all"])
    gd, pl = out["guided"], out["plain"]
    out["claim"] = {"guided_rounds_x_rows": gd["rounds"] * gd["expanded"], "plain_rounds_x_rows": pl["rounds"] * pl["expanded"],
                    "cost_no_worse": all(a <= b for a, b in zip(gd["costs"], pl["costs"]))}
    env1.close()
    env.close()
    return out


def step_host(m):
    p, s, g = problem(m, 1)

    def planner(control, U):
        pl = m.MapPlanner(2, device=0)
        mu = m.MapUtil(2)
        mu.setMap(p["origin"], p["md"], p["cells"], p["res"])
        pl.setMapUtil(mu)
        pl.setVmax(1.0)
        pl.setAmax(1.0)
        pl.setDt(1.0)
        pl.setU(U)
        pl.setBatch(p["batch"])
        return pl
    first, second, plain = planner(m.VEL, 2.0 * p["U"]), planner(m.JRK, p["U"]), planner(m.JRK, p["U"])
    for pl in (second, plain):
        pl.setEpsilon(1.0)
        pl.setW(10)
        pl.setTol(0.5)
    wp = lambda c, x: m.Waypoint(2, c, pos=x)
    out = {"two_stage": {"wall_ms_all": []}, "plain": {"wall_ms_all": []}}
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        ok1 = first.plan(wp(m.VEL, s[0]), wp(m.VEL, g[0]))
        second.setPriorTrajectory(first)
        ok2 = second.plan(wp(m.JRK, s[0]), wp(m.VEL, g[0]))
        ms = (time.perf_counter() - t0) * 1e3
        s1, s2 = first.summary(), second.summary()
        out["two_stage"].update({"ok": bool(ok1 and ok2), "cost": s2["cost"], "expansions": [s1["expansions"], s2["expansions"]]})
        if rep:
            out["two_stage"]["wall_ms_all"].append(ms)
        t0 = time.perf_counter()
        ok3 = plain.plan(wp(m.JRK, s[0]), wp(m.VEL, g[0]))
        ms = (time.perf_counter() - t0) * 1e3
        out["plain"].update({"ok": bool(ok3), "cost": plain.summary()["cost"], "expansions": plain.summary()["expansions"]})
        if rep:
            out["plain"]["wall_ms_all"].append(ms)
    for pl in (first, second, plain):
        pl.close()
    for rec in out.values():
        rec["wall_ms"] = med(rec["wall_ms_all"])
    return out


def load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {"repetitions": REPS}


def step(name, path):
    import motion_primitive_library_amd as m
    kind = name.split("_")[0]
    out = step_host(m) if name == "host" else (step_set if kind == "set" else step_pipe)(m, int(name.split("_")[1]))
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
            raise SystemExit("prior_times: step %s ended with %d: stopping" % (name, rc))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "measure":
        measure(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "step":
        step(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
