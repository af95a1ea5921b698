"""What the dynamics-aware heuristic (include/mplx_heur.h) costs and saves on an MI355X: one warm-up, 7 repetitions, the
median.  Writes profiles/heur_dyn_times.json (or the path given).

  push      a push of 4 093 seeded rows, default against ROBUST, for a 3-D ACC and a 3-D JRK state space (device time
            between two events on the context's stream)
  corridor  the reference's corridor problem (test_planner_2d settings): device search and host plan(), default against
            ROBUST: rounds, expansions, wall time
  3D 120^3  the problem of bench.py's plan leg (ACC, |U| = 729, v_max 2): the same

    python profiles/micro/heur_dyn_times.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import motion_primitive_library_amd as m  # noqa: E402
from motion_primitive_library_amd import workloads as W  # noqa: E402

REPS, ROWS = 7, 4093


def median_of(fn):
    fn()
    t = [fn() for _ in range(REPS)]
    return float(np.median(t)), t


def push_times(control, name):
    D = 3
    env = m.EnvMap(D)
    env.setMap([0.0] * D, [64] * D, np.zeros(64 ** 3, np.int8), 0.25)
    env.set_control(control)
    env.set_u(W.grid_controls([-1.0, 0.0, 1.0], D))
    env.set_w(1.0)
    env.set_v_max(2.0)
    env.set_dt(1.0)
    rng = np.random.default_rng(1)
    s = np.zeros((env.n_fields, ROWS))
    # distinct positions on a 0.01 grid (distinct lattice states whatever the hash does with the other rows)
    idx = rng.choice(1500 ** 2, ROWS, replace=False)
    s[0], s[1], s[2] = 0.5 + (idx % 1500) * 0.01, 0.5 + (idx // 1500) * 0.01, 0.5 + rng.integers(0, 1500, ROWS) * 0.01
    s[D:2 * D] = rng.integers(-8, 9, (D, ROWS)) / 4.0
    if control == m.JRK:
        s[2 * D:3 * D] = rng.integers(-4, 5, (D, ROWS)) / 4.0
    goal = np.zeros(env.n_fields)
    goal[:D] = [12.25, 11.25, 10.25]
    env.set_goal(goal, tol_pos=0.5)
    tab = env.alloc_table(1 << 13)
    opn = env.alloc_open(tab)
    fr = m.TableFrontier(env, ROWS)
    n = tab.seed(s, frontier=fr)

    def one():
        env.synchronize()
        env.timer_begin()
        opn.push(fr, n_max=n, eps=1.0)
        return env.timer_end()

    out = {"rows": int(n)}
    out["default_ms"], out["default_ms_all"] = median_of(one)
    opn.set_heur("robust")
    out["robust_ms"], out["robust_ms_all"] = median_of(one)
    for b in (fr, opn, tab):
        b.free()
    env.close()
    print(name, out["default_ms"], out["robust_ms"], flush=True)
    return out


def search_times(env, start, goal, kw):
    out = {}
    for name, heur in (("default", None), ("robust", "robust")):
        def one():
            t0 = time.perf_counter()
            r = env.search(start, goal, heur=heur, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            one.last = (r.status, r.cost, r.rounds, r.expanded)
            r.free()
            return dt
        try:
            ms, all_ms = median_of(one)
        except RuntimeError as e:  # (a table that ran full: said, not hidden)
            out[name] = {"error": str(e)}
            print("search", name, "failed:", e, flush=True)
            continue
        out[name] = {"wall_ms": ms, "wall_ms_all": all_ms, "status": one.last[0], "cost": one.last[1], "rounds": one.last[2],
                     "expanded": one.last[3]}
        print("search", name, out[name]["wall_ms"], one.last, flush=True)
    return out


def plan_times(make):
    out = {}
    for name, args in (("default", (True, False)), ("robust", (False, True))):
        planner, start, goal = make()
        planner.setHeurIgnoreDynamics(*args)

        def one():
            t0 = time.perf_counter()
            ok = planner.plan(start, goal)
            dt = (time.perf_counter() - t0) * 1e3
            s = planner.summary()
            one.last = (bool(ok), s["cost"], s["expansions"])
            return dt
        ms, all_ms = median_of(one)
        out[name] = {"wall_ms": ms, "wall_ms_all": all_ms, "ok": one.last[0], "cost": one.last[1], "expansions": one.last[2]}
        print("plan", name, out[name]["wall_ms"], one.last, flush=True)
        planner.close()
    return out


def corridor():
    from test_plan_known_answer import corridor as load
    c = load()
    U = W.grid_controls([-0.5, 0.0, 0.5], 2)

    def make():
        planner = m.MapPlanner(2)
        mu = m.MapUtil(2)
        mu.setMap(c["origin"], c["dim"], c["cells"], c["res"])
        planner.setMapUtil(mu)
        planner.setVmax(1.0)
        planner.setAmax(1.0)
        planner.setDt(1.0)
        planner.setU(U)
        return planner, m.Waypoint(2, m.ACC, pos=c["start"]), m.Waypoint(2, m.ACC, pos=c["goal"])

    env = m.EnvMap(2)
    env.setMap(c["origin"], c["dim"], c["cells"], c["res"])
    env.set_control(m.ACC)
    env.set_u(U)
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    s, g = m.Waypoint(2, m.ACC, pos=c["start"]).to_row(), m.Waypoint(2, m.ACC, pos=c["goal"]).to_row()
    out = {"device_search": search_times(env, s, g, dict(capacity=1 << 16, max_frontier=4096)), "host_plan": plan_times(make)}
    env.close()
    return out


def problem_3d(edge=120):
    res = 0.1
    flat = W.box_map([edge] * 3, res, 0.08, 4242, side_m=(0.5, 2.5)).ravel()
    U3 = W.grid_controls(np.linspace(-2.0, 2.0, 9), 3)

    def free_near(p):
        cc = np.array([int(x / res) for x in p])
        for r in range(0, 30):
            for d in np.ndindex(2 * r + 1, 2 * r + 1, 2 * r + 1):
                q = cc + np.array(d) - r
                if np.all(q >= 0) and np.all(q < edge) and flat[q[0] + edge * (q[1] + edge * q[2])] == 0:
                    return [(q[i] + 0.5) * res for i in range(3)]
        raise RuntimeError("no free cell")

    ps, pg = free_near([1.0, 1.0, 1.0]), free_near([edge * res - 1.0, edge * res - 1.2, edge * res - 1.5])

    def make():
        planner = m.MapPlanner(3)
        mu = m.MapUtil(3)
        mu.setMap([0.0] * 3, [edge] * 3, flat, res)
        planner.setMapUtil(mu)
        planner.setVmax(2.0)
        planner.setAmax(2.0)
        planner.setDt(1.0)
        planner.setU(U3)
        planner.setBatch(64)
        return planner, m.Waypoint(3, m.ACC, pos=ps), m.Waypoint(3, m.ACC, pos=pg)

    env = m.EnvMap(3)
    env.setMap([0.0] * 3, [edge] * 3, flat, res)
    env.set_control(m.ACC)
    env.set_u(U3)
    env.set_v_max(2.0)
    env.set_a_max(2.0)
    env.set_dt(1.0)
    s, g = m.Waypoint(3, m.ACC, pos=ps).to_row(), m.Waypoint(3, m.ACC, pos=pg).to_row()
    out = {"device_search": search_times(env, s, g, dict(capacity=1 << 22, max_frontier=1 << 12, delta=0.0, max_expand=300000)), "host_plan": plan_times(make)}
    env.close()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "heur_dyn_times.json")
    out = {"repetitions": REPS, "warm_up": 1, "statistic": "median", "device": m.EnvMap(2).device_info()}
    out["push_3d_acc"] = push_times(m.ACC, "push ACC")
    out["push_3d_jrk"] = push_times(m.JRK, "push JRK")
    for name, fn in (("corridor", corridor), ("problem_3d_120", problem_3d)):
        out[name] = fn()
        with open(path, "w") as f:  # (after every part: a later failure keeps what was measured)
            json.dump(out, f, indent=1, default=str)
    print("wrote", path)


if __name__ == "__main__":
    main()
