"""What a re-key costs and what an anytime schedule on one tree buys (include/mplx_anytime.h).

    python profiles/micro/anytime_times.py measure [OUT.json]   # GPU box; default profiles/anytime_times.json

(a) one re-key (write, no cut, no read-back inside the window) of
      - the table the corridor search leaves (about 10 k nodes), and
      - a table of 2^20 seeded lattice states (3-D, at rest, g from eight values),
    beside the push of the same nodes as one frontier -- open_push_kernel, which this change does not touch: the bound on
    what one pass over the heuristic of those nodes can cost.  A timed window is CALLS = 20 back-to-back calls between
    timer_begin / timer_end (events on the context's stream) after one untimed call; the figure is the window over CALLS,
    the median of REPS = 5 windows.  Also the bound alone (write = 0) with its read-back, by a host clock (it ends in a
    synchronise).
(b) on the corridor and on the 3-D 120^3 problem of bench.py's plan leg (profiles/micro/open_times.py builds both): the
    schedule eps = 3, 2, 1.5, 1 through search.anytime (the first stage is a search at eps = 3), against four fresh
    searches at those eps and against one fresh search at eps = 1.  Host clock around each stage / search (every one ends
    in the read-back of its last select), the median of REPS = 5 runs after one untimed run; rounds, expansions, cost,
    lower and ratio per stage.  delta is the search's default (w * dt).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REPS, CALLS = 5, 20
SCHEDULE = [3.0, 2.0, 1.5, 1.0]


def med(xs):
    return float(np.median(xs))


def windows(env, fn):
    fn()
    env.synchronize()
    out = []
    for _ in range(REPS):
        env.timer_begin()
        for _ in range(CALLS):
            fn()
        out.append(env.timer_end() / CALLS)
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


def rekey_and_push(m, env, states, g, eps):
    """A table seeded with `states` (distinct lattice states), everything pushed: one re-key against one push of all nodes."""
    n = states.shape[1]
    tab = env.alloc_table(n + 64)
    opn = env.alloc_open(tab)
    fr = m.TableFrontier(env, n)
    count = tab.seed(states, g, frontier=fr)
    opn.push(fr, n_max=count, eps=eps)
    d0 = opn.download()
    rk = windows(env, lambda: opn.rekey(eps, want_result=False))
    d1 = opn.download()
    same = bool(np.array_equal(d0["f"].view(np.uint64), d1["f"].view(np.uint64)) and np.array_equal(d0["flags"], d1["flags"]))
    ps = windows(env, lambda: opn.push(fr, n_max=count, eps=eps))
    bd = host_clock(env, lambda: opn.rekey(eps, write=False))
    out = {"nodes": int(count), "rekey_ms": med(rk), "rekey_ms_all": rk, "push_all_nodes_ms": med(ps), "push_all_nodes_ms_all": ps,
           "bound_with_read_back_ms": med(bd), "bound_with_read_back_ms_all": bd, "rekey_at_the_push_eps_is_identity": same}
    for b in (fr, opn, tab):
        b.free()
    return out


def million(m):
    env = m.EnvMap(3)
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls([-1.0, 0.0, 1.0], 3))
    env.set_v_max(2.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    goal = m.Waypoint(3, m.ACC, pos=[40.0, 40.0, 20.0]).to_row()
    env.set_goal(goal, w=10.0, v_max=2.0)
    k = np.arange(1 << 20)
    s = np.zeros((env.n_fields, k.size))
    s[0], s[1], s[2] = 0.25 * (k % 128), 0.25 * ((k // 128) % 128), 0.25 * (k // 16384)
    g = np.random.default_rng(1).integers(0, 8, k.size) * 0.5
    out = rekey_and_push(m, env, s, g, 2.0)
    env.close()
    return out


def schedule(m, p):
    import open_times as OT
    env = OT.make_env(m, p)
    start, goal = p["start"].to_row(), p["goal"].to_row()
    kw = {"capacity": p["capacity"], "max_frontier": p["max_frontier"], "max_rounds": 20000}
    out = {"schedule": SCHEDULE, "anytime": [], "fresh": []}
    stage_ms, fresh_ms = [[] for _ in SCHEDULE], [[] for _ in SCHEDULE]
    for rep in range(REPS + 1):
        env.synchronize()
        t0 = time.perf_counter()
        r = env.search(start, goal, eps=SCHEDULE[0], **kw)
        ms = [(time.perf_counter() - t0) * 1e3]
        b = r.bound()
        rows = [{"eps": SCHEDULE[0], "status": m.search.STATUS_NAMES[r.status], "cost": r.cost, "lower": b["lower"], "ratio": b["ratio"],
                 "rounds": r.rounds, "expanded": r.expanded}]
        stopped = None
        for eps in SCHEDULE[1:]:
            t0 = time.perf_counter()
            r, st = m.search.anytime(r, [eps])
            ms.append((time.perf_counter() - t0) * 1e3)  # (improve and the bound's pass)
            s = st[0]
            rows.append({"eps": eps, "status": m.search.STATUS_NAMES[s["status"][0]], "cost": s["cost"][0], "lower": s["lower"][0],
                         "ratio": s["ratio"][0], "rounds": s["rounds"][0], "expanded": s["expanded"][0],
                         "pruned": r.rekey_info[0]["n_pruned"]})
            if s["certified"][0] and s["ratio"][0] <= 1.0 and stopped is None:
                stopped = eps  # (search.anytime with the whole schedule would stop here; the stages go on to be measured)
        nodes = r.table.stats()[0]
        r.free()
        fresh = []
        for i, eps in enumerate(SCHEDULE):
            env.synchronize()
            t0 = time.perf_counter()
            f = env.search(start, goal, eps=eps, **kw)
            fm = (time.perf_counter() - t0) * 1e3
            fresh.append({"eps": eps, "status": m.search.STATUS_NAMES[f.status], "cost": f.cost, "rounds": f.rounds, "expanded": f.expanded,
                          "nodes": f.table.stats()[0]})
            f.free()
            if rep:
                fresh_ms[i].append(fm)
        if rep:
            for i, x in enumerate(ms):
                stage_ms[i].append(x)
        out["anytime"], out["fresh"], out["anytime_nodes"], out["anytime_would_stop_at_eps"] = rows, fresh, nodes, stopped
    for i in range(len(SCHEDULE)):
        out["anytime"][i].update({"ms": med(stage_ms[i]), "ms_all": stage_ms[i]})
        out["fresh"][i].update({"ms": med(fresh_ms[i]), "ms_all": fresh_ms[i]})
    out["anytime_total_ms"] = float(sum(x["ms"] for x in out["anytime"]))
    out["four_fresh_total_ms"] = float(sum(x["ms"] for x in out["fresh"]))
    out["fresh_eps_1_ms"] = out["fresh"][-1]["ms"]
    env.close()
    return out


def corridor_table(m):
    import open_times as OT
    p = OT.corridor_problem(m)
    env = OT.make_env(m, p)
    start, goal = p["start"].to_row(), p["goal"].to_row()
    r = env.search(start, goal, capacity=p["capacity"], max_frontier=p["max_frontier"])
    d = r.table.download()
    r.free()
    env.set_goal(goal)
    out = rekey_and_push(m, env, d["state"], d["g"], 1.0)
    env.close()
    return out


def measure(path):
    import torch

    import motion_primitive_library_amd as m
    import open_times as OT
    out = {"device": torch.cuda.get_device_name(0), "repetitions": REPS, "calls_per_window": CALLS,
           "rekey": {"corridor_table": corridor_table(m), "seeded_2^20": million(m)},
           "schedule": {"corridor": schedule(m, OT.corridor_problem(m)), "plan3d_120": schedule(m, OT.plan3d_problem(m))}}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["rekey"]))
    for k, v in out["schedule"].items():
        print(k, "anytime", v["anytime_total_ms"], "four fresh", v["four_fresh_total_ms"], "fresh eps 1", v["fresh_eps_1_ms"])


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "measure":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "anytime_times.json"))
    else:
        print(__doc__)
