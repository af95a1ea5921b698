"""Time of a goal distance field build (include/mplx_field.h) next to the host model of the same field, and of the trap
and corridor searches with and without a field.

    python profiles/micro/field_times.py measure [OUT.json]   # GPU box; default profiles/field_times.json

A build reads one counter back per pass, so it is timed by a host clock: one untimed call, then the median of REPS = 5
calls.  Builds: F = 1 and F = 64 on the corridor map of tests/golden and on a 512 x 512 maze (a random spanning tree of
256 x 256 rooms, walls one cell thick); F = 1 on the 3-D 160^3 map of workloads.make("C3", scale=160 / 256).  The pass
count is recorded beside each.  tests/field_model.py (a deque BFS in Python) is the only other route to the same field:
it is timed once per 2-D map for F = 1, and not on the 160^3 map (4.1 M cells, 26 neighbours: minutes).
Searches (eps = 1, delta = 0, host clock, median of 3): the trap of tests/test_gpu_field.py and the corridor, with
field=None and with a caller's field built beforehand, so that build and search show separately; and field=True, which
pays for both."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

REPS = 5


def median(xs):
    return float(np.median(np.asarray(xs)))


def maze(rooms=256, seed=9):
    """(2 rooms) x (2 rooms) cells: a random spanning tree of the rooms by an iterative depth-first walk."""
    rng = np.random.default_rng(seed)
    n = 2 * rooms
    c = np.full((n, n), 100, np.int8)
    seen = np.zeros((rooms, rooms), bool)
    stack = [(0, 0)]
    seen[0, 0] = True
    c[0, 0] = 0
    while stack:
        y, x = stack[-1]
        nb = [(y + dy, x + dx) for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1))
              if 0 <= y + dy < rooms and 0 <= x + dx < rooms and not seen[y + dy, x + dx]]
        if not nb:
            stack.pop()
            continue
        v, u = nb[int(rng.integers(len(nb)))]
        seen[v, u] = True
        c[2 * v, 2 * u] = 0
        c[y + v, x + u] = 0
        stack.append((v, u))
    return c.ravel()


def build_times(m, FM, dims, origin, cells, res, goal_pos, Fs, model=True):
    D = len(dims)
    env = m.EnvMap(D)
    env.setMap(list(origin), list(dims), cells, res)
    fld = env.alloc_field()
    out = {"dims": list(dims), "blocked_share": float(np.mean(cells == 100))}
    lo1, hi1 = FM.goal_box(goal_pos, 0.5, list(origin), res)
    for F in Fs:
        rng = np.random.default_rng(F)
        lo = [lo1] + [[int(rng.integers(0, dims[i])) for i in range(D)] for _ in range(F - 1)]
        hi = [hi1] + [[a + 2 for a in b] for b in lo[1:]]
        fld.build_boxes(lo, hi)
        ts = []
        for _ in range(REPS):
            t = time.perf_counter()
            fld.build_boxes(lo, hi)
            ts.append((time.perf_counter() - t) * 1e3)
        rec = {"ms": median(ts), "ms_all": ts, "passes": fld.passes}
        if F == 1:
            d = fld.dist()[0]
            rec["reached_share"], rec["largest_dist"] = float(np.mean(d >= 0)), int(d.max())
            if model:
                t = time.perf_counter()
                want = FM.field(FM.blocked_of(cells), dims, [lo1], [hi1])[0]
                rec["host_model_ms"] = (time.perf_counter() - t) * 1e3
                assert np.array_equal(d, want)
        out["F%d" % F] = rec
    fld.free()
    env.close()
    return out


def search_times(m, env, start, goal, kw):
    out = {}
    mine = env.alloc_field()
    t = time.perf_counter()
    mine.build(goal, 0.5)
    out["field_build_first_ms"] = (time.perf_counter() - t) * 1e3
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        mine.build(goal, 0.5)
        ts.append((time.perf_counter() - t) * 1e3)
    out["field_build_ms"], out["field_passes"] = median(ts), mine.passes
    for name, extra in (("plain", {}), ("callers_field", dict(field=mine)), ("field_true", dict(field=True))):
        ts = []
        for _ in range(4):  # (the first is untimed)
            t = time.perf_counter()
            r = env.search(start, goal, **dict(kw, **extra))
            ts.append((time.perf_counter() - t) * 1e3)
            rec = {"status": r.status, "cost": r.cost, "rounds": r.rounds, "expanded": r.expanded, "nodes": r.table.stats()[0]}
            r.free()
        out[name] = dict(rec, wall_ms=median(ts[1:]), wall_ms_all=ts[1:])
    mine.free()
    return out


def measure(path):
    import field_model as FM
    import motion_primitive_library_amd as m
    from test_gpu_field import trap_env
    from test_gpu_open import corridor_env
    from test_plan_known_answer import corridor
    res = {"repetitions": REPS}
    c = corridor()
    res["build_corridor"] = build_times(m, FM, c["dim"], c["origin"], np.asarray(c["cells"], np.int8).ravel(), c["res"], c["goal"], (1, 64))
    res["build_maze_512"] = build_times(m, FM, [512, 512], [0.0, 0.0], maze(), 0.25, [127.625, 127.625], (1, 64))
    wl = m.workloads.make("C3", scale=160.0 / 256.0, n_nodes=1)
    grid = np.ascontiguousarray(wl.grid, np.int8).ravel()
    res["build_3d_160"] = build_times(m, FM, list(wl.map_dim), list(wl.origin), grid, wl.res, [8.05, 8.05, 8.05], (1,), model=False)
    env, start, goal = trap_env(m)
    res["search_trap"] = search_times(m, env, start, goal, dict(eps=1.0, delta=0.0, capacity=1 << 17, max_frontier=1 << 13))
    env.close()
    env, start, goal = corridor_env(m)
    res["search_corridor"] = search_times(m, env, start, goal, dict(eps=1.0, delta=0.0, capacity=1 << 15, max_frontier=4096))
    res["search_corridor_default_delta"] = search_times(m, env, start, goal, dict(capacity=1 << 15, max_frontier=4096))
    env.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "measure":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "field_times.json"))
    else:
        raise SystemExit(__doc__)
