"""Time of the wait-edge launch (include/mplx_wait.h) and of the park veto (mplx_reserve_park_device, include/mplx_reserve.h)
next to the check, the relax and the push of the round they join, and of a corridor search with and without them.

    python profiles/micro/park_times.py measure [OUT.json [PARENT_ROOT]]   # GPU box; default profiles/park_times.json
    python profiles/micro/park_times.py corridor [ROOT]                    # the corridor figures alone, package from ROOT

Workload: that of profiles/micro/reserve_times.py -- 2-D, ACC, 81 controls, dt = 1, an all-free 256 x 256 map of 0.25 m
cells, a frontier of 4096 distinct states (4093 nodes) with t = (k mod 8) dt, lists of stride 96 -- with n_steps = 480
instants of step 0.25 and radii 0, so that nothing is blocked or vetoed and every call does the same, full work.
  add_wait  on the round's frontier as it is (velocities in quarters within +-1: few rows are at rest) and on the same
            frontier at rest (every row takes an entry).  The counts are put back before every window: a call appends.
  park      on the round's selection frontier (4093 rows) pushed into the open set, with a goal tolerance that makes
            every node a goal node (100 %) and one that takes about 1 % of them; a looked-at row walks every instant from
            its t to the horizon against all B reservations (pair_instants counts exactly those).
  check / relax / push of the same round beside them.
A timed window is CALLS = 5 back-to-back device calls between mplx_timer_begin / _end after one untimed call; the figure
is the window divided by CALLS, the median of REPS = 5 windows.
The search: EnvMap.search on the corridor of tests/golden, robot 1 on the way back against robot 0's plan, host clock,
median of 3: with avoid and both flags off (also from a build of the parent, PARENT_ROOT, in a child process), with
wait, and with wait and park_goal."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG_ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "corridor" else ROOT
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, PKG_ROOT)

N, REPS, CALLS, STEP, N_STEPS = 4096, 5, 5, 0.25, 480


def median(xs):
    return float(np.median(np.asarray(xs)))


def windows(env, call, before=None):
    if before:
        before()
    call()
    env.synchronize()
    out = []
    for _ in range(REPS):
        if before:
            before()
            env.synchronize()
        env.timer_begin()
        for _ in range(CALLS):
            call()
        out.append(env.timer_end() / CALLS)
        env.synchronize()
    return out


def round_times(m):
    rng = np.random.default_rng(77)
    nine = [-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0]
    U, stride = m.workloads.grid_controls(nine, 2), 96
    env = m.EnvMap(2)
    env.setMap([0.0, 0.0], [256, 256], np.zeros(256 * 256, np.int8), 0.25)
    env.set_control(m.ACC)
    env.set_u(U)
    env.set_v_max(2.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    F = env.n_fields
    st = np.zeros((F, N))
    cells = rng.permutation(200 * 200)[:N]
    st[0], st[1] = 7.0 + (cells % 200) * 0.25, 7.0 + (cells // 200) * 0.25
    st[2:4] = rng.integers(-4, 5, (2, N)) / 4.0
    tab = env.alloc_table(N * stride + N)
    opn = env.alloc_open(tab)
    fr, imp = m.TableFrontier(env, N), m.TableFrontier(env, N * stride)
    n = tab.seed(st, frontier=fr)
    tt = fr.download(n)["state"]
    tt[F - 1] = (np.arange(n) % 8) * 1.0
    up = np.zeros((F, N))
    up[:, :n] = tt
    fr.state.upload(up)
    lists = env.alloc_lists(N, want_state=True, stride=stride)
    out = {"controls": len(U), "stride": stride, "rows": n}
    out["expand_ms"] = median(windows(env, lambda: env.expand_lists_resident(fr, lists, n_nodes=n)))
    count0 = lists.count.download(np.int32, (N,))
    out["entries"] = int(count0[:n].sum())
    res0 = env.alloc_reservations((st[:, :1], np.zeros((1, 1), np.int32)), STEP, n_steps=N_STEPS, radius=0.0)
    d_na = m.DeviceArray(env, 8)

    def added(call):
        lists.count.upload(count0)
        d_na.upload(np.zeros(1, np.int64))
        call()
        env.synchronize()
        return int(d_na.download(np.int64, (1,))[0])
    # ---- add_wait: the round's frontier, then the same frontier at rest
    call = lambda: res0.add_waits(fr, lists, n, n_added=d_na)
    reset = lambda: lists.count.upload(count0)
    out["add_wait_round"] = {"added_per_call": added(call), "ms_all": windows(env, call, reset)}
    rest = up.copy()
    rest[2:4] = 0.0
    fr_rest = m.TableFrontier(env, N)
    fr_rest.id.upload(np.arange(N, dtype=np.int32))
    fr_rest.state.upload(rest)
    env.expand_lists_resident(fr_rest, lists, n_nodes=n)
    count_rest = lists.count.download(np.int32, (N,))
    call_r = lambda: res0.add_waits(fr_rest, lists, n, n_added=d_na)
    reset_r = lambda: lists.count.upload(count_rest)
    reset_r()
    d_na.upload(np.zeros(1, np.int64))
    call_r()
    env.synchronize()
    out["add_wait_at_rest"] = {"added_per_call": int(d_na.download(np.int64, (1,))[0]), "ms_all": windows(env, call_r, reset_r)}
    for k in ("add_wait_round", "add_wait_at_rest"):
        out[k]["ms"] = median(out[k]["ms_all"])
    # ---- the round again as it is, and what follows it
    env.expand_lists_resident(fr, lists, n_nodes=n)
    goal = np.zeros(F)
    goal[:2] = 32.0
    for B in (1024, 64):
        r_st = np.zeros((F, B))
        r_st[:2] = rng.uniform(7.0, 57.0, (2, B))
        r_ac = rng.integers(0, len(U), (8, B)).astype(np.int32)
        res = env.alloc_reservations((r_st, r_ac), STEP, n_steps=N_STEPS, t0=rng.integers(0, 9, B) / 4.0, radius=0.0)
        res.set_queries(0.0, 0.0)
        rec = {"check_ms": median(windows(env, lambda: res.check(fr, lists, n)))}
        for name, tol in (("goal_100pct", 1e9), ("goal_1pct", 2.5)):
            env.set_goal(goal, tol_pos=tol)
            opn.push(fr, n_max=n)
            env.synchronize()
            flags = opn.download()["flags"][:n]
            ids = fr.id.download(np.int32, (n,))
            is_goal = (flags[ids] & m.search.IS_GOAL) != 0
            ts = fr.state.download(np.float64, (F, N))[F - 1, :n]
            instants = np.maximum(N_STEPS - np.ceil(ts / STEP), 0)[is_goal].sum()
            d_nv = m.DeviceArray(env, 8)
            d_nv.upload(np.zeros(1, np.int64))
            w = windows(env, lambda: res.park(opn, fr, n, n_vetoed=d_nv))
            assert int(d_nv.download(np.int64, (1,))[0]) == 0
            pi = float(instants) * B
            rec["park_" + name] = {"goal_rows": int(is_goal.sum()), "ms": median(w), "ms_all": w, "pair_instants": pi,
                                   "pair_instants_per_s": pi / (median(w) * 1e-3)}
            d_nv.free()
        out["B%d" % B] = rec
        res.free()
    out["relax_ms"] = median(windows(env, lambda: tab.relax(lists, fr.id, fr.g, frontier=imp, n_nodes=n, want_count=False)))
    env.set_goal(goal, tol_pos=2.5)
    out["push_ms"] = median(windows(env, lambda: opn.push(imp, n_max=n * stride)))
    out["push_rows"] = int(imp.count.download(np.int64, (1,))[0])
    for b in (d_na, res0, fr_rest, lists, fr, imp, opn, tab):
        b.free()
    env.close()
    return out


def corridor_search(m):
    from test_gpu_open import corridor_env
    from test_multi import corridor_queries
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    r0 = env.search(starts[:, 0], goals[0], capacity=1 << 15, max_frontier=4096)
    p = r0.path()
    res = env.alloc_reservations((p[0].reshape(-1, 1), p[1].reshape(-1, 1)), STEP, n_steps=640, radius=0.4)
    cases = [("avoid_flags_off", {})]
    if hasattr(m._abi, "WAIT_SYMBOLS"):
        cases += [("avoid_wait", dict(wait=True)), ("avoid_wait_park_goal", dict(wait=True, park_goal=True))]
    out = {}
    for name, kw in cases:
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            r = env.search(starts[:, 2], goals[2], capacity=1 << 18, max_frontier=4096, avoid=res, radius=0.4, **kw)
            ts.append((time.perf_counter() - t) * 1e3)
            rec = {"status": r.status, "cost": r.cost, "rounds": r.rounds, "expanded": r.expanded, "nodes": r.table.stats()[0]}
            r.free()
        out[name] = dict(rec, wall_ms=median(ts), wall_ms_all=ts)
    res.free()
    r0.free()
    env.close()
    return out


def measure(path, parent_root):
    import motion_primitive_library_amd as m
    res = {"repetitions": REPS, "calls_per_window": CALLS, "step": STEP, "n_steps": N_STEPS}
    res["round_81"] = round_times(m)
    res["corridor"] = corridor_search(m)
    if parent_root:  # a build of the parent commit, in a process of its own
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "corridor", parent_root], capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise SystemExit("the parent's run failed:\n" + p.stderr)
        res["corridor_parent"] = json.loads(p.stdout.strip().splitlines()[-1])
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "measure":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "park_times.json"),
                sys.argv[3] if len(sys.argv) > 3 else None)
    elif len(sys.argv) >= 2 and sys.argv[1] == "corridor":
        import motion_primitive_library_amd as m
        assert os.path.abspath(m.__file__).startswith(PKG_ROOT), m.__file__
        print(json.dumps(corridor_search(m)))
    else:
        raise SystemExit(__doc__)
