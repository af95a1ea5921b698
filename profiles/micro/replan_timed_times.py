"""Time of the timed rebase (include/mplx_replan_timed.h): its reservation pass alone, and a whole replan_timed against a
fresh timed search from the same root.

    python profiles/micro/replan_timed_times.py [OUT.json]      # GPU box; default profiles/replan_timed_times.json

The protocol of DESIGN.md 4.18: one untimed call, then windows of CALLS = 5 device calls between mplx_timer_begin /
_end; the figure is the window divided by CALLS, the median of REPS = 5 windows.

Reservation pass.  The table of a corridor search among reservations (tests/golden's corridor, robot 1 on the way back
against robot 0's plan, time keys and waits, stopped after enough rounds for about 13 000 nodes).  rebase_timed with
check_edges = 0 and the seed as root, against B = 64 and B = 1024 reservations of radius 0 with a query of radius 0:
nothing is blocked, so the table is the same after every call and every call does the same, full work (every instant
of every edge against every reservation).  The same call with res = NULL is the rebase's other launches; the
difference is the pass (and the memset of its bad bytes).

Whole replan.  The same corridor, searched to the goal with wait and park_goal; robot 1 has made K = 4 primitives, robot 0
is delayed by 2 s.  replan_timed on the table against EnvMap.search from the root state (t = 0, t0 + t_root, start_g =
g_root), host clock, median of 3; each replan consumes a result, so the search is run again before each (not timed)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

REPS, CALLS, STEP, N_STEPS, K, DELAY = 5, 5, 0.25, 640, 4, 2.0


def median(xs):
    return float(np.median(np.asarray(xs)))


def windows(env, call):
    call()
    env.synchronize()
    out = []
    for _ in range(REPS):
        env.timer_begin()
        for _ in range(CALLS):
            call()
        out.append(env.timer_end() / CALLS)
        env.synchronize()
    return out


def main(path):
    import motion_primitive_library_amd as m
    from test_gpu_open import corridor_env
    from test_multi import corridor_queries
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    r0 = env.search(starts[:, 0], goals[0], capacity=1 << 15, max_frontier=4096)
    p = r0.path()
    chain0 = (p[0].reshape(-1, 1), p[1].reshape(-1, 1))
    res = env.alloc_reservations(chain0, STEP, n_steps=N_STEPS, radius=0.4)
    kw = dict(capacity=1 << 18, max_frontier=4096, avoid=res, radius=0.4, wait=True)
    out = {"repetitions": REPS, "calls_per_window": CALLS, "step": STEP, "n_steps": N_STEPS}
    # ---- the reservation pass alone
    part, rounds = None, 8
    while rounds < 4096:
        cand = env.search(starts[:, 2], goals[2], max_rounds=rounds, **kw)
        done = cand.status != m.search.MAX_ROUNDS
        if part is not None:
            part.free()
        part = cand
        if part.table.stats()[0] >= 13000 or done:
            break
        rounds *= 2
    tab = part.table
    n = tab.stats()[0]
    kept = m.TableFrontier(env, tab.capacity)
    rng = np.random.default_rng(5)
    rec = {"nodes": n, "rounds": rounds}
    rec["no_res_ms_all"] = windows(env, lambda: tab.rebase_timed([-1], check_edges=False, allow_wait=True, frontier=kept, want_result=False))
    rec["no_res_ms"] = median(rec["no_res_ms_all"])
    for B in (64, 1024):
        r_st = np.zeros((env.n_fields, B))
        r_st[:2] = rng.uniform(2.0, 30.0, (2, B))
        r_ac = rng.integers(0, len(env._U_host), (8, B)).astype(np.int32)
        table = env.alloc_reservations((r_st, r_ac), STEP, n_steps=N_STEPS, t0=rng.integers(0, 9, B) / 4.0, radius=0.0)
        table.set_queries(0.0, 0.0)
        info = tab.rebase_timed([-1], check_edges=False, allow_wait=True, avoid=table, frontier=kept)
        assert info["n_blocked"] == 0 and info["n_kept"] == n, info
        w = windows(env, lambda: tab.rebase_timed([-1], check_edges=False, allow_wait=True, avoid=table, frontier=kept, want_result=False))
        rec["B%d" % B] = {"ms": median(w), "ms_all": w, "pass_ms": median(w) - rec["no_res_ms"]}
        table.free()
    w = windows(env, lambda: tab.rebase_timed([-1], check_edges=True, allow_wait=True, frontier=kept, want_result=False))
    rec["edges_no_res_ms"] = median(w)
    out["reservation_pass"] = rec
    kept.free()
    part.free()
    # ---- a whole replan against a fresh search from the same root
    kw["park_goal"] = True
    t_replan, t_fresh, t_search = [], [], []
    for _ in range(3):
        res.fill(chain0, STEP, N_STEPS, None, 0.4, None, True)
        t = time.perf_counter()
        r1 = env.search(starts[:, 2], goals[2], **kw)
        t_search.append((time.perf_counter() - t) * 1e3)
        root = int(r1.table.path(r1.goal_id)[0][K])
        s = r1.table.state_of(root)
        g_root = float(r1.table._read(r1.table.view().g + 8 * root, np.float64, 1)[0])
        t_root = float(s[-1])
        s[-1] = 0.0
        res.fill(chain0, STEP, N_STEPS, [DELAY], 0.4, None, True)
        env.synchronize()
        t = time.perf_counter()
        new = r1.replan_timed(avoid=res, advance=K)
        t_replan.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        fresh = env.search(s, goals[2], t0=t_root, start_g=g_root, **kw)
        t_fresh.append((time.perf_counter() - t) * 1e3)
        last = {"replan": {"status": new.status, "cost": new.cost, "rounds": new.rounds, "expanded": new.expanded, "rebase": new.rebase_info},
                "fresh": {"status": fresh.status, "cost": fresh.cost, "rounds": fresh.rounds, "expanded": fresh.expanded},
                "first_search": {"cost": r1.cost if hasattr(r1, "cost") else None}}
        new.free()
        fresh.free()
    out["whole"] = dict(last, replan_ms=median(t_replan), replan_ms_all=t_replan, fresh_ms=median(t_fresh), fresh_ms_all=t_fresh,
                        first_search_ms=median(t_search), advance=K, delay=DELAY)
    res.free()
    r0.free()
    env.close()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "replan_timed_times.json"))
