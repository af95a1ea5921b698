"""Times of the persistent node table (include/mplx_table.h), in one process:

    python profiles/micro/table_times.py measure OUT.json

  relax        one mplx_table_relax_device over the lists of a full-size C4 launch (65 536 nodes x 729 controls, about
               20.4 M successors, stride 736) into an EMPTY table (every key is inserted, every node created and
               emitted) and again into the FILLED one (every key found, no candidate lowers anything, empty frontier).
  post canon   mplx_post_lists_device with canon only over the same lists: the one-shot table / partition that answers
               "which successors of this batch are the same state", the yardstick for a table that lives one call.
  corridor     EnvMap.cost_to_come on the corridor of tests/golden (36 rounds, 21 677 nodes, 114 107 counting entries)
               end to end: wall clock, with its 37 count read-backs.
  host search  ns per relaxed edge of the host A* on the 3D problem of profiles/micro/plan3d_timing.py (relax_ms /
               relaxed of mplx_planner_timing), on the same box.

Event times (mplx_timer_begin / _end on the context's stream), one warm-up and REPS repetitions, median.  "Algorithmic
bytes" are what any implementation must move: per counting entry its hash and cost (16 B); per created node its hash, g,
pred, pred_action (24 B) and its state column read and written (2 x 8 (4D+2) B); per emitted node its frontier row (12 B)
and its state rows read and written (2 x 8 (4D+2) B).  Scratch, slots and atomics are the implementation's own."""
import ctypes as C
import json
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


def c4_relax(m, res):
    wl = m.workloads.make("C4")
    env = m.EnvMap(3, 0)
    wl.apply(env)
    res["device"] = env.device_info()[0]
    n, F = wl.n_nodes, 14
    frontier = env.upload_frontier(wl.nodes)
    lists = env.alloc_lists(n, want_state=True)
    env.expand_lists_resident(frontier, lists)
    env.synchronize()
    S = lists.stride
    successors = int(lists.count.download(np.int32, (n,)).sum())
    pid = m.DeviceArray(env, n * 4)
    pid.upload(np.arange(n, dtype=np.int32))
    pg = m.DeviceArray(env, n * 8)
    pg.upload(np.zeros(n))
    eid = m.DeviceArray(env, n * S * 4)
    tab = env.alloc_table(successors)
    fr = m.TableFrontier(env, successors)
    empty_ms, filled_ms = [], []
    for r in range(REPS + 1):
        tab.clear()
        env.synchronize()
        env.timer_begin()
        tab.relax(lists, pid, pg, frontier=fr, entry_id=eid, want_count=False)
        ms = env.timer_end()
        emitted = int(fr.count.download(np.int64, (1,))[0])
        nodes, status = tab.stats()
        assert status == 0, status
        if r:
            empty_ms.append(ms)
    counting = int((eid.download(np.int32, (n * S,)) >= 0).sum())
    for r in range(REPS + 1):
        env.timer_begin()
        tab.relax(lists, pid, pg, frontier=fr, want_count=False)
        ms = env.timer_end()
        assert int(fr.count.download(np.int64, (1,))[0]) == 0 and tab.stats() == (nodes, 0)
        if r:
            filled_ms.append(ms)
    # the one-shot yardstick: node identity of the batch alone
    canon = m.DeviceArray(env, n * S * 4)
    goal = np.zeros(F)
    g = m._abi.GoalSpec()
    g.goal, g.control, g.w, g.v_max, g.tol_pos, g.tol_vel, g.tol_acc, g.tol_yaw = goal.ctypes.data, m.ACC, 10.0, 2.0, 0.5, -1.0, -1.0, -1.0
    o = m._abi.Post()
    o.canon = canon.ptr
    s = lists.c_struct()
    s.state = None  # (lists without state rows: the identity pass alone, no heuristic / flags kernel behind it)
    canon_ms = []
    for r in range(REPS + 1):
        env.timer_begin()
        m._abi.check(env._ctx, m._abi.lib().mplx_post_lists_device(env._ctx, C.byref(s), n, C.byref(g), C.byref(o)))
        ms = env.timer_end()
        if r:
            canon_ms.append(ms)
    e_ms, f_ms = med(empty_ms), med(filled_ms)
    bytes_empty = counting * 16 + nodes * (24 + 16 * F) + emitted * (12 + 16 * F)
    res["c4"] = {"nodes_expanded": n, "stride": S, "list_slots": n * S, "successors": successors, "counting_entries": counting,
                 "table_nodes": nodes, "emitted": emitted,
                 "relax_empty_ms": e_ms, "relax_empty_ms_all": empty_ms, "relax_empty_ns_per_counting_entry": e_ms * 1e6 / counting,
                 "relax_empty_algorithmic_GBps": bytes_empty / (e_ms * 1e-3) / 1e9,
                 "relax_filled_ms": f_ms, "relax_filled_ms_all": filled_ms, "relax_filled_ns_per_counting_entry": f_ms * 1e6 / counting,
                 "relax_filled_algorithmic_GBps": counting * 16 / (f_ms * 1e-3) / 1e9,
                 "post_canon_ms": med(canon_ms), "post_canon_ms_all": canon_ms, "post_canon_ns_per_successor": med(canon_ms) * 1e6 / successors,
                 "identity_form": env.last_identity_form()}
    print("c4", json.dumps(res["c4"]), flush=True)
    tab.free()
    for b in (fr, canon, eid, pid, pg, lists, frontier):
        b.free()
    env.close()


def corridor_sweep(m, res):
    from test_plan_known_answer import corridor
    c = corridor()
    env = m.EnvMap(2)
    env.setMap(c["origin"], c["dim"], c["cells"], c["res"])
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    start = m.Waypoint(2, m.ACC, pos=c["start"]).to_row()
    wall = []
    for r in range(REPS + 1):
        t0 = time.perf_counter()
        tab, rounds = env.cost_to_come(start, g_max=351.5, capacity=1 << 15, max_frontier=2048)
        ms = (time.perf_counter() - t0) * 1e3
        nodes = tab.stats()[0]
        tab.free()
        if r:
            wall.append(ms)
    counting = 114107  # tests/test_table.py counts them
    res["corridor"] = {"rounds": rounds, "nodes": nodes, "counting_entries": counting, "sweep_wall_ms": med(wall), "sweep_wall_ms_all": wall,
                       "ms_per_round": med(wall) / rounds, "wall_ns_per_counting_entry": med(wall) * 1e6 / counting}
    print("corridor", json.dumps(res["corridor"]), flush=True)
    env.close()


def host_search(m, res, edge=120):
    import bench
    W = m.workloads
    r_ = 0.1
    grid = W.box_map([edge] * 3, r_, 0.08, 4242, side_m=(0.5, 2.5))
    flat = grid.ravel()
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
    r = bench.engine_plan(m, 3, [0.0] * 3, [edge] * 3, flat, r_, U3, s3, g3, 2.0, 2.0, 64, reps=3)
    sp = r["timing_split"]
    res["host_search"] = {"edge": edge, "batch": 64, "wall_ms": r["wall_ms"], "relax_ms": sp["relax_ms"], "relaxed_edges": sp["relaxed"],
                          "ns_per_relaxed_edge": sp["relax_ms"] * 1e6 / max(sp["relaxed"], 1)}
    print("host_search", json.dumps(res["host_search"]), flush=True)


def measure(path):
    import motion_primitive_library_amd as m
    res = {"repetitions": REPS}
    corridor_sweep(m, res)
    host_search(m, res)
    c4_relax(m, res)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "measure":
        measure(sys.argv[2])
    else:
        raise SystemExit(__doc__)
