"""Times of MapUtil's map operations on the device (include/mplx_map_util.h) on C4's map (512^3, 15 % occupied).

    python profiles/micro/map_util_times.py measure OUT.json   # device-event times (GPU box)
    python profiles/micro/map_util_times.py trace              # the same calls once each, for a kernel trace of its own:
        rocprofv3 --kernel-trace --stats -d DIR -o m -- python profiles/micro/map_util_times.py trace
    python profiles/micro/map_util_times.py merge OUT.json KERNEL_TRACE.csv REF.json RESULT.json

measure: one warm-up, 7 repetitions, median, each call bracketed by mplx_timer_begin / _end (events on the
context's stream; the call's own synchronisation is inside the bracket).  dilate (26-box; ball r = 3), freeUnknown and
freeAll start every repetition from C4's map (uploaded outside the bracket); getCloud is timed as its count pass (count +
scan, xyz = NULL) under events and as the whole call with the copy of the points to the host on the wall clock.  The
first expansion after a dilate rebuilds the blocked bits and the free-box table: timed against the second one.
merge: adds the kernel times of the trace, the reference's one-thread dilate time (tests/golden/make_map_util_golden.py
--time, measured on the CPU build machine, not on the GPU box's host) and the byte floor.
"""
import ctypes as C
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

EDGE = 512
COPY_TBS = 6.29   # measured device copy rate, TB/s
PEAK_TBS = 8.0    # HBM roofline, TB/s
REPS = 7


def offsets():
    r = np.arange(-3, 4)
    g = np.array(np.meshgrid(r, r, r, indexing="ij")).reshape(3, -1).T[:, ::-1]
    box = g[(np.abs(g) <= 1).all(axis=1) & (np.abs(g).sum(axis=1) > 0)]
    ball = g[(g ** 2).sum(axis=1) <= 9]
    assert len(box) == 26 and len(ball) == 123
    return {"box26": np.ascontiguousarray(box, np.int32), "ball_r3": np.ascontiguousarray(ball, np.int32)}


def setup(n_nodes=4096):
    import motion_primitive_library_amd as m
    wl = m.workloads.make("C4", n_nodes=n_nodes)
    env = m.EnvMap(3, 0)
    wl.apply(env)
    return m, wl, env


def timed(m, env, fn):
    L = m._abi.lib()
    ms = C.c_float()
    m._abi.check(env._ctx, L.mplx_timer_begin(env._ctx))
    fn()
    m._abi.check(env._ctx, L.mplx_timer_end(env._ctx, C.byref(ms)))
    return float(ms.value)


def series(m, env, wl, fn, reset=True):
    out = []
    for r in range(REPS + 1):  # the first is the warm-up
        if reset:
            env.setMap(wl.origin, wl.map_dim, wl.grid, wl.res)
        t = timed(m, env, fn)
        if r:
            out.append(t)
    return {"median_ms": float(np.median(out)), "ms": out}


def measure(path):
    m, wl, env = setup()
    flat = np.ascontiguousarray(wl.grid).ravel()
    n = flat.size
    res = {"map": "C4 (workloads.make('C4')): %d^3, %.4f occupied, %d unknown" % (EDGE, float((flat == 100).mean()), int((flat == -1).sum())),
           "n_cells": int(n), "device": env.device_info()[0], "repetitions": REPS}
    L = m._abi.lib()
    for k, off in offsets().items():
        res["dilate_" + k] = series(m, env, wl, lambda: env.dilate(off, read_back=False))
        env.setMap(wl.origin, wl.map_dim, wl.grid, wl.res)
        new = env.dilate(off)
        res["dilate_" + k]["changed_cells"] = int((new != flat).sum())
    res["freeUnknown"] = series(m, env, wl, lambda: env.freeUnknown(read_back=False))
    res["freeAll"] = series(m, env, wl, lambda: env.freeAll(read_back=False))
    env.setMap(wl.origin, wl.map_dim, wl.grid, wl.res)
    cnt = C.c_int64()
    res["getCloud_count_scan"] = series(m, env, wl, lambda: m._abi.check(env._ctx, L.mplx_map_cloud(env._ctx, 0, None, 0, C.byref(cnt))),
                                        reset=False)
    res["getCloud_count_scan"]["points"] = int(cnt.value)
    wall = []
    for r in range(REPS + 1):
        t0 = time.perf_counter()
        pts = env.getCloud()
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
    res["getCloud_whole_call_wall"] = {"median_ms": float(np.median(wall)), "ms": wall, "points": int(len(pts)),
                                       "note": "count + scan + fill + copy of %d MB of points to pageable host memory" % (pts.nbytes >> 20)}
    del pts
    # the expansion after a dilate: blocked bits + free-box table rebuilt by the first one
    fr = env.upload_frontier(wl.nodes)
    lists = env.alloc_lists(wl.n_nodes, want_state=False)
    first, second = [], []
    for r in range(REPS + 1):
        env.setMap(wl.origin, wl.map_dim, wl.grid, wl.res)
        env.dilate(offsets()["box26"], read_back=False)
        a = timed(m, env, lambda: env.expand_lists_resident(fr, lists))
        b = timed(m, env, lambda: env.expand_lists_resident(fr, lists))
        if r:
            first.append(a)
            second.append(b)
    res["expansion_after_dilate"] = {"nodes": int(wl.n_nodes), "route": env.last_lists_route(),
                                     "first_median_ms": float(np.median(first)), "second_median_ms": float(np.median(second)),
                                     "first_ms": first, "second_ms": second}
    env.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in res.items()}, indent=1))


def trace():
    m, wl, env = setup()
    off = offsets()
    fr = env.upload_frontier(wl.nodes)
    lists = env.alloc_lists(wl.n_nodes, want_state=False)
    env.expand_lists_resident(fr, lists)
    env.synchronize()
    for k in ("box26", "ball_r3"):
        env.setMap(wl.origin, wl.map_dim, wl.grid, wl.res)
        env.dilate(off[k], read_back=False)
    env.expand_lists_resident(fr, lists)  # the first expansion after the dilate: blocked bits + free-box table
    env.synchronize()
    env.setMap(wl.origin, wl.map_dim, wl.grid, wl.res)
    env.freeUnknown(read_back=False)
    n = len(env.getCloud())
    env.freeAll(read_back=False)
    env.close()
    print("trace ok: %d occupied cells" % n)


def short_name(name):
    """The kernel's own name out of its demangled signature."""
    m = re.search(r"(\w+)(?:<[^()]*>)?\(", name.replace("(anonymous namespace)", ""))
    return m.group(1) if m else name


def merge(dev_path, trace_path, ref_path, out_path):
    """trace_path: the per-dispatch kernel trace (rocprofv3 --kernel-trace: *_kernel_trace.csv) of `trace`."""
    dev = json.load(open(dev_path))
    n = dev["n_cells"]
    disp = []
    with open(trace_path) as f:
        for row in csv.DictReader(f):
            disp.append((int(row["Start_Timestamp"]), short_name(row["Kernel_Name"]),
                         (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    disp.sort()
    calls = {}
    for _, k, us in disp:
        calls.setdefault(k, []).append(us)
    out = {"device_event_times": dev, "kernel_trace_us": calls,
           "trace_order": "expansion (setup), dilate box26, dilate ball_r3, first expansion after the dilate (blocked bits + "
                          "free-box table), freeUnknown, getCloud (count, scan, fill), freeAll (a memset: no kernel)",
           "reference_cpu": json.load(open(ref_path))}
    floor = {"rule": "dilation reads the int8 map once and writes the cells it changes; bytes / 6.29 TB/s (measured copy "
                     "rate); roofline share = algorithmic bytes / kernel time / 8 TB/s",
             "map_bytes": n, "floor_us_map_read": n / (COPY_TBS * 1e12) * 1e6}
    pk, ap = calls.get("pack_occupancy_kernel", []), calls.get("dilate_apply_kernel", [])
    for i, k in enumerate(("box26", "ball_r3")):
        if i < len(pk) and i < len(ap):
            alg = n + dev["dilate_" + k]["changed_cells"]
            t_us = pk[i] + ap[i]
            f_us = alg / (COPY_TBS * 1e12) * 1e6
            floor["dilate_" + k] = {"pack_us": pk[i], "apply_us": ap[i], "kernel_us": t_us, "algorithmic_bytes": alg,
                                    "floor_us": f_us, "kernel_over_floor": t_us / f_us,
                                    "roofline_share": alg / (t_us * 1e-6) / (PEAK_TBS * 1e12)}
    fu = calls.get("free_unknown_kernel", [])
    if fu:
        floor["freeUnknown"] = {"kernel_us": fu[0], "floor_us": floor["floor_us_map_read"],
                                "kernel_over_floor": fu[0] / floor["floor_us_map_read"]}
    cc, cf, sc = calls.get("cloud_count_kernel", []), calls.get("cloud_fill_kernel", []), calls.get("scan_counts_kernel", [])
    if cc and cf and sc:
        pts = dev["getCloud_count_scan"]["points"]
        t_us = cc[-1] + sc[-1] + sum(cf)  # the call that fills: its count pass, its scan, every fill window
        floor["getCloud"] = {"count_us": cc[-1], "scan_us": sc[-1], "fill_us": sum(cf), "fill_windows": len(cf),
                             "kernel_us": t_us, "bytes_map_twice_plus_points": n * 2 + pts * 24,
                             "roofline_share": (n * 2 + pts * 24) / (t_us * 1e-6) / (PEAK_TBS * 1e12)}
    bb = [calls.get(k, []) for k in ("build_blocked_bits_kernel", "sat_seed_kernel", "sat_scan_x_kernel", "sat_scan_y_kernel",
                                     "sat_scan_z_kernel")]
    if all(bb):
        floor["first_expansion_after_a_dilate"] = {"blocked_bits_us": bb[0][-1], "free_box_table_us": sum(b[-1] for b in bb[1:]),
                                                   "note": "rebuilt by the first expansion after any map change, as after mplx_set_map"}
    out["byte_floor"] = floor
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(floor, indent=1))


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "measure"
    if cmd == "measure":
        measure(sys.argv[2])
    elif cmd == "trace":
        trace()
    elif cmd == "merge":
        merge(*sys.argv[2:6])
    else:
        raise SystemExit(__doc__)
