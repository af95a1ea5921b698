"""Times of the device trajectory calls (include/mplx_traj.h) at user size.

    python profiles/micro/traj_times.py measure [OUT.json]   # device-event times (GPU box); default profiles/traj_times.json
    python profiles/micro/traj_times.py trace                # a few calls per case, for a kernel trace of its own:
        rocprofv3 --kernel-trace --stats -d DIR -o t -- python profiles/micro/traj_times.py trace

Workload: K = 65 536 trajectories of H = 8 ACC segments (27 controls, dt 0.5) on C4's map (512^3, res 0.1), starts at
rest uniform in the inner 80 % of the map.  mplx_traj_info_device, mplx_traj_sample_device with N = 64 in both forms,
and mplx_traj_traverse_device with a short n (v_max 1: n = 40), a middle one (v_max 3: n = 120) and a long one (v_max 8: n = 320) for lanes 4 / 16 / 64
and the automatic rule.  Every call includes the chain launch that builds the segment table.  Beside every time: the
bytes the call writes to its outputs.  The first 512 trajectories of every result are compared with the numpy model
(tests/traj_model.py).  The reference on one host thread over the same trajectories:
tests/golden/make_traj_golden.py --time.

measure: one warm-up + 7 repetitions, median; mplx_timer_begin / _end (events on the context's stream).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, H, REPS, SAMPLE_N, CHECK = 65536, 8, 7, 64, 512
MD, ORG, RES, DT = [512] * 3, [0.0] * 3, 0.1, 0.5
V_MAX = {"short": 1.0, "mid": 3.0, "long": 8.0}
ACC = 0x03


def c4_map():
    import motion_primitive_library_amd.workloads as W
    return W.box_map(MD, RES, 0.15, 1004)  # C4's map (workloads.make("C4"))


def workload(kind, n=K):
    """A case dict in the form of tests/traj_model.py fixture_cases() (tests/golden/make_traj_golden.py --time reads it)."""
    import traj_model as M
    rng = np.random.default_rng(616)
    U = M.control_table(ACC, 3)
    starts = np.zeros((14, n))
    starts[:3] = rng.uniform(5.12, 46.08, size=(3, n))
    actions = rng.integers(0, len(U), size=(H, n)).astype(np.int32)
    grid = c4_map().ravel()
    return {"name": kind, "control": ACC, "dim": 3, "dt": DT, "U": U, "starts": starts, "actions": actions,
            "geo": (MD, ORG, RES), "grid": grid, "pot": None, "v_max": V_MAX[kind]}


def timed(env, fn, reps=REPS):
    ms = []
    for r in range(reps + 1):  # the first is the warm-up
        env.timer_begin()
        fn()
        t = env.timer_end()
        env.synchronize()
        if r:
            ms.append(t)
    return float(np.median(ms)), ms


def setup(m, case):
    from motion_primitive_library_amd.env import DeviceArray
    env = m.EnvMap(3, 0)
    env.setMap(ORG, MD, case["grid"], RES)
    env.set_control(ACC)
    env.set_dt(DT)
    env.set_u(case["U"])
    env.set_v_max(case["v_max"])
    d_s, d_a = DeviceArray(env, case["starts"].nbytes), DeviceArray(env, case["actions"].nbytes)
    d_s.upload(case["starts"])
    d_a.upload(case["actions"])
    return env, d_s, d_a


def measure(path):
    import motion_primitive_library_amd as m
    import traj_model as M
    res = {"repetitions": REPS, "trajectories": K, "horizon": H}
    case = workload("short")
    trajs = M.build_set(ACC, 3, DT, case["U"], case["starts"][:, :CHECK], case["actions"][:, :CHECK])
    env, d_s, d_a = setup(m, case)
    res["device"] = env.device_info()[0]
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

    info = env.alloc_traj_info(K, H)
    med, all_ms = timed(env, lambda: env.traj_info_resident(d_s, d_a, info, H))
    got = info.download()
    ok = bool(np.array_equal(bits(got["effort"][:, :CHECK]), bits(np.stack([t.effort for t in trajs], axis=1))))
    res["info"] = {"ms": med, "ms_all": all_ms, "bytes_written": K * (1 + 4 + 8 + 40), "equals_model": ok}
    print("info", json.dumps(res["info"]), flush=True)
    info.free()

    out = env.alloc_traj_samples(K, SAMPLE_N + 1)
    res["sample"] = {}
    for form, name, rows in ((m.TRAJ_COMMAND, "command", 15), (m.TRAJ_WAYPOINT, "waypoint", 13)):
        med, all_ms = timed(env, lambda: env.traj_sample_resident(d_s, d_a, out, H, N=SAMPLE_N, form=form))
        first = out.out.download(np.float64, (CHECK, SAMPLE_N + 1))  # row 0 (x) of the first trajectories
        ok = bool(np.array_equal(bits(first), bits(np.stack([t.sample(SAMPLE_N, form)[0] for t in trajs]))))
        nbytes = K * (SAMPLE_N + 1) * rows * 8
        res["sample"][name] = {"ms": med, "ms_all": all_ms, "bytes_written": nbytes, "gb_per_s": nbytes / (med * 1e-3) / 1e9,
                               "samples_per_s": K * (SAMPLE_N + 1) / (med * 1e-3), "equals_model": ok}
        print("sample", name, json.dumps(res["sample"][name]), flush=True)
    out.free()

    res["traverse"] = {}
    tout = env.alloc_traj_traverse(K)
    for kind in ("short", "mid", "long"):
        env.set_v_max(V_MAX[kind])
        want = M.traverse_set(trajs, case["grid"], None, MD, ORG, RES, V_MAX[kind], 0.1, 0.0)
        rec = {"v_max": V_MAX[kind], "n": int(want["n_samples"].max()) - 1, "bytes_written": K * (1 + 8 + 4 + 4 + 4), "lanes": {}}
        for lanes in (4, 16, 64, 0):
            med, all_ms = timed(env, lambda: env.traj_traverse_resident(d_s, d_a, tout, H, lanes=lanes))
            got = tout.download()
            ok = bool(np.array_equal(bits(got["cost"][:CHECK]), bits(want["cost"])) and
                      all(np.array_equal(got[k][:CHECK], want[k]) for k in ("n_samples", "n_cells", "stop_sample")))
            samples = int(np.where(got["stop_sample"] >= 0, got["stop_sample"] + 1, got["n_samples"]).sum())
            rec["lanes"]["auto" if lanes == 0 else str(lanes)] = {"ms": med, "ms_all": all_ms, "traj_per_s": K / (med * 1e-3),
                                                                  "samples_walked": samples, "equals_model": ok}
        rec["free_share"] = float((got["cost"] == 0).mean())
        res["traverse"][kind] = rec
        print("traverse", kind, json.dumps(rec), flush=True)
    env.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def trace():
    import motion_primitive_library_amd as m
    case = workload("short")
    env, d_s, d_a = setup(m, case)
    out = env.alloc_traj_samples(K, SAMPLE_N + 1)
    tout = env.alloc_traj_traverse(K)
    for _ in range(3):
        env.traj_sample_resident(d_s, d_a, out, H, N=SAMPLE_N)
        for kind in ("short", "long"):
            env.set_v_max(V_MAX[kind])
            for lanes in (4, 16, 64):
                env.traj_traverse_resident(d_s, d_a, tout, H, lanes=lanes)
        env.synchronize()
    print("trace ok", flush=True)
    env.close()


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "measure"
    if cmd == "measure":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "traj_times.json"))
    elif cmd == "trace":
        trace()
    else:
        raise SystemExit(__doc__)
