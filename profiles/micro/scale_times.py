"""Times of sampling a time-scaled trajectory set (include/mplx_scale.h) against plain sampling of the same set.

    python profiles/micro/scale_times.py measure [OUT.json]   # device-event times (GPU box); default profiles/scale_times.json

Workload: K = 65 536 loaded 3-D trajectories of S = 5 quintic segments (coefficients sixteenths in +-2, durations quarters
in [0.5, 3]), scale(ri, rf) with ratios from [0.25, 4] per trajectory.  mplx_poly_scale_device in both modes, then
mplx_poly_sample_device with N = 64 Commands: without a Lambda, with a REFERENCE one, with a ROBUST one; and
mplx_poly_tau_device alone.  Beside every time: the bytes the call writes to its outputs.  The x row of the first 256
trajectories of the ROBUST samples is compared with the numpy model (tests/scale_model.py) evaluated at the device's own
tau.  The reference on one host thread over the same kind of set: tests/golden/make_scale_golden.py --time.

measure: a timed window is CALLS = 50 back-to-back calls between mplx_timer_begin / _end (events on the context's
stream), so a window lasts milliseconds, not one launch; the figure is the window divided by CALLS.  The three sampling
variants alternate inside every one of the REPS = 7 rounds (plain, REFERENCE, ROBUST, each after its own untimed state
change and one untimed warm-up call), so drift of the clocks falls on all three alike; median over the rounds.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, S, REPS, CALLS, SAMPLE_N, CHECK = 65536, 5, 7, 50, 64, 256
RATIOS = [0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0]
JRKxYAW = 0x17


def workload(n=K):
    """coeff [n][S][4][6], dts [n][S], ri, rf [n]: the layout of tests/golden/make_scale_golden.py run_case."""
    rng = np.random.default_rng(909)
    coeff = rng.integers(-32, 33, (n, S, 4, 6)).astype(np.float64) / 16.0
    coeff[:, :, 3, :4] = 0.0
    dts = rng.integers(2, 13, (n, S)).astype(np.float64) / 4.0
    return coeff, dts, rng.choice(RATIOS, n), rng.choice(RATIOS, n)


def window(env, fn, calls=CALLS):
    """Milliseconds per call over one window of `calls` calls, after one untimed call."""
    fn()
    env.synchronize()
    env.timer_begin()
    for _ in range(calls):
        fn()
    t = env.timer_end()
    env.synchronize()
    return t / calls


def measure(path):
    import motion_primitive_library_amd as m
    import scale_model as SM
    coeff, dts, ri, rf = workload()
    env = m.EnvMap(3, 0)
    env.set_control(JRKxYAW)
    res = {"repetitions": REPS, "trajectories": K, "segments": S, "samples": SAMPLE_N + 1, "device": env.device_info()[0]}
    poly = env.load_traj(np.ascontiguousarray(coeff.transpose(1, 2, 3, 0)), np.ascontiguousarray(dts.T), control=JRKxYAW)
    d_ri, d_rf = m.DeviceArray(env, K * 8), m.DeviceArray(env, K * 8)
    d_ri.upload(ri)
    d_rf.upload(rf)
    rows = env.alloc_lambda_rows(K, S + 1, SAMPLE_N + 1)
    out = env.alloc_traj_samples(K, SAMPLE_N + 1)
    nbytes = K * (SAMPLE_N + 1) * 15 * 8
    names = ("plain", "reference", "robust")
    ms = {"sample_" + n: [] for n in names}
    ms.update({"tau_" + n: [] for n in names[1:]})
    ms.update({"scale_" + n: [] for n in names[1:]})
    for _ in range(REPS):
        for name in names:  # the variants alternate within a round
            if name == "plain":
                poly.clear_lambda()
            else:
                ms["scale_" + name].append(window(env, lambda: poly.scale_resident(rows, d_ri, d_rf, robust=name == "robust")))
            ms["sample_" + name].append(window(env, lambda: poly.sample_resident(out, N=SAMPLE_N)))
            if name != "plain":
                ms["tau_" + name].append(window(env, lambda: poly.tau_resident(rows, N=SAMPLE_N)))
    res["calls_per_window"] = CALLS
    for key, v in ms.items():
        res[key] = {"ms": float(np.median(v)), "ms_all": v}
        if key.startswith("sample_"):
            res[key].update({"bytes_written": nbytes, "samples_per_s": K * (SAMPLE_N + 1) / (res[key]["ms"] * 1e-3)})
    for name in names[1:]:
        res["sample_" + name]["over_plain"] = res["sample_" + name]["ms"] / res["sample_plain"]["ms"]
        res["scale_" + name]["bytes_written"] = K * (1 + 4 + 8 + (S + 1) * 8 + 64)
    # the poly holds the ROBUST Lambda of the last round: its rows against the model at the device's own tau
    poly.sample_resident(out, N=SAMPLE_N)
    poly.tau_resident(rows, N=SAMPLE_N)
    env.synchronize()
    x = out.out.download(np.float64, (CHECK, SAMPLE_N + 1))
    tau = rows.download()["tau"][:CHECK]
    ok = True
    for k in range(CHECK):
        taus = np.concatenate([[0.0], np.cumsum(dts[k])])  # (quarters: exact in any order)
        r = SM.scale(taus, ri[k], rf[k], SM.ROBUST)
        for i in (0, 7, 31, SAMPLE_N):
            t, l, ld = r["lam"].clamp_eval(tau[k, i], r["total"], taus[-1])
            want = SM.sample_rows(coeff[k][:, :3, :], coeff[k][:, 3, :], taus, t, l, ld, 0.0, True)[0]
            ok = ok and np.float64(want).view(np.uint64) == x[k, i].view(np.uint64)
    res["sample_robust"]["equals_model"] = bool(ok)
    for key in sorted(ms):
        print(key, json.dumps({k: v for k, v in res[key].items() if k != "ms_all"}), "min %.4f max %.4f" % (min(ms[key]), max(ms[key])), flush=True)
    env.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "measure"
    if cmd == "measure":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "scale_times.json"))
    else:
        raise SystemExit("usage: scale_times.py measure [OUT.json]")
