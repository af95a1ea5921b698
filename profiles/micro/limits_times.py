"""Times of the dynamic limits of a solved set (include/mplx_limits.h): K = 4096 problems of W = 17 waypoints in 3-D,
smoothing order 2 (JRK ends), so every segment is a full quintic and the velocity extrema go through the cubic.

    python profiles/micro/limits_times.py OUT.json [K]

  solve            one mplx_solve_device, for scale (profiles/micro/solve_times.py measures it in its own right)
  limits_ref       one mplx_poly_limits_device in MPLX_LIMITS_REFERENCE mode: K x 16 lanes of poly_limits_kernel, then
                   the reduction over each problem's segments
  limits_all       the same in MPLX_LIMITS_ALL_ROOTS mode
  load             one mplx_poly_load_device of the K x 16 segments the solve produced (resident coefficients)
  shortcut         one mplx_shortcut_device of Q = 64 of the same paths as chains of 17 states one second apart (max_hop =
                   16: 64 x 16 x 16 pair problems), on a free 96^3 map: pairs, solve, info, limits, traverse, costs,
                   programme and gather, queued without a read-back; polys and outputs allocated before

The device times are the context's timer (events on its stream) around the launches, one warm-up and REPS = 7
repetitions; medians and all samples are reported.  No threshold is set."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REPS = 7


def main(out_path, K):
    import torch  # noqa: F401  before the library: both then share the HIP runtime
    import motion_primitive_library_amd as m
    from solve_times import D, W, problem_set
    wp, v = problem_set(K)
    env = m.EnvMap(D)
    env.set_control(m.JRK)
    env.set_v_max(2.0)
    d_wp, d_v = m.DeviceArray(env, wp.nbytes), m.DeviceArray(env, v.nbytes)
    d_wp.upload(wp)
    d_v.upload(v)
    poly = env.alloc_poly(K, W)
    out = env.alloc_solve_out(K, W, m.JRK)
    lim = env.alloc_poly_limits(K)
    res = {"K": K, "W": W, "D": D, "so": 2, "reps": REPS, "device": env.device_info()}

    def solve():
        env.solve_traj_resident(poly, d_wp, K, W, v_arr=d_v, control=m.JRK, out=out)

    def timed(name, fn):
        samples = []
        for rep in range(REPS + 1):
            env.synchronize()
            env.timer_begin()
            fn()
            ms = env.timer_end()
            if rep:
                samples.append(ms)
        res[name + "_ms"] = {"median": float(np.median(samples)), "samples": samples}

    timed("solve", solve)
    for name, all_roots in (("limits_ref", False), ("limits_all", True)):
        timed(name, lambda: poly.limits_resident(lim, 2.0, 3.0, 0.0, all_roots=all_roots))
        env.synchronize()
        d = lim.download()
        res[name + "_valid"] = int(d["valid"].sum())
        res[name + "_peak_vel"] = float(d["max_vel"].max())
    assert not poly.status.any()
    seg, dts = poly.segments(), poly.dts()
    d_seg, d_dts = m.DeviceArray(env, seg.nbytes), m.DeviceArray(env, dts.nbytes)
    d_seg.upload(seg)
    d_dts.upload(dts)
    loaded = env.alloc_poly(K, W)
    timed("load", lambda: env.load_traj_resident(loaded, d_seg, d_dts, K, W, control=m.JRK))
    import ctypes as C
    Q, hop = 64, W - 1
    env.setMap([0.0, 0.0, 0.0], [96, 96, 96], np.zeros(96 ** 3, np.int8), 0.25)
    env._flush()
    st = np.ascontiguousarray(wp[:, :, :Q])
    st[4 * D + 1] = np.arange(W, dtype=np.float64)[:, None]
    d_st = m.DeviceArray(env, st.nbytes)
    d_st.upload(st)
    P = Q * (W - 1) * hop
    pairs, short = env.alloc_poly(P, 2), env.alloc_poly(Q, W)
    outs = [m.DeviceArray(env, n) for n in (Q, Q * 4, W * Q * 4, Q * 8, Q * 8)]
    i, o = m._abi.ShortcutIn(), m._abi.ShortcutOut()
    i.states, i.n_query, i.w_max, i.control, i.stride, i.max_hop = d_st.ptr, Q, W, m.JRK, Q, hop
    o.status, o.n_keep, o.keep, o.cost, o.chain_cost = (b.ptr for b in outs)
    o.keep_stride = Q
    timed("shortcut", lambda: m._abi.check(env._ctx, m._abi.lib().mplx_shortcut_device(pairs._h, short._h, C.byref(i), C.byref(o))))
    env.synchronize()
    res["shortcut_Q"], res["shortcut_pairs"] = Q, P
    res["shortcut_kept_mean"] = float(outs[1].download(np.int32, (Q,)).mean())
    res["shortcut_status_ok"] = int((outs[0].download(np.uint8, (Q,)) == 0).sum())
    for b in outs + [d_st]:
        b.free()
    pairs.free()
    short.free()
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    for p in (poly, loaded):
        p.free()
    for b in (d_wp, d_v, d_seg, d_dts):
        b.free()
    lim.free()
    env.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
