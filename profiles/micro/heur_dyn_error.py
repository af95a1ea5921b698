"""The error of the ROBUST dynamics-aware heuristic (include/mplx_heur.h) against the exact minimum, on the CPU: per
branch 50 000 random lattice states (tests/heur_model.py::sweep_states, D = 2 and 3, the settings SWEEP_SETTINGS), the
exact minimum by mpmath at 60 digits, the worst |h - h*| in units of 2^-52 * sum |terms of C at the minimiser|; and the
redone probe of the reference's misses: the share of states where REFERENCE is above the true minimum, and the largest
factor.  Writes profiles/heur_dyn_error.json.

    python profiles/micro/heur_dyn_error.py [states per branch] [processes]"""
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import heur_model as HM  # noqa: E402

CHUNK = 250


def work(job):
    bi, D, si, seed = job
    branch, (w, v_max) = HM.BRANCHES[bi], HM.SWEEP_SETTINGS[si]
    s, goal = HM.sweep_states(branch, D, CHUNK, seed)
    rows = HM.sweep_units(branch, D, s, goal, w, v_max)
    ref_above, ref_factor, ref_none = 0, 1.0, 0
    if branch in ((HM.ACC, HM.ACC), (HM.ACC, HM.VEL)) and v_max > 0:
        for k, (u, npos, where, h, hs, scale) in enumerate(rows):
            r = HM.reference(s[:, k], goal, branch[0], branch[1], w, v_max, D)
            if r > 1e300:
                ref_none += 1
            elif hs > 0 and r > hs * (1 + 1e-9):
                ref_above += 1
                ref_factor = max(ref_factor, r / hs)
    return (bi, max(u for u, *_ in rows), sum(1 for r in rows if r[1] >= 3), sum(1 for r in rows if r[2] == "bar"),
            sum(1 for r in rows if r[2] == "interior"), sum(1 for r in rows if r[2] is None), ref_above, ref_factor, ref_none)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    procs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    jobs = []
    for bi in range(len(HM.BRANCHES)):
        for c in range(n // CHUNK):
            jobs.append((bi, 2 + c % 2, (c // 2) % len(HM.SWEEP_SETTINGS), 7919 * bi + c))
    out = {}
    with multiprocessing.Pool(procs) as pool:
        for bi, worst, n3, bar, interior, none, ra, rf, rn in pool.imap_unordered(work, jobs, chunksize=4):
            name = "%02x-%02x" % HM.BRANCHES[bi]
            o = out.setdefault(name, {"states": 0, "worst_units": 0.0, "three_stationary_points": 0, "minimum_at_t_bar": 0,
                                      "interior_minimum": 0, "no_candidate": 0, "reference_above_true_minimum": 0,
                                      "reference_largest_factor": 1.0, "reference_no_candidate": 0})
            o["states"] += CHUNK
            o["worst_units"] = max(o["worst_units"], worst)
            o["three_stationary_points"] += n3
            o["minimum_at_t_bar"] += bar
            o["interior_minimum"] += interior
            o["no_candidate"] += none
            o["reference_above_true_minimum"] += ra
            o["reference_largest_factor"] = max(o["reference_largest_factor"], rf)
            o["reference_no_candidate"] += rn
    res = {"unit": "2^-52 * sum |terms of C at the minimiser|", "bisect": HM.BISECT, "settings_w_vmax": HM.SWEEP_SETTINGS,
           "worst_units": max(o["worst_units"] for o in out.values()), "branches": out}
    path = os.path.join(ROOT, "profiles", "heur_dyn_error.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
