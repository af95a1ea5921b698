"""Generates tests/golden/heur_golden.npz from the REFERENCE's own env_base<Dim>::cal_heur with heur_ignore_dynamics_ ==
false (env_base.h:56-211) and from its MapPlanner<2> with setHeurIgnoreDynamics(false).  The two small C++ drivers below
are compiled into a temporary directory against the reference's headers, where they lie, and the stand-in Eigen / Boost
of oracle/stub_include (flags of oracle/Makefile; the planner as oracle/ref_planner_shim.cpp's recipe compiles it);
nothing but the .npz is kept.  Run in the build container:

    python tests/golden/make_heur_golden.py

REF (environment) names the reference tree, as in oracle/Makefile.

Recorded, as bit patterns (uint64): per case "d<D>_<state control>_<goal control>" the settings (w, v_max), the goal row,
N_STATES lattice state columns (positions and velocities on a 0.25 grid; some with dp = 0) and cal_heur of each.  Cases:
VEL-VEL, ACC-ACC, ACC-VEL and the else branch (an ACCxYAW state, an SNP state) for D = 2 and 3, under w = 10, v_max = 3
and w = 1, v_max = 2.  "no_root/<case>": the states of the case for which the reference's quartic returned nothing.
"plan/...": cost, expanded states and trajectory duration of the reference's MapPlanner<2> on tests/golden/corridor_map.npz
with the settings of test_planner_2d and setHeurIgnoreDynamics(false)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("REF", "/root/reference")
N_STATES = 200
VEL, ACC, JRK, SNP, ACCxYAW = 0x01, 0x03, 0x07, 0x0f, 0x13
CASES = [(VEL, VEL), (ACC, ACC), (ACC, VEL), (ACCxYAW, ACCxYAW), (SNP, SNP)]
SETTINGS = [(10.0, 3.0), (1.0, 2.0)]

HEUR_DRIVER = r"""
// argv: in out.  in (doubles): D control goal_control w v_max K, the goal's 4D+1 rows, K states of 4D+1 rows each.
// out: per state cal_heur and the number of roots quartic returned for the ACC branches (-1 elsewhere).
#include <mpl_planner/common/env_base.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

template <int D>
static Waypoint<D> load(const double *r, int control) {
  Waypoint<D> w((Control::Control)control);
  for (int i = 0; i < D; i++) { w.pos(i) = r[i]; w.vel(i) = r[D + i]; w.acc(i) = r[2 * D + i]; w.jrk(i) = r[3 * D + i]; }
  w.yaw = r[4 * D];
  return w;
}

template <int D>
static void run(const std::vector<double> &in, std::vector<double> &out) {
  const int control = (int)in[1], goal_control = (int)in[2], F = 4 * D + 1;
  const size_t K = (size_t)in[5];
  MPL::env_base<D> env;
  env.set_w(in[3]);
  env.set_v_max(in[4]);
  env.set_heur_ignore_dynamics(false);
  const double *g = in.data() + 6, *s = g + F;
  const Waypoint<D> goal = load<D>(g, goal_control);
  for (size_t k = 0; k < K; k++, s += F) {
    const Waypoint<D> st = load<D>(s, control);
    out.push_back(env.cal_heur(st, goal));
    double roots = -1;
    if (control == Control::ACC && (goal_control == Control::ACC || goal_control == Control::VEL)) {
      const Vecf<D> dp = goal.pos - st.pos;
      const bool aa = goal_control == Control::ACC;
      const decimal_t c1 = aa ? -36 * dp.dot(dp) : -9 * dp.dot(dp);
      const decimal_t c2 = aa ? 24 * (st.vel + goal.vel).dot(dp) : 12 * st.vel.dot(dp);
      const decimal_t c3 = aa ? -4 * (st.vel.dot(st.vel) + st.vel.dot(goal.vel) + goal.vel.dot(goal.vel)) : -3 * st.vel.dot(st.vel);
      roots = (double)quartic(in[3], 0, c3, c2, c1).size();
    }
    out.push_back(roots);
  }
}

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  std::vector<double> in, out;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  in.resize((size_t)std::ftell(f) / sizeof(double));
  std::fseek(f, 0, SEEK_SET);
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  if ((int)in[0] == 2) run<2>(in, out); else run<3>(in, out);
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
  std::fclose(f);
  return 0;
}
"""

PLAN_DRIVER = r"""
// argv: in out.  in (doubles): dim0 dim1 origin0 origin1 res start0 start1 goal0 goal1, then dim0 * dim1 cells.
// out: ok, cost, expanded states, trajectory duration, segments.  test_planner_2d.cpp's settings, the dynamics on.
#include <mpl_planner/planner/map_planner.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "REFSRC/src/mpl_planner/map_planner.cpp"

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  std::vector<double> in;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  in.resize((size_t)std::ftell(f) / sizeof(double));
  std::fseek(f, 0, SEEK_SET);
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  Veci<2> dim((int)in[0], (int)in[1]);
  Vecf<2> ori(in[2], in[3]);
  const size_t n = (size_t)dim(0) * (size_t)dim(1);
  MPL::Tmap cells(n);
  for (size_t i = 0; i < n; i++) cells[i] = (int8_t)in[9 + i];
  std::shared_ptr<MPL::OccMapUtil> mu = std::make_shared<MPL::OccMapUtil>();
  mu->setMap(ori, dim, cells, in[4]);
  MPL::OccMapPlanner planner(false);
  planner.setMapUtil(mu);
  planner.setVmax(1.0);
  planner.setAmax(1.0);
  planner.setDt(1.0);
  vec_E<VecDf> U;
  const decimal_t du = 0.5;
  for (decimal_t dx = -0.5; dx <= 0.5; dx += du)
    for (decimal_t dy = -0.5; dy <= 0.5; dy += du) U.push_back(Vec2f(dx, dy));
  planner.setU(U);
  planner.setHeurIgnoreDynamics(false);
  Waypoint2D start, goal;
  start.pos = Vec2f(in[5], in[6]);
  start.vel = Vec2f::Zero(); start.acc = Vec2f::Zero(); start.jrk = Vec2f::Zero(); start.yaw = 0;
  start.use_pos = true; start.use_vel = true; start.use_acc = false; start.use_jrk = false; start.use_yaw = false;
  goal = start;
  goal.pos = Vec2f(in[7], in[8]);
  const bool ok = planner.plan(start, goal);
  const auto traj = planner.getTraj();
  const double out[5] = {ok ? 1.0 : 0.0, planner.getTrajCost(), (double)planner.getExpandedNum(), traj.getTotalTime(),
                         (double)traj.getPrimitives().size()};
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out, sizeof(double), 5, f) != 5) return 4;
  std::fclose(f);
  return 0;
}
"""

FLAGS = ["-O2", "-std=c++14", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused", "-Wno-sign-compare"]


def build(tmp, name, text):
    src, exe = os.path.join(tmp, name + ".cpp"), os.path.join(tmp, name)
    with open(src, "w") as f:
        f.write(text.replace("REFSRC", REF))
    subprocess.run(["g++"] + FLAGS + ["-I", os.path.join(ROOT, "oracle", "stub_include"), "-I", os.path.join(REF, "include"), "-o", exe, src],
                   check=True)
    return exe


def make_states(D, control, seed):
    """[4D+1][N_STATES] lattice columns: positions in +-6, velocities up to 3 (0.25 grid), accelerations / jerks / yaw where
    the flag has them; every tenth column at the goal's position (dp = 0), column 0 the goal itself."""
    rng = np.random.default_rng(seed)
    q = lambda lim: rng.integers(-int(lim * 4), int(lim * 4) + 1, (D, N_STATES)).astype(np.float64) / 4.0
    s = np.zeros((4 * D + 1, N_STATES))
    s[:D] = q(6.0)
    base = control & 0x0f
    if base >= ACC:
        s[D:2 * D] = q(3.0)
    if base >= JRK:
        s[2 * D:3 * D] = q(2.0)
    if base >= SNP:
        s[3 * D:4 * D] = q(1.0)
    if control & 0x10:
        s[4 * D] = rng.integers(-6, 7, N_STATES) * 0.25
    s[:D, ::10] = 0.0
    s[:, 0] = 0.0
    return s


def goal_row(D, goal_control):
    g = np.zeros(4 * D + 1)
    if (goal_control & 0x0f) >= ACC:
        g[D:2 * D] = [0.5, -0.25, 0.25][:D]
    return g


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, "heur_driver", HEUR_DRIVER)
        ipath, opath = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        for D in (2, 3):
            for ci, (cs, cg) in enumerate(CASES):
                for si, (w, v_max) in enumerate(SETTINGS):
                    s, g = make_states(D, cs, 1000 * D + 10 * ci + si), goal_row(D, cg)
                    np.concatenate([[D, cs, cg, w, v_max, N_STATES], g, s.T.ravel()]).astype(np.float64).tofile(ipath)
                    subprocess.run([exe, ipath, opath], check=True)
                    r = np.fromfile(opath, dtype=np.float64).reshape(N_STATES, 2)
                    name = "d%d_%02x_%02x_%d" % (D, cs, cg, si)
                    out[name + "/setting"] = np.array([w, v_max]).view(np.uint64)
                    out[name + "/goal"] = g.view(np.uint64)
                    out[name + "/states"] = np.ascontiguousarray(s).view(np.uint64)
                    out[name + "/h"] = np.ascontiguousarray(r[:, 0]).view(np.uint64)
                    out[name + "/n_roots"] = r[:, 1].astype(np.int32)
                    print(name, "no root:", int((r[:, 1] == 0).sum()), "DBL_MAX:", int((r[:, 0] > 1e300).sum()))
        z = np.load(os.path.join(ROOT, "tests", "golden", "corridor_map.npz"))
        n = int(z["n_cells"])
        cells = np.where(np.unpackbits(z["occupied_bits"])[:n].astype(bool), 100.0, 0.0)
        exe = build(tmp, "plan_driver", PLAN_DRIVER)
        head = [float(z["dim"][0]), float(z["dim"][1]), float(z["origin"][0]), float(z["origin"][1]), float(z["resolution"]),
                float(z["start"][0]), float(z["start"][1]), float(z["goal"][0]), float(z["goal"][1])]
        np.concatenate([head, cells]).astype(np.float64).tofile(ipath)
        subprocess.run([exe, ipath, opath], check=True, stdout=subprocess.DEVNULL)
        ok, cost, expanded, duration, segments = np.fromfile(opath, dtype=np.float64)
        print("plan: ok %d cost %r expanded %d duration %r segments %d" % (ok, cost, expanded, duration, segments))
        out["plan/ok"] = np.array([int(ok)], np.int32)
        out["plan/cost"] = np.array([cost]).view(np.uint64)
        out["plan/expanded"] = np.array([int(expanded)], np.int64)
        out["plan/duration"] = np.array([duration]).view(np.uint64)
        out["plan/segments"] = np.array([int(segments)], np.int32)
    path = os.path.join(ROOT, "tests", "golden", "heur_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
