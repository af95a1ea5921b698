"""Generates tests/golden/traj_golden.npz from the REFERENCE's own Trajectory<Dim> (trajectory.h) and
env_map<Dim>::traverse_trajectory (env_map.h:229-255).  The small C++ driver below is compiled into a temporary
directory against the reference's headers, where they lie, and the stand-in Eigen of oracle/stub_include (flags of
oracle/Makefile); nothing but the .npz is kept.  Run in the build container:

    python tests/golden/make_traj_golden.py            # writes the fixture
    python tests/golden/make_traj_golden.py --time     # one-thread time of the reference on the workload of
                                                       # profiles/micro/traj_times.py (JSON)

REF (environment) names the reference tree, as in oracle/Makefile.

Inputs: tests/traj_model.py fixture_cases() / fixture_queries().  Per case and trajectory the fixture holds S, T, the
five efforts, the Command and Waypoint rows of sample(UNIFORM_N) and of the query times, and per map mode (occupancy,
potential with gradient weight 0 and 0.25) traverse_trajectory's cost and n + 1.  A trajectory without segments is not
evaluated (the reference divides 0 by 0 there); the model defines its rows."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("REF", "/root/reference")

DRIVER = r"""
// argv: in map pot out [reps].  in (doubles): dim control dt v_max pot_w nU udim K H Q N d0 d1 d2 o0 o1 o2 res, then U
// [nU][udim], starts [K][4D+2], actions [K][H], queries [K][Q], gradient weights [3] (mode 0: no potential map).  map, pot:
// one int8 per cell (pot "-": all zero).  out (doubles), per trajectory: S T J[4] Jyaw, and for S > 0: Command rows
// of sample(N) [(N+1)][4D+3], Waypoint rows [(N+1)][4D+1], the same two for the Q query times, then per mode
// {traverse cost, n + 1}.  With reps: per pass {seconds of sample(N), seconds of traverse_trajectory} over all
// trajectories.
#include <mpl_basis/trajectory.h>
#include <mpl_collision/map_util.h>
#include <mpl_planner/env/env_map.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

static std::vector<double> slurp(const char *path) {
  std::vector<double> v;
  FILE *f = std::fopen(path, "rb");
  if (!f) std::exit(2);
  std::fseek(f, 0, SEEK_END);
  v.resize((size_t)std::ftell(f) / sizeof(double));
  std::fseek(f, 0, SEEK_SET);
  if (std::fread(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(3);
  std::fclose(f);
  return v;
}

template <int D>
int run(const std::vector<double> &in, const char *map_path, const char *pot_path, const char *out_path, int reps) {
  const double *h = in.data();
  const Control::Control control = (Control::Control)(int)h[1];
  const double dt = h[2], v_max = h[3], pot_w = h[4], res = h[17];
  const int nU = (int)h[5], udim = (int)h[6], K = (int)h[7], H = (int)h[8], Q = (int)h[9], N = (int)h[10];
  Veci<D> dim;
  Vecf<D> ori;
  size_t cells = 1;
  for (int i = 0; i < D; i++) {
    dim(i) = (int)h[11 + i];
    ori(i) = h[14 + i];
    cells *= (size_t)dim(i);
  }
  const double *p = h + 18;
  vec_E<VecDf> U;
  for (int a = 0; a < nU; a++) {
    VecDf u(udim);
    for (int i = 0; i < udim; i++) u(i) = p[a * udim + i];
    U.push_back(u);
  }
  p += nU * udim;
  const double *starts = p;
  p += K * (4 * D + 2);
  const double *actions = p;
  p += K * H;
  const double *queries = p;
  p += K * Q;
  const double *grad_w = p;
  p += 3;
  MPL::Tmap map(cells);
  std::vector<int8_t> pot(cells, 0);
  FILE *f = std::fopen(map_path, "rb");
  if (!f || std::fread(map.data(), 1, cells, f) != cells) return 6;
  std::fclose(f);
  if (pot_path[0] != '-') {
    f = std::fopen(pot_path, "rb");
    if (!f || std::fread(pot.data(), 1, cells, f) != cells) return 7;
    std::fclose(f);
  }
  auto mu = std::make_shared<MPL::MapUtil<D>>();
  mu->setMap(ori, dim, map, res);

  std::vector<Trajectory<D>> trajs;
  for (int k = 0; k < K; k++) {
    Waypoint<D> s(control);
    const double *r = starts + k * (4 * D + 2);
    for (int i = 0; i < D; i++) {
      s.pos(i) = r[i];
      s.vel(i) = r[D + i];
      s.acc(i) = r[2 * D + i];
      s.jrk(i) = r[3 * D + i];
    }
    s.yaw = r[4 * D];
    s.t = r[4 * D + 1];
    vec_E<Primitive<D>> prs;
    for (int hh = 0; hh < H; hh++) {
      const int a = (int)actions[k * H + hh];
      if (a < 0) break;
      Primitive<D> pr(s, U[a], dt);  // env_map.h:156-161
      Waypoint<D> tn = pr.evaluate(dt);
      tn.t = s.t + dt;
      prs.push_back(pr);
      s = tn;
    }
    trajs.push_back(Trajectory<D>(prs));
  }

  FILE *out = std::fopen(out_path, "wb");
  if (!out) return 4;
  auto put = [&](double v) { std::fwrite(&v, sizeof v, 1, out); };
  MPL::env_map<D> env(mu);
  env.set_v_max(v_max);
  env.set_dt(dt);
  env.set_potential_weight(pot_w);
  if (reps > 0) {
    for (int r = 0; r < reps; r++) {
      double acc = 0;
      auto t0 = std::chrono::steady_clock::now();
      for (const auto &tr : trajs) acc += tr.sample(N).back().pos(0);
      const double s1 = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      t0 = std::chrono::steady_clock::now();
      for (const auto &tr : trajs) acc += tr.segs.empty() ? 0 : env.traverse_trajectory(tr);
      const double s2 = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      put(s1);
      put(s2);
      put(acc);
    }
    std::fclose(out);
    return 0;
  }
  for (int k = 0; k < K; k++) {
    const Trajectory<D> &tr = trajs[k];
    put((double)tr.segs.size());
    put(tr.getTotalTime());
    put(tr.J(Control::VEL));
    put(tr.J(Control::ACC));
    put(tr.J(Control::JRK));
    put(tr.J(Control::SNP));
    put(tr.Jyaw());
    if (tr.segs.empty()) continue;
    auto put_command = [&](const Command<D> &c) {
      for (int i = 0; i < D; i++) put(c.pos(i));
      for (int i = 0; i < D; i++) put(c.vel(i));
      for (int i = 0; i < D; i++) put(c.acc(i));
      for (int i = 0; i < D; i++) put(c.jrk(i));
      put(c.yaw);
      put(c.yaw_dot);
      put(c.t);
    };
    auto put_waypoint = [&](const Waypoint<D> &w) {
      for (int i = 0; i < D; i++) put(w.pos(i));
      for (int i = 0; i < D; i++) put(w.vel(i));
      for (int i = 0; i < D; i++) put(w.acc(i));
      for (int i = 0; i < D; i++) put(w.jrk(i));
      put(w.yaw);
    };
    const auto cmds = tr.sample(N);
    for (const auto &c : cmds) put_command(c);
    const double step = tr.getTotalTime() / N;
    for (int i = 0; i <= N; i++) put_waypoint(tr.evaluate(i * step));
    for (int q = 0; q < Q; q++) {
      Command<D> c;
      if (!tr.evaluate(queries[k * Q + q], c)) return 5;
      put_command(c);
    }
    for (int q = 0; q < Q; q++) put_waypoint(tr.evaluate(queries[k * Q + q]));
    for (int mode = 0; mode < 3; mode++) {
      env.set_potential_map(mode == 0 ? std::vector<int8_t>() : pot);
      env.set_gradient_weight(grad_w[mode]);
      put(env.traverse_trajectory(tr));
      put((double)((int)std::ceil(v_max * tr.getTotalTime() / res) + 1));
    }
  }
  std::fclose(out);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 5) return 1;
  const std::vector<double> in = slurp(argv[1]);
  const int reps = argc > 5 ? std::atoi(argv[5]) : 0;
  return (int)in[0] == 2 ? run<2>(in, argv[2], argv[3], argv[4], reps) : run<3>(in, argv[2], argv[3], argv[4], reps);
}
"""


def build_driver(tmp):
    src = os.path.join(tmp, "traj_driver.cpp")
    exe = os.path.join(tmp, "traj_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused", "-Wno-sign-compare",
                    "-I", os.path.join(ROOT, "oracle", "stub_include"), "-I", os.path.join(REF, "include"), "-o", exe, src],
                   check=True)
    return exe


def write_input(path, case, queries, n_uniform, grad_ws, pot_w):
    md, org, res = case["geo"]
    dim = case["dim"]
    U, starts, actions = case["U"], case["starts"], case["actions"]
    K = actions.shape[1]
    if starts.shape[1] == 1:
        starts = np.repeat(starts, K, axis=1)
    head = [dim, case["control"], case["dt"], case["v_max"], pot_w, U.shape[0], U.shape[1], K, actions.shape[0], queries.shape[1],
            n_uniform] + list(md) + [1] * (3 - dim) + list(org) + [0.0] * (3 - dim) + [res]
    blob = np.concatenate([np.asarray(head, np.float64), U.ravel(), starts.T.ravel(), actions.T.astype(np.float64).ravel(),
                           queries.ravel(), np.asarray(grad_ws, np.float64)])
    blob.tofile(path)
    np.ascontiguousarray(case["grid"], dtype=np.int8).tofile(path + ".map")
    if case["pot"] is not None:
        np.ascontiguousarray(case["pot"], dtype=np.int8).tofile(path + ".pot")
    return [path, path + ".map", path + ".pot" if case["pot"] is not None else "-"]


def run_case(exe, tmp, case, queries, n_uniform, grad_ws, pot_w):
    ipath, opath = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    subprocess.run([exe] + write_input(ipath, case, queries, n_uniform, grad_ws, pot_w) + [opath], check=True, stdout=subprocess.DEVNULL)
    raw = np.fromfile(opath, dtype=np.float64)
    D, K, Q, N = case["dim"], case["actions"].shape[1], queries.shape[1], n_uniform
    rc, rw = 4 * D + 3, 4 * D + 1
    head = np.zeros((K, 7))
    cmd_u, way_u = np.zeros((K, N + 1, rc)), np.zeros((K, N + 1, rw))
    cmd_q, way_q = np.zeros((K, Q, rc)), np.zeros((K, Q, rw))
    trav = np.zeros((K, 3, 2))
    at = 0
    for k in range(K):
        head[k] = raw[at:at + 7]
        at += 7
        if head[k, 0] == 0:
            continue
        for arr in (cmd_u, way_u, cmd_q, way_q, trav):
            n = arr[k].size
            arr[k] = raw[at:at + n].reshape(arr[k].shape)
            at += n
    assert at == raw.size
    return head, cmd_u, way_u, cmd_q, way_q, trav


def time_reference(exe, tmp):
    """One host thread of the reference over the trajectories of profiles/micro/traj_times.py on C4's 512^3 map."""
    sys.path.insert(0, os.path.join(ROOT, "profiles", "micro"))
    import traj_times as TT
    rep = {}
    for kind in ("short", "long"):
        case = TT.workload(kind, 4096)  # a sixteenth of the device's set: the reference is linear in it
        ipath, opath = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        args = write_input(ipath, case, np.zeros((case["actions"].shape[1], 1)), TT.SAMPLE_N, [0.0, 0.0, 0.0], 0.1)
        subprocess.run([exe] + args + [opath, "3"], check=True, stdout=subprocess.DEVNULL)
        t = np.fromfile(opath, dtype=np.float64).reshape(-1, 3)
        rep[kind] = {"trajectories": 4096, "v_max": case["v_max"], "sample_s": float(np.median(t[:, 0])),
                     "traverse_s": float(np.median(t[:, 1]))}
    print(json.dumps({"reference_cpu_traj_512": rep, "threads": 1}, indent=1))


def main():
    import traj_model as M

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        if "--time" in sys.argv:
            return time_reference(exe, tmp)
        for case in M.fixture_cases():
            trajs = M.case_trajs(case)
            queries = M.fixture_queries(case, trajs)
            head, cmd_u, way_u, cmd_q, way_q, trav = run_case(exe, tmp, case, queries, M.UNIFORM_N, [m[2] for m in M.MODES], M.POT_W)
            name = case["name"]
            for key, arr in (("head", head), ("cmd_u", cmd_u), ("way_u", way_u), ("cmd_q", cmd_q), ("way_q", way_q), ("trav", trav)):
                out[name + "/" + key] = arr.view(np.uint64)
    path = os.path.join(ROOT, "tests", "golden", "traj_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
