"""Generates tests/golden/scale_golden.npz from the REFERENCE's own Lambda (lambda.h) and Trajectory::scale / evaluate /
sample (trajectory.h).  The small C++ driver below is compiled into a temporary directory against the reference's
headers, where they lie, and the stand-in Eigen of oracle/stub_include (flags of oracle/Makefile); nothing but the .npz
is kept.  Run in the build container:

    python tests/golden/make_scale_golden.py            # writes the fixture
    python tests/golden/make_scale_golden.py --time     # one-thread time of the reference on the workload of
                                                        # profiles/micro/scale_times.py (JSON)

REF (environment) names the reference tree, as in oracle/Makefile.

Inputs: tests/scale_model.py is not needed; the cases are made here and stored with the results -- per case (D in {2, 3},
S in {1, 3, 5}) a dozen trajectories loaded as Primitive(cs, t, control) from binary-fraction coefficients and durations,
scale(ri, rf) with ratios from [0.25, 4]; trajectory 0 of every case has ri == rf (the linear branch of solve), trajectory
1 of every S = 5 case lasts 64 s or more (the 1e-5 clamp of LambdaSeg fires).  Recorded per trajectory: LambdaSeg::a and
dT, Ts, the total, getTau (and whether it found a root: it returns -1 otherwise) at QUERY interior times total (i + 1/2)
/ 8 and at the end points 0, total and 9 * (total / 9), the Commands of sample(9) and the Waypoints at the same times.
Everything as bit patterns (uint64)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("REF", "/root/reference")

N_TRAJ, N_SAMPLE, N_INTERIOR = 12, 9, 8
N_QUERY = N_INTERIOR + 3
RATIOS = [0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0]
JRK = 0x07

DRIVER = r"""
// argv: in out [reps].  in (doubles): D K S N, then per trajectory: ri rf, dts [S], coefficients [S][D + 1][6].
// out (doubles), per trajectory: a[4] dT Ts[S + 1] total, then {getTau, found} at the N_INTERIOR interior times and at 0,
// total, N * (total / N), then the Commands of sample(N) [(N + 1)][4D + 3] and the Waypoints at the same times
// [(N + 1)][4D + 1].  With reps: per pass the seconds of scale + sample(N) over all trajectories.
#include <mpl_basis/trajectory.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
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
int run(const std::vector<double> &in, const char *out_path, int reps) {
  const int K = (int)in[1], S = (int)in[2], N = (int)in[3];
  const double *p = in.data() + 4;
  std::vector<Trajectory<D>> trajs;
  std::vector<double> ri(K), rf(K);
  for (int k = 0; k < K; k++) {
    ri[k] = p[0];
    rf[k] = p[1];
    const double *dts = p + 2, *cs = p + 2 + S;
    vec_E<Primitive<D>> prs;
    for (int s = 0; s < S; s++) {
      vec_E<Vec6f> c(D + 1);
      for (int a = 0; a <= D; a++)
        for (int j = 0; j < 6; j++) c[a](j) = cs[(s * (D + 1) + a) * 6 + j];
      prs.push_back(Primitive<D>(c, dts[s], Control::JRKxYAW));
    }
    trajs.push_back(Trajectory<D>(prs));
    p += 2 + S + S * (D + 1) * 6;
  }
  FILE *out = std::fopen(out_path, "wb");
  if (!out) return 4;
  auto put = [&](double v) { std::fwrite(&v, sizeof v, 1, out); };
  if (reps > 0) {
    for (int r = 0; r < reps; r++) {
      double acc = 0;
      auto t0 = std::chrono::steady_clock::now();
      for (int k = 0; k < K; k++) {
        Trajectory<D> tr = trajs[k];
        tr.scale(ri[k], rf[k]);
        acc += tr.sample(N).back().pos(0);
      }
      put(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
      put(acc);
    }
    std::fclose(out);
    return 0;
  }
  for (int k = 0; k < K; k++) {
    Trajectory<D> &tr = trajs[k];
    tr.scale(ri[k], rf[k]);
    const Lambda l = tr.lambda();
    for (int i = 0; i < 4; i++) put(l.segs[0].a(i));
    put(l.segs[0].dT);
    for (int s = 0; s <= S; s++) put(tr.Ts[s]);
    const double total = tr.getTotalTime();
    put(total);
    std::vector<double> q;
    for (int i = 0; i < 8; i++) q.push_back(total * (i + 0.5) / 8);
    q.push_back(0.0);
    q.push_back(total);
    q.push_back(N * (total / N));
    for (double t : q) {
      const double tau = l.getTau(t);
      put(tau);
      put(tau == -1 ? 0.0 : 1.0);
    }
    const auto cmds = tr.sample(N);
    for (const auto &c : cmds) {
      for (int i = 0; i < D; i++) put(c.pos(i));
      for (int i = 0; i < D; i++) put(c.vel(i));
      for (int i = 0; i < D; i++) put(c.acc(i));
      for (int i = 0; i < D; i++) put(c.jrk(i));
      put(c.yaw);
      put(c.yaw_dot);
      put(c.t);
    }
    const double step = total / N;
    for (int i = 0; i <= N; i++) {
      const Waypoint<D> w = tr.evaluate(i * step);
      for (int j = 0; j < D; j++) put(w.pos(j));
      for (int j = 0; j < D; j++) put(w.vel(j));
      for (int j = 0; j < D; j++) put(w.acc(j));
      for (int j = 0; j < D; j++) put(w.jrk(j));
      put(w.yaw);
    }
  }
  std::fclose(out);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  const std::vector<double> in = slurp(argv[1]);
  const int reps = argc > 3 ? std::atoi(argv[3]) : 0;
  return (int)in[0] == 2 ? run<2>(in, argv[2], reps) : run<3>(in, argv[2], reps);
}
"""


def build_driver(tmp):
    src = os.path.join(tmp, "scale_driver.cpp")
    exe = os.path.join(tmp, "scale_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused", "-Wno-sign-compare",
                    "-I", os.path.join(ROOT, "oracle", "stub_include"), "-I", os.path.join(REF, "include"), "-o", exe, src],
                   check=True)
    return exe


def make_case(D, S, seed):
    """coeff [K][S][D + 1][6] (sixteenths in +-2; of the yaw primitive c(4), c(5) only), dts [K][S] (quarters in [0.5, 3]),
    ri, rf [K]."""
    rng = np.random.default_rng(seed)
    K = N_TRAJ
    coeff = rng.integers(-32, 33, (K, S, D + 1, 6)).astype(np.float64) / 16.0
    coeff[:, :, D, :4] = 0.0
    dts = rng.integers(2, 13, (K, S)).astype(np.float64) / 4.0
    ri, rf = rng.choice(RATIOS, K), rng.choice(RATIOS, K)
    same = ri == rf
    rf[same] = np.where(ri[same] == 4.0, 0.25, 4.0)  # only trajectory 0 has ri == rf
    rf[0] = ri[0]
    if S == 5:  # a long one: 2 |1/rf - 1/ri| / T^3 < 1e-5 / 2
        dts[1] = [16.0, 12.0, 16.0, 8.0, 12.0 + 4.0 * (D - 2)]
        coeff[1] /= 64.0  # (so the positions stay moderate over 64 s)
        ri[1], rf[1] = 1.0, 2.0
    return coeff, dts, ri, rf


def run_case(exe, tmp, D, S, coeff, dts, ri, rf, reps=0, n_sample=N_SAMPLE):
    K = coeff.shape[0]
    ipath, opath = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    blob = [np.asarray([D, K, S, n_sample], np.float64)]
    for k in range(K):
        blob += [np.asarray([ri[k], rf[k]]), dts[k].ravel(), coeff[k].ravel()]
    np.concatenate(blob).tofile(ipath)
    subprocess.run([exe, ipath, opath] + ([str(reps)] if reps else []), check=True, stdout=subprocess.DEVNULL)
    raw = np.fromfile(opath, dtype=np.float64)
    if reps:
        return raw.reshape(-1, 2)
    rc, rw, N = 4 * D + 3, 4 * D + 1, n_sample
    per = 4 + 1 + (S + 1) + 1 + 2 * N_QUERY + (N + 1) * (rc + rw)
    raw = raw.reshape(K, per)
    at = 0
    out = {}
    for key, n in (("a", 4), ("dT", 1), ("Ts", S + 1), ("total", 1), ("tau", 2 * N_QUERY), ("cmd", (N + 1) * rc), ("way", (N + 1) * rw)):
        out[key] = raw[:, at:at + n]
        at += n
    q = out.pop("tau").reshape(K, N_QUERY, 2)
    out["tau"], out["found"] = np.ascontiguousarray(q[:, :, 0]), np.ascontiguousarray(q[:, :, 1])
    out["cmd"], out["way"] = out["cmd"].reshape(K, N + 1, rc), out["way"].reshape(K, N + 1, rw)
    return out


def time_reference(exe, tmp):
    """One host thread of the reference: scale + sample(N) over the trajectories of profiles/micro/scale_times.py."""
    sys.path.insert(0, os.path.join(ROOT, "profiles", "micro"))
    import scale_times as ST
    coeff, dts, ri, rf = ST.workload(4096)  # a sixteenth of the device's set: the reference is linear in it
    t = run_case(exe, tmp, 3, coeff.shape[1], coeff, dts, ri, rf, reps=3, n_sample=ST.SAMPLE_N)
    print(json.dumps({"reference_cpu_scale_sample": {"trajectories": 4096, "samples": ST.SAMPLE_N + 1,
                                                     "scale_and_sample_s": float(np.median(t[:, 0]))}, "threads": 1}, indent=1))


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        if "--time" in sys.argv:
            return time_reference(exe, tmp)
        for D in (2, 3):
            for S in (1, 3, 5):
                coeff, dts, ri, rf = make_case(D, S, 1000 + 10 * D + S)
                res = run_case(exe, tmp, D, S, coeff, dts, ri, rf)
                name = "d%d_s%d" % (D, S)
                for key, arr in (("coeff", coeff), ("dts", dts), ("ri", ri), ("rf", rf)):
                    out[name + "/" + key] = np.ascontiguousarray(arr).view(np.uint64)
                for key, arr in res.items():
                    out[name + "/" + key] = np.ascontiguousarray(arr).view(np.uint64)
    path = os.path.join(ROOT, "tests", "golden", "scale_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
