// scale_kernel.hip -- time scaling of the set an mplx_poly holds, for gfx950 (MI355X): Lambda(vs), Trajectory::scale,
// the restated scale_down and Lambda::getTau (include/mplx_scale.h; reference include/mpl_basis/lambda.h,
// include/mpl_basis/trajectory.h:140-225, include/mpl_basis/math.h:69-131).
//
// lambda_build_kernel: one lane per problem.  Up to 9 virtual points -> up to 8 segments (mplx_scale_math.h build_seg)
// into the poly's Lambda table, then Ts[s] = Lambda::getT(taus[s]) and the total.  A problem with a status gets no
// Lambda and writes its status only; the outputs of a good one are copied from the table in a second pass, so a failure
// in a late segment leaves the caller's bytes alone.
// lambda_scale_points_kernel / lambda_down_*: fill the scratch points the build then reads.  scale_down: one lane per
// (problem, segment), problem-minor, records max_l / t_lo / t_hi of the segment; then one lane per problem walks its
// segments in order -- two launches instead of atomics, every value written once from inputs only.
// lambda_tau_kernel: one lane per (problem, time), the time index minor: a wave mostly shares one Lambda segment and one
// branch of cubic.
//
// Register audit (-Rpass-analysis=kernel-resource-usage) in DESIGN.md 4.17.
//
// Bit-exactness: -ffp-contract=off; the arithmetic is mplx_scale_math.h.  cbrt, acos and cos are the device library's.
#include "mplx_internal.h"
#include "mplx_scale_math.h"

namespace mplx {
namespace {

constexpr int kBlock = 256;
constexpr int kProbBlock = 64;  // one wave: K problems spread over as many CUs as K / 64 allows (as poly_load_kernel)

using scale::TableLoader;

__global__ __launch_bounds__(kProbBlock) void lambda_build_kernel(const ScaleArgs P) {
  const int64_t n = P.n_prob;
  const int64_t k = (int64_t)blockIdx.x * kProbBlock + threadIdx.x;
  if (k >= n) return;
  const int S = P.tab_S[k];
  if (S == 0 || (P.only && !P.only[k])) {  // a failed problem of the solve or load, or one scale_down left alone
    P.lam_n[k] = 0;
    P.lam_status[k] = 0;
    return;
  }
  int np = P.n_pts ? P.n_pts[k] : 9;
  int status = (np < 2 || np > 9) ? scale::kBadPoints : 0;
  double *seg = P.lam_seg + k;
  if (!status) {
    const double *pt = P.pts + k;
    double p1 = pt[0], v1 = pt[P.pts_stride], t1 = pt[2 * P.pts_stride];
    for (int j = 0; j + 1 < np; j++) {
      const double *q = pt + (int64_t)(j + 1) * 3 * P.pts_stride;
      const double p2 = q[0], v2 = q[P.pts_stride], t2 = q[2 * P.pts_stride];
      double o[8];
      status |= scale::build_seg(p1, v1, t1, p2, v2, t2, P.robust != 0, o);
#pragma unroll
      for (int f = 0; f < 8; f++) seg[(int64_t)(j * 8 + f) * n] = o[f];
      p1 = p2; v1 = v2; t1 = t2;
    }
    if (status & scale::kBadPoints) status = scale::kBadPoints;
  }
  P.lam_status[k] = (uint8_t)status;
  if (P.status) P.status[k] = (uint8_t)status;
  if (status) {
    P.lam_n[k] = 0;
    return;
  }
  const int nl = np - 1;
  const TableLoader ld{seg, n};
  // trajectory.h:155-158: Ts[s] = lambda.getT(taus[s]) (this lane reads back its own stores)
  double last = 0.0;
  for (int s = 0; s <= S; s++) {
    last = scale::lambda_getT(ld, nl, P.tab_tau[(int64_t)s * n + k]);
    P.lam_Ts[(int64_t)s * n + k] = last;
    if (P.Ts) P.Ts[(int64_t)s * P.ts_stride + k] = last;
  }
  P.lam_total[k] = last;
  P.lam_n[k] = nl;
  if (P.total) P.total[k] = last;
  if (P.n_lseg) P.n_lseg[k] = nl;
  if (P.segs) {
    for (int r = 0; r < nl * 8; r++) P.segs[(int64_t)r * P.seg_stride + k] = seg[(int64_t)r * n];
  }
}

// Trajectory::scale, trajectory.h:140-153: (1 / ri, 0, 0) and (1 / rf, 0, taus.back()); a ratio that is <= 0 or not finite leaves no points
__global__ __launch_bounds__(kProbBlock) void lambda_scale_points_kernel(const ScaleArgs P) {
  const int64_t n = P.n_prob;
  const int64_t k = (int64_t)blockIdx.x * kProbBlock + threadIdx.x;
  if (k >= n) return;
  const double ri = P.ri_arr ? P.ri_arr[k] : P.ri, rf = P.rf_arr ? P.rf_arr[k] : P.rf;
  double *pt = P.w_pts + k;
  pt[0 * n] = 1.0 / ri;
  pt[1 * n] = 0.0;
  pt[2 * n] = 0.0;
  pt[3 * n] = 1.0 / rf;
  pt[4 * n] = 0.0;
  pt[5 * n] = P.tab_T[k];
  P.w_npts[k] = (ri > 0 && rf > 0 && isfinite(ri) && isfinite(rf)) ? 2 : 0;
}

template <int D>
__global__ __launch_bounds__(kBlock) void lambda_down_seg_kernel(const ScaleArgs P) {
  constexpr int NC = 6 * D + 2;
  const int64_t n = P.n_prob;
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int s_max = P.w_max - 1;
  if (g >= n * s_max) return;
  const int64_t s = g / n, k = g - s * n;
  if (s >= P.tab_S[k]) return;
  const double *seg = P.tab_seg + s * NC * n + k;
  const double T = P.tab_dt[s * n + k], tau0 = P.tab_tau[s * n + k];
  scale::DownRec r{0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < D; i++) {
    double c[6];
#pragma unroll
    for (int j = 0; j < 6; j++) c[j] = seg[(int64_t)(6 * i + j) * n];
    if (P.mv > 0) scale::down_axis<1>(c, T, tau0, s == 0, P.mv, r);
    if (P.ma > 0) scale::down_axis<2>(c, T, tau0, s == 0, P.ma, r);
  }
  double *o = P.down_seg + s * 3 * n + k;
  o[0] = r.max_l;
  o[n] = r.t_lo;
  o[2 * n] = r.t_hi;
}

__global__ __launch_bounds__(kProbBlock) void lambda_down_points_kernel(const ScaleArgs P) {
  const int64_t n = P.n_prob;
  const int64_t k = (int64_t)blockIdx.x * kProbBlock + threadIdx.x;
  if (k >= n) return;
  const int S = P.tab_S[k];
  if (S == 0) {
    P.w_scaled[k] = 0;
    return;  // a failed problem: the caller's bytes stay
  }
  scale::DownRec r{0.0, 0.0, 0.0};
  for (int s = 0; s < S; s++) {
    const double *o = P.down_seg + (int64_t)s * 3 * n + k;
    if (o[0] == 0) continue;
    scale::down_record(r, o[0], o[n]);
    scale::down_record(r, o[0], o[2 * n]);
  }
  const bool scaled = r.max_l > 0;
  P.w_scaled[k] = scaled ? 1 : 0;
  if (P.scaled) P.scaled[k] = scaled ? 1 : 0;
  if (!scaled) return;
  P.w_res[k] = r.max_l;
  P.w_res[n + k] = r.t_lo;
  P.w_res[2 * n + k] = r.t_hi;
  if (P.max_l) P.max_l[k] = r.max_l;
  if (P.t_lo) P.t_lo[k] = r.t_lo;
  if (P.t_hi) P.t_hi[k] = r.t_hi;
  const double T = P.tab_T[k];
  // ri / rf <= 0: max_l; a NaN is kept and fails the build
  const double pi = P.ri <= 0 ? r.max_l : P.ri, pf = P.rf <= 0 ? r.max_l : P.rf;
  double *pt = P.w_pts + k;
  int np = 0;
  auto put = [&](double p, double t) {
    pt[(int64_t)(np * 3 + 0) * n] = p;
    pt[(int64_t)(np * 3 + 1) * n] = 0.0;
    pt[(int64_t)(np * 3 + 2) * n] = t;
    np++;
  };
  put(pi, 0.0);
  put(r.max_l, r.t_lo);  // (t_lo > 0: a record of segment 0 is a root inside it or its end)
  if (r.t_hi > r.t_lo) put(r.max_l, r.t_hi);
  if (T > r.t_hi) put(pf, T);
  P.w_npts[k] = np;
}

__global__ __launch_bounds__(kBlock) void lambda_tau_kernel(const ScaleArgs P) {
  const int64_t n = P.n_prob;
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n * P.count) return;
  const int64_t k = g / P.count, i = g - k * P.count;
  if (P.tab_S[k] == 0) return;
  const int nl = P.lam_n[k];
  const double T = P.tab_T[k], total = nl > 0 ? P.lam_total[k] : T;
  double time;
  if (P.n_uniform > 0) {
    const double step = total / (double)P.n_uniform;  // trajectory.h:233-234
    time = scale::uniform_time(i, P.n_uniform, step, total, nl > 0 && P.robust != 0);
  } else {
    time = P.times[k * P.time_stride + i];
  }
  double tau = time, lam = 1.0, lam_dot = 0.0;
  bool found = true;
  if (!isfinite(time)) {
    tau = lam = lam_dot = NAN;
    found = false;
  } else if (nl > 0) {
    const TableLoader ld{P.lam_seg + k, n};
    double raw;
    scale::sample_tau(ld, nl, P.robust != 0, time, total, T, &raw, &found, &lam, &lam_dot);
    tau = raw;
  }
  const int64_t o = k * P.out_stride + i;
  if (P.tau) P.tau[o] = tau;
  if (P.lam) P.lam[o] = lam;
  if (P.lam_dot) P.lam_dot[o] = lam_dot;
  if (P.found) P.found[o] = found ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void lambda_total_kernel(const ScaleArgs P) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= P.n_prob) return;
  if (P.tab_S[k] > 0 && P.lam_n[k] > 0) P.total_time[k] = P.lam_total[k];
}

hipError_t blocks_of(int64_t lanes, int block, unsigned *out) {
  const int64_t b = (lanes + block - 1) / block;
  if (b > 0x7fffffffLL) return hipErrorInvalidValue;
  *out = (unsigned)b;
  return hipSuccess;
}

}  // namespace

hipError_t launch_lambda_build(const ScaleArgs &a, hipStream_t s) {
  if (a.n_prob == 0) return hipSuccess;
  unsigned b;
  if (hipError_t e = blocks_of(a.n_prob, kProbBlock, &b)) return e;
  hipLaunchKernelGGL(lambda_build_kernel, dim3(b), dim3(kProbBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_lambda_scale(const ScaleArgs &a, hipStream_t s) {
  if (a.n_prob == 0) return hipSuccess;
  unsigned b;
  if (hipError_t e = blocks_of(a.n_prob, kProbBlock, &b)) return e;
  hipLaunchKernelGGL(lambda_scale_points_kernel, dim3(b), dim3(kProbBlock), 0, s, a);
  ScaleArgs q = a;
  q.pts = a.w_pts; q.pts_stride = a.n_prob; q.n_pts = a.w_npts; q.only = nullptr;
  return launch_lambda_build(q, s);
}

hipError_t launch_lambda_scale_down(int dim, const ScaleArgs &a, hipStream_t s) {
  if (a.n_prob == 0) return hipSuccess;
  unsigned b, sb;
  if (hipError_t e = blocks_of(a.n_prob, kProbBlock, &b)) return e;
  if (hipError_t e = blocks_of(a.n_prob * (a.w_max - 1), kBlock, &sb)) return e;
  if (dim == 2) hipLaunchKernelGGL((lambda_down_seg_kernel<2>), dim3(sb), dim3(kBlock), 0, s, a);
  else if (dim == 3) hipLaunchKernelGGL((lambda_down_seg_kernel<3>), dim3(sb), dim3(kBlock), 0, s, a);
  else return hipErrorInvalidValue;
  hipLaunchKernelGGL(lambda_down_points_kernel, dim3(b), dim3(kProbBlock), 0, s, a);
  ScaleArgs q = a;
  q.pts = a.w_pts; q.pts_stride = a.n_prob; q.n_pts = a.w_npts; q.only = a.w_scaled;
  return launch_lambda_build(q, s);
}

hipError_t launch_lambda_tau(const ScaleArgs &a, hipStream_t s) {
  if (a.n_prob * a.count == 0) return hipSuccess;
  unsigned b;
  if (hipError_t e = blocks_of(a.n_prob * a.count, kBlock, &b)) return e;
  hipLaunchKernelGGL(lambda_tau_kernel, dim3(b), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_lambda_total(const ScaleArgs &a, hipStream_t s) {
  if (a.n_prob == 0) return hipSuccess;
  unsigned b;
  if (hipError_t e = blocks_of(a.n_prob, kBlock, &b)) return e;
  hipLaunchKernelGGL(lambda_total_kernel, dim3(b), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace mplx
