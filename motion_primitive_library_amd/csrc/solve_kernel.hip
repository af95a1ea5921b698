// solve_kernel.hip -- the batched trajectory solver for gfx950 (MI355X): K independent minimum-velocity / acceleration /
// jerk polynomials through waypoints (include/mplx_solve.h; reference src/mpl_traj_solver/poly_solver.cpp:23-221,
// include/mpl_traj_solver/traj_solver.h, src/mpl_traj_solver/poly_traj.cpp).
//
// solve_kernel<D, SO>: one lane per problem, the shape of rollout_kernel / traj_chain_kernel.  The reference forms three
// dense S N x S N matrices; none is formed here.  h = SO + 1 derivatives per waypoint, N = 2 h coefficients per segment:
//   * A is block diagonal, so a segment of duration T contributes H = A^-T Q A^-1, an N x N cost on the derivatives of
//     its two ends.  In the scaled variable s = t / T that matrix is a constant Hhat (integers, hhat() below) and
//     H[i][j] = Hhat[i][j] / T^(2h - 1 - k_i - k_j), k the derivative order of a row: no inverse is computed.
//   * summed over the segments, R is block tridiagonal in waypoint order with h x h blocks G_w = H_{w-1}[TT] + H_w[00]
//     and C_w = H_w[0T].  A fixed derivative keeps its place in the block: its row and column become the identity and its
//     value moves to the right-hand sides, so every block has the compile-time size h and the free system is the
//     reference's Rpp (its free block is in waypoint order as well) bordered by ones.
//   * forward over the waypoints: G'_w = G_w - C_{w-1}^T Z_{w-1}, b'_w = b_w - C_{w-1}^T z_{w-1}, an LDL^T of G'_w without
//     pivoting (the matrix is symmetric positive definite for a well-posed problem; a pivot that is not finite or <= 0 is
//     MPLX_SOLVE_SINGULAR), Z_w = G'_w^-1 C_w, z_w = G'_w^-1 b'_w for the D axes that share the matrix.  Z and z go to the
//     workspace of the poly, problem-minor: row r of waypoint w at ws[(w * (h h + h D) + r) * n + k].
//   * backward: x_w = z_w - Z_w x_{w+1}; with both ends' derivatives in registers the segment's coefficients: the low
//     half p_k = d_k / k!, the high half from the h x h system of the end conditions, whose inverse in the scaled variable
//     is again a constant (binv()).
// Every small matrix lives in registers with compile-time indices (all loops over h, D are unrolled); no LDS, no
// cross-lane traffic; every global access is [row][k], coalesced over the wave.
//
// Bit-exactness: -ffp-contract=off, true divisions, powers by repeated multiply.  dts of allocate_time, taus, the whole
// SO = 0 solve with fixed positions (p0 = pos_w, p1 = (pos_{w+1} - pos_w) / T) and the yaw solve are the reference's
// arithmetic bit for bit; the coefficients for SO >= 1 follow another elimination order than Eigen's dense LU and agree
// to rounding.
#include "mplx_internal.h"

#include <math.h>

namespace mplx {
namespace {

constexpr int kBlock = 64;  // one wave: K problems spread over as many CUs as K / 64 allows

// Hhat of a unit-duration segment: rows / columns = the h derivatives at its start, then at its end.
template <int H>
__device__ __forceinline__ constexpr double hhat(int i, int j) {
  if constexpr (H == 1) {
    constexpr double t[2][2] = {{1, -1}, {-1, 1}};
    return t[i][j];
  } else if constexpr (H == 2) {
    constexpr double t[4][4] = {{12, 6, -12, 6}, {6, 4, -6, 2}, {-12, -6, 12, -6}, {6, 2, -6, 4}};
    return t[i][j];
  } else {
    constexpr double t[6][6] = {{720, 360, 60, -720, 360, -60},  {360, 192, 36, -360, 168, -24}, {60, 36, 9, -60, 24, -3},
                                {-720, -360, -60, 720, -360, 60}, {360, 168, 24, -360, 192, -36}, {-60, -24, -3, 60, -36, 9}};
    return t[i][j];
  }
}

// inverse of B[r][j] = (h + j)! / (h + j - r)!: the end conditions of the high half in the scaled variable
template <int H>
__device__ __forceinline__ constexpr double binv(int j, int r) {
  if constexpr (H == 1) {
    return 1.0;
  } else if constexpr (H == 2) {
    constexpr double t[2][2] = {{3, -1}, {-2, 1}};
    return t[j][r];
  } else {
    constexpr double t[3][3] = {{10, -4, 0.5}, {-15, 7, -1}, {6, -3, 0.5}};
    return t[j][r];
  }
}

__device__ __forceinline__ constexpr double fact(int n) { return n <= 1 ? 1.0 : n * fact(n - 1); }
// n! / (n - q)!
__device__ __forceinline__ constexpr double falling(int n, int q) { return q == 0 ? 1.0 : (n - q + 1) * falling(n, q - 1); }

template <int D, int SO>
__global__ __launch_bounds__(kBlock) void solve_kernel(const SolveArgs P) {
  constexpr int h = SO + 1, N = 2 * h, F = 4 * D + 2, NC = 6 * D + 2, WS = h * h + h * D;
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= P.n_prob) return;
  const int64_t n = P.cap;
  const int64_t wmax = P.w_max;
  int W = P.n_wp ? P.n_wp[k] : P.w_max;
  if (W > P.w_max) W = P.w_max;
  const double *wp = P.waypoints + k;
  const double vk = P.v_arr ? P.v_arr[k] : P.v;
  uint8_t status = W < 2 ? 1 : 0;  // MPLX_SOLVE_EMPTY

  // ---- forward: durations, taus, the elimination
  double cur[h][D], nx[h][D];
  uint32_t fc = 0, fn = 0;  // fixed masks of the current / next waypoint
  double gtt[h][h], carry[h][D], cp[h][h], zp[h][h], zr[h][D];
#pragma unroll
  for (int a = 0; a < h; a++) {
#pragma unroll
    for (int b = 0; b < h; b++) gtt[a][b] = cp[a][b] = zp[a][b] = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) carry[a][i] = zr[a][i] = nx[a][i] = cur[a][i] = 0.0;
  }
  if (!status) {
#pragma unroll
    for (int a = 0; a < h; a++)
#pragma unroll
      for (int i = 0; i < D; i++) cur[a][i] = wp[((int64_t)(a * D + i) * wmax + 0) * P.wp_stride];
    fc = P.wp_flags ? (P.wp_flags[k] & ((1u << h) - 1)) : (1u << h) - 1;
  }
  double tau = 0.0;
  if (!status) P.tab_tau[k] = tau;
  for (int w = 0; w < W && !status; w++) {
    const bool last = w == W - 1;
    double H00[h][h], H0T[h][h], HTT[h][h];
#pragma unroll
    for (int a = 0; a < h; a++)
#pragma unroll
      for (int b = 0; b < h; b++) H00[a][b] = H0T[a][b] = HTT[a][b] = 0.0;
    if (!last) {
#pragma unroll
      for (int a = 0; a < h; a++)
#pragma unroll
        for (int i = 0; i < D; i++) nx[a][i] = wp[((int64_t)(a * D + i) * wmax + (w + 1)) * P.wp_stride];
      if (P.wp_flags) fn = P.wp_flags[(int64_t)(w + 1) * P.flag_stride + k] & ((1u << h) - 1);
      else fn = (w + 1 == W - 1) ? (1u << h) - 1 : 1u;
      double T;
      if (P.dts) {
        T = P.dts[(int64_t)w * P.dt_stride + k];
      } else {  // traj_solver.h:122-130: the L-inf distance over v
        double m = fabs(nx[0][0] - cur[0][0]);
#pragma unroll
        for (int i = 1; i < D; i++) {
          const double d = fabs(nx[0][i] - cur[0][i]);
          if (d > m) m = d;
        }
        T = m / vk;
      }
      if (!(T > 0.0) || !isfinite(T) || (!P.dts && !(vk > 0.0))) {
        status = 2;  // MPLX_SOLVE_BAD_TIME
        break;
      }
      P.tab_dt[(int64_t)w * n + k] = T;
      tau = tau + T;  // poly_traj.cpp:67
      P.tab_tau[(int64_t)(w + 1) * n + k] = tau;
      double tp[N];
      tp[0] = 1.0;
#pragma unroll
      for (int m = 1; m < N; m++) tp[m] = tp[m - 1] * T;
#pragma unroll
      for (int a = 0; a < h; a++)
#pragma unroll
        for (int b = 0; b < h; b++) {
          H00[a][b] = hhat<h>(a, b) / tp[2 * h - 1 - a - b];
          H0T[a][b] = hhat<h>(a, h + b) / tp[2 * h - 1 - a - b];
          HTT[a][b] = hhat<h>(h + a, h + b) / tp[2 * h - 1 - a - b];
        }
    }
    double G[h][h], C[h][h], b[h][D];
#pragma unroll
    for (int a = 0; a < h; a++)
#pragma unroll
      for (int c = 0; c < h; c++) G[a][c] = gtt[a][c] + H00[a][c];
    // right-hand sides: minus the fixed derivatives of w - 1 (carried), w and w + 1 through R
#pragma unroll
    for (int a = 0; a < h; a++) {
#pragma unroll
      for (int i = 0; i < D; i++) {
        double acc = carry[a][i];
#pragma unroll
        for (int j = 0; j < h; j++)
          if (fc >> j & 1) acc = acc - G[a][j] * cur[j][i];
#pragma unroll
        for (int j = 0; j < h; j++)
          if (!last && (fn >> j & 1)) acc = acc - H0T[a][j] * nx[j][i];
        b[a][i] = (fc >> a & 1) ? cur[a][i] : acc;
      }
    }
#pragma unroll
    for (int a = 0; a < h; a++)
#pragma unroll
      for (int c = 0; c < h; c++) {
        C[a][c] = (!last && !(fc >> a & 1) && !(fn >> c & 1)) ? H0T[a][c] : 0.0;
        if ((fc >> a & 1) || (fc >> c & 1)) G[a][c] = a == c ? 1.0 : 0.0;
      }
    if (w > 0) {  // the Schur complement of the waypoints before
#pragma unroll
      for (int a = 0; a < h; a++) {
#pragma unroll
        for (int c = 0; c <= a; c++) {
          double s = G[a][c];
#pragma unroll
          for (int m = 0; m < h; m++) s = s - cp[m][a] * zp[m][c];
          G[a][c] = s;
          G[c][a] = s;
        }
#pragma unroll
        for (int i = 0; i < D; i++) {
          double s = b[a][i];
#pragma unroll
          for (int m = 0; m < h; m++) s = s - cp[m][a] * zr[m][i];
          b[a][i] = s;
        }
      }
    }
    // G = L diag(dd) L^T
    double L[h][h], dd[h];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < h; j++) {
      double s = G[j][j];
#pragma unroll
      for (int m = 0; m < j; m++) s = s - L[j][m] * L[j][m] * dd[m];
      dd[j] = s;
      bad = bad || !(s > 0.0) || !isfinite(s);
#pragma unroll
      for (int i = j + 1; i < h; i++) {
        double q = G[i][j];
#pragma unroll
        for (int m = 0; m < j; m++) q = q - L[i][m] * L[j][m] * dd[m];
        L[i][j] = q / s;
      }
    }
    if (bad) {
      status = 8;  // MPLX_SOLVE_SINGULAR
      break;
    }
    // [Z | z] = G^-1 [C | b]
    double X[h][h + D];
#pragma unroll
    for (int a = 0; a < h; a++) {
#pragma unroll
      for (int c = 0; c < h; c++) X[a][c] = C[a][c];
#pragma unroll
      for (int i = 0; i < D; i++) X[a][h + i] = b[a][i];
    }
#pragma unroll
    for (int c = 0; c < h + D; c++) {
#pragma unroll
      for (int a = 0; a < h; a++)
#pragma unroll
        for (int m = 0; m < a; m++) X[a][c] = X[a][c] - L[a][m] * X[m][c];
#pragma unroll
      for (int a = 0; a < h; a++) X[a][c] = X[a][c] / dd[a];
#pragma unroll
      for (int a = h - 1; a >= 0; a--)
#pragma unroll
        for (int m = a + 1; m < h; m++) X[a][c] = X[a][c] - L[m][a] * X[m][c];
    }
    double *ws = P.ws + (int64_t)w * WS * n + k;
#pragma unroll
    for (int a = 0; a < h; a++) {
#pragma unroll
      for (int c = 0; c < h; c++) {
        zp[a][c] = X[a][c];
        cp[a][c] = C[a][c];
        ws[(int64_t)(a * h + c) * n] = X[a][c];
      }
#pragma unroll
      for (int i = 0; i < D; i++) {
        zr[a][i] = X[a][h + i];
        ws[(int64_t)(h * h + a * D + i) * n] = X[a][h + i];
      }
    }
    // what waypoint w + 1 inherits: H[TT], and minus H[T0] times the fixed derivatives of w
#pragma unroll
    for (int a = 0; a < h; a++) {
#pragma unroll
      for (int c = 0; c < h; c++) gtt[a][c] = HTT[a][c];
#pragma unroll
      for (int i = 0; i < D; i++) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < h; j++)
          if (fc >> j & 1) acc = acc - H0T[j][a] * cur[j][i];
        carry[a][i] = acc;
      }
    }
#pragma unroll
    for (int a = 0; a < h; a++)
#pragma unroll
      for (int i = 0; i < D; i++) cur[a][i] = nx[a][i];
    fc = fn;
  }

  P.tab_status[k] = status;
  if (P.status) P.status[k] = status;
  if (status) {  // a failed problem: its status only; samples and traversals skip it (S = 0)
    P.tab_S[k] = 0;
    P.tab_T[k] = 0.0;
    return;
  }
  const int S = W - 1;
  P.tab_S[k] = S;
  P.tab_T[k] = tau;
  if (P.n_segs) P.n_segs[k] = S;
  if (P.total_time) P.total_time[k] = tau;
  if (P.taus_out) P.taus_out[(int64_t)S * P.taus_stride + k] = tau;

  // ---- backward: x_w = z_w - Z_w x_{w+1}, then the coefficients of segment w
  double xn[h][D];
  double yaw_n = wp[((int64_t)(4 * D) * wmax + S) * P.wp_stride];
#pragma unroll
  for (int a = 0; a < h; a++)
#pragma unroll
    for (int i = 0; i < D; i++) xn[a][i] = (fc >> a & 1) ? cur[a][i] : zr[a][i];  // (cur, fc: waypoint W - 1)
#pragma unroll
  for (int f = 0; f < F; f++) P.tab_wp[((int64_t)f * wmax + S) * n + k] = wp[((int64_t)f * wmax + S) * P.wp_stride];
  for (int w = S - 1; w >= 0; w--) {
    const double *ws = P.ws + (int64_t)w * WS * n + k;
    uint32_t fw;
    if (P.wp_flags) fw = P.wp_flags[(int64_t)w * P.flag_stride + k] & ((1u << h) - 1);
    else fw = w == 0 ? (1u << h) - 1 : 1u;
    double x[h][D];
#pragma unroll
    for (int a = 0; a < h; a++) {
#pragma unroll
      for (int i = 0; i < D; i++) {
        double s = ws[(int64_t)(h * h + a * D + i) * n];
#pragma unroll
        for (int j = 0; j < h; j++) s = s - ws[(int64_t)(a * h + j) * n] * xn[j][i];
        const double given = wp[((int64_t)(a * D + i) * wmax + w) * P.wp_stride];
        x[a][i] = (fw >> a & 1) ? given : s;
      }
    }
#pragma unroll
    for (int f = 0; f < F; f++) P.tab_wp[((int64_t)f * wmax + w) * n + k] = wp[((int64_t)f * wmax + w) * P.wp_stride];
    const double T = P.tab_dt[(int64_t)w * n + k];
    double tp[N];
    tp[0] = 1.0;
#pragma unroll
    for (int m = 1; m < N; m++) tp[m] = tp[m - 1] * T;
    double *seg = P.tab_seg + (int64_t)w * NC * n + k;
#pragma unroll
    for (int i = 0; i < D; i++) {
      double p[N], pt[h], r[h];
#pragma unroll
      for (int a = 0; a < h; a++) {
        p[a] = x[a][i] / fact(a);
        pt[a] = p[a] * tp[a];
      }
#pragma unroll
      for (int q = 0; q < h; q++) {  // what the low half leaves of the end's derivative q, in the scaled variable
        double acc = xn[q][i] * tp[q];
#pragma unroll
        for (int m = q; m < h; m++) acc = acc - falling(m, q) * pt[m];
        r[q] = acc;
      }
#pragma unroll
      for (int j = 0; j < h; j++) {
        double acc = binv<h>(j, 0) * r[0];
#pragma unroll
        for (int q = 1; q < h; q++) acc = acc + binv<h>(j, q) * r[q];
        p[h + j] = acc / tp[h + j];
      }
#pragma unroll
      for (int m = 0; m < N; m++)
        if (P.coeff) P.coeff[((int64_t)(w * N + m) * D + i) * P.coeff_stride + k] = p[m];
      // poly_traj.cpp:72-88: Vec6f c_j = p_{5-j} (5-j)!, absent coefficients 0
#pragma unroll
      for (int j = 0; j < 6; j++) seg[(int64_t)(6 * i + j) * n] = (5 - j) < N ? p[5 - j] * fact(5 - j) : 0.0;
    }
    // the yaw solve with yaw_control = VEL (traj_solver.h:87-101): every yaw fixed
    const double yaw_w = wp[((int64_t)(4 * D) * wmax + w) * P.wp_stride];
    const double y0 = yaw_w / 1.0, uy = (yaw_n - yaw_w) / T;
    seg[(int64_t)(6 * D) * n] = uy * 1.0;
    seg[(int64_t)(6 * D + 1) * n] = y0 * 1.0;
    if (P.yaw_coeff) {
      P.yaw_coeff[(int64_t)(2 * w) * P.yaw_stride + k] = y0;
      P.yaw_coeff[(int64_t)(2 * w + 1) * P.yaw_stride + k] = uy;
    }
    if (P.dts_out) P.dts_out[(int64_t)w * P.dts_out_stride + k] = T;
    if (P.taus_out) P.taus_out[(int64_t)w * P.taus_stride + k] = P.tab_tau[(int64_t)w * n + k];
    yaw_n = yaw_w;
#pragma unroll
    for (int a = 0; a < h; a++)
#pragma unroll
      for (int i = 0; i < D; i++) xn[a][i] = x[a][i];
  }
}

template <int D, int SO>
hipError_t solve_one(const SolveArgs &a, hipStream_t s) {
  const int64_t blocks = (a.n_prob + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((solve_kernel<D, SO>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <int D>
hipError_t solve_dim(const SolveArgs &a, hipStream_t s) {
  switch (a.so) {
    case 0: return solve_one<D, 0>(a, s);
    case 1: return solve_one<D, 1>(a, s);
    case 2: return solve_one<D, 2>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_solve(int dim, const SolveArgs &a, hipStream_t s) {
  if (a.n_prob == 0) return hipSuccess;
  if (dim == 2) return solve_dim<2>(a, s);
  if (dim == 3) return solve_dim<3>(a, s);
  return hipErrorInvalidValue;
}

}  // namespace mplx
