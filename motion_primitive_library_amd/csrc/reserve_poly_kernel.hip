// reserve_poly_kernel.hip -- the problems of a solved set against a reservation table, for gfx950 (MI355X)
// (include/mplx_reserve_poly.h states the semantics; tests/reserve_poly_model.py restates them sequentially).
//
// reserve_poly_kernel<D, LAMBDA>: one wave (a workgroup of 64 lanes) per problem.  Everything of the problem is
// wave-uniform: its status, S, total, t_start, radius, ignored group, the horizon test and the first instant -- a guess
// from t_start / step, then a scan of at most kScan instants for the first with tl_i >= 0 (tl_i is monotone in i).  A
// problem is active at few instants (a shortcut's pair lasts a handful of primitives), so no K x n_steps position table
// is built: the wave walks the problem's instants upwards in blocks of 64.  Per block each lane evaluates the problem's
// own position at ONE instant -- the glue of conflict_pos_kernel around scale::sample_tau, traj::find_segment and
// traj::eval_segment, so the position is the table's own for this set -- and leaves it in LDS (64 D doubles); the block
// ends at the first instant past total or n_steps.  Then the lanes are 64 consecutive reservations: coalesced reads of
// pos[d][i][b0 + lane] and active[i][b0 + lane], the own position read from LDS at a wave-uniform address (a
// broadcast), kInst instants per pass without a branch that depends on a load so that the reads of a pass are in flight
// together.  A lane keeps the smallest (i << 32 | b) it meets; instants ascend from pass to pass, so the first pass with
// a hit ends the problem and a wave minimum is its answer.  What a lane needs of its first kKeep reservations (radius
// sum, or NaN where the reservation is excluded or of the ignored group: rr = NaN makes d2 < rr * rr false) is computed
// once per problem and kept in registers; segment coefficients are not held across the loop.
//
// Every output is a minimum or a sum of integers, hence a pure function of the inputs.  No workgroup waits for another;
// every loop is bounded by kScan, n_steps, B or S (the bisection of find_segment); the barriers are inside loops whose
// trip counts are wave-uniform and the workgroup is one wave.  LDS: 64 D doubles = 1.5 KB at D = 3.
//
// reserve_pair_rows_kernel: one lane per pair of a timed shortcut: its clock start, radius and ignored group.
#include "mplx_internal.h"
#include "mplx_scale_math.h"
#include "mplx_traj_device.h"

#include <math.h>

namespace mplx {
namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kScan = 4;   // the guess is floor(x) - 1 with x within a few ulps of the first instant's index
constexpr int kKeep = 4;   // reservations per lane whose radius sum stays in registers
constexpr int kInst = 8;   // instants per pass
constexpr long long kNoHit = 0x7fffffffffffffffLL;

template <int D, bool LAMBDA>
__global__ __launch_bounds__(kWave) void reserve_poly_kernel(const ReservePolyArgs P) {
  __shared__ double s_p[D][kWave];
  const ReserveArgs &A = P.res;
  const TrajArgs &R = P.traj;
  const int64_t k = blockIdx.x, N = P.K;
  const int lane = threadIdx.x;

  // ---- the problem (wave-uniform)
  const uint8_t st = R.tab_status[k];
  const int S = R.tab_S[k];
  const double ts = P.t_start[k];
  const double rq = P.radius ? P.radius[k] : P.radius_all;
  const int32_t ign = P.ignore ? P.ignore[k] : -1;
  const bool bad = !isfinite(ts) || !(rq >= 0.0) || !isfinite(rq);
  long long out = -1;
  if (S > 0 && st == 0 && !bad) {
    const double T = R.tab_T[k];
    const int nl = LAMBDA ? R.lam_n[k] : 0;
    const double total = nl > 0 ? R.lam_total[k] : T;
    if ((double)(A.n_steps - 1) * A.step - ts < total) {
      out = -2;
    } else {
      // the first instant with tl_i >= 0; n_steps: none
      int64_t i_first = A.n_steps;
      {
        const double x = ts / A.step;
        int64_t g = 0;
        if (x >= 1.0) g = x < 2147483647.0 ? (int64_t)x - 1 : (int64_t)A.n_steps;
        for (int s = 0; s < kScan; s++) {
          const int64_t i = g + s;
          if (i >= A.n_steps) break;
          if ((double)i * A.step - ts >= 0.0) {
            i_first = i;
            break;
          }
        }
      }
      double rrk[kKeep];
#pragma unroll
      for (int j = 0; j < kKeep; j++) {
        const int64_t b = (int64_t)j * kWave + lane;
        rrk[j] = NAN;
        if (b < A.B && A.incl[b] != 0 && A.group[b] != ign) rrk[j] = rq + A.r[b];
      }
      long long key = kNoHit;
      for (int64_t ib = i_first; ib < A.n_steps && key == kNoHit; ib += kWave) {
        // ---- the problem's own positions of this block, one instant per lane
        const int64_t il = ib + lane;
        const double tl = (double)il * A.step - ts;
        const bool in = il < A.n_steps && tl >= 0.0 && tl <= total;
        const int nv = __popcll(__ballot(in));  // (tl is monotone: the instants of the problem are the first nv of the block)
        if (nv == 0) break;
        __syncthreads();  // the previous block has been read
        if (in) {
          // conflict_pos_kernel, Command form, on a solved set
          double tau = tl, lambda = 1.0, lambda_dot = 0.0;
          if (nl > 0) {
            const scale::TableLoader ld{R.lam_seg + k, N};
            double raw;
            bool found;
            tau = scale::sample_tau(ld, nl, R.lam == 2, tl, R.lam_total[k], T, &raw, &found, &lambda, &lambda_dot);
          } else {
            if (tau < 0) tau = 0;
            if (tau > T) tau = T;
          }
          const double *taus = R.tab_tau + k;
          const int id = traj::find_segment<true, true>(taus, N, S, tau, R.env.dt);
          tau -= taus[(int64_t)id * N];
          traj::Sample<D> sm;
          traj::eval_segment<D, true, false, true>(R.tab_seg + (int64_t)id * (6 * D + 2) * N + k, N, tau, sm);
#pragma unroll
          for (int d = 0; d < D; d++) s_p[d][lane] = sm.pos[d];
        }
        __syncthreads();
        // ---- against the reservations, kInst instants per pass
        for (int u0 = 0; u0 < nv && key == kNoHit; u0 += kInst) {
          long long mine = kNoHit;
          int j = 0;
          for (int64_t b = lane; b < A.B; b += kWave, j++) {
            double rr;
            if (j < kKeep) {
              rr = j == 0 ? rrk[0] : j == 1 ? rrk[1] : j == 2 ? rrk[2] : rrk[3];
            } else {
              rr = (A.incl[b] != 0 && A.group[b] != ign) ? rq + A.r[b] : NAN;
            }
            const double rr2 = rr * rr;
#pragma unroll
            for (int u = 0; u < kInst; u++) {
              if (u0 + u < nv) {  // (wave-uniform)
                const int64_t iu = ib + u0 + u, at = iu * A.B + b;
                const bool on = A.act[at] != 0;
                const double dx = s_p[0][u0 + u] - A.pos[at], dy = s_p[1][u0 + u] - A.pos[(int64_t)A.n_steps * A.B + at];
                double d2 = (dx * dx) + dy * dy;
                if (D == 3) {
                  const double dz = s_p[D - 1][u0 + u] - A.pos[(int64_t)(D - 1) * A.n_steps * A.B + at];
                  d2 = d2 + dz * dz;
                }
                const long long cand = (long long)((unsigned long long)iu << 32) | (long long)b;
                if (on && d2 < rr2 && cand < mine) mine = cand;  // (a NaN on either side compares false)
              }
            }
          }
          // instants ascend from pass to pass: the minimum over the pass is the problem's smallest
          if (__ballot(mine != kNoHit) != 0ull) {
            for (int m = 1; m < kWave; m <<= 1) {
              const long long o = __shfl_xor(mine, m);
              mine = o < mine ? o : mine;
            }
            key = mine;
          }
        }
        if (nv < kWave) break;  // the problem's last instant lay in this block
      }
      if (key != kNoHit) out = key;
    }
  }
  if (lane == 0) {
    if (P.hit) P.hit[k] = out;
    if (P.status) P.status[k] = (uint8_t)(st | (bad ? 128 : 0));  // MPLX_CONFLICT_BAD_INPUT
    if (P.n_hit && out != -1) atomicAdd(P.n_hit, 1ull);
  }
}

__global__ __launch_bounds__(kBlock) void reserve_pair_rows_kernel(const PairRowsArgs P) {
  const int64_t NP = P.n_query * (P.w_max - 1) * P.max_hop;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= NP) return;
  const int64_t ki = p / P.max_hop;
  const int64_t k = ki / (P.w_max - 1);
  const int i = (int)(ki - k * (P.w_max - 1));
  P.t_start[p] = P.q_t0[k] + P.t_row[(int64_t)i * P.stride + k];
  P.radius[p] = P.q_r[k];
  P.ignore[p] = P.q_ignore[k];
}

}  // namespace

hipError_t launch_reserve_check_poly(int dim, const ReservePolyArgs &a, hipStream_t s) {
  if (a.K <= 0) return hipSuccess;
  if (a.K > 0x7fffffffLL || !a.traj.poly) return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.K), block(kWave);
  if (dim == 2) {
    if (a.traj.lam) hipLaunchKernelGGL((reserve_poly_kernel<2, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((reserve_poly_kernel<2, false>), grid, block, 0, s, a);
  } else if (dim == 3) {
    if (a.traj.lam) hipLaunchKernelGGL((reserve_poly_kernel<3, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((reserve_poly_kernel<3, false>), grid, block, 0, s, a);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_reserve_pair_rows(const PairRowsArgs &a, hipStream_t s) {
  const int64_t np = a.n_query * (a.w_max - 1) * a.max_hop, blocks = (np + kBlock - 1) / kBlock;
  if (np == 0) return hipSuccess;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(reserve_pair_rows_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace mplx
