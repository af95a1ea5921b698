// reserve_kernel.hip -- the check of successor lists against a reservation table, for gfx950 (MI355X)
// (include/mplx_reserve.h states the semantics; tests/reserve_model.py restates them sequentially).
//
// reserve_check_kernel<D, K>: one wave (a workgroup of 64 lanes) per list row.  Everything a row's entries share is
// wave-uniform and computed once: the query, tp, tc, the horizon test and the row's instants -- a guess from
// (tp + t0) / step, then a scan of at most n_scan = ceil(dt / step) + 3 instants for those with tp <= tl_i <= tc (tl_i is
// monotone in i, so they are contiguous).  The lanes are 2^sp_log2 entries x P = 64 >> sp_log2 slices of the
// reservations: with |U| = 9 a row would fill 9 of 64 lanes, so four slices of 16 lanes share its entries and split
// the reservations between them; rows of more than 64 entries take several passes of one slice.  A lane holds its
// entry's segment in registers (traj::chain_segment, the chain launch's own function, with N = 1) and evaluates its
// position once per instant (traj::eval_segment).  Per instant the reservations go through LDS in tiles of kTile:
// D position doubles and one double that is the reservation's radius, or NaN where it is excluded, inactive at the
// instant or of the query's ignored group -- rr = r_q + NaN makes d2 < rr * rr false, so the inner loop is the pair
// test alone.  A lane reads the tile at an address its slice shares (a broadcast), keeps the first (i << 32 | b) it
// meets -- instants and reservations both ascend, so the first is the smallest of its slice -- and after every instant
// the slices of an entry are folded with __shfl_xor.  An instant at which no lane still looks for a conflict (ballot)
// ends the pass.
//
// Every output is a minimum or a sum of integers, hence a pure function of the inputs.  No workgroup waits for another;
// every loop is bounded by S, n_scan, n_steps or B; the barriers are inside loops whose trip counts are wave-uniform
// and the workgroup is one wave.  LDS: kTile * (D + 1) * 8 bytes = 8 KB at D = 3.
#include "mplx_internal.h"
#include "mplx_pair_device.h"
#include "mplx_traj_device.h"

#include <math.h>

namespace mplx {
namespace {

constexpr int kWave = 64;
constexpr int kTile = 256;  // reservations staged in LDS at a time
constexpr long long kNoHit = 0x7fffffffffffffffLL;

template <int D, int K>
__global__ __launch_bounds__(kWave) void reserve_check_kernel(const ReserveArgs A) {
  __shared__ double s_pos[D][kTile];
  __shared__ double s_r[kTile];

  const int64_t k = blockIdx.x;
  const int lane = threadIdx.x;
  const int SP = 1 << A.sp_log2, P = kWave >> A.sp_log2;
  const int jl = lane & (SP - 1), slice = lane >> A.sp_log2;
  const int64_t S = A.S;

  // ---- the row (wave-uniform)
  const int32_t pid = A.parent_id[k];
  const int cnt = A.count[k];
  bool row_ok = pid >= 0;
  int32_t q = 0;
  if (row_ok && A.node_query) {
    if ((int64_t)pid >= A.node_cap) row_ok = false;
    else q = A.node_query[pid];
  }
  if (q < 0 || q >= A.Q) {
    row_ok = false;
    q = 0;
  }
  const double t0 = A.q_t0[q], rq = A.q_r[q];
  const int32_t ign = A.q_ignore[q];
  constexpr int F = 4 * D + 2;
  double ps[4 * D];
#pragma unroll
  for (int f = 0; f < 4 * D; f++) ps[f] = A.parent_state[(int64_t)f * A.parent_stride + k];
  const double tp = A.parent_state[(int64_t)(F - 1) * A.parent_stride + k];
  const double tc = tp + A.dt;
  const bool horizon = (double)(A.n_steps - 1) * A.step - t0 < tc;
  // the instants [i0, i0 + ni): the guess is at most the first one (x is off by far less than 1 wherever i < 2^31)
  int i0 = 0, ni = 0;
  if (row_ok && !horizon) {
    const double x = (tp + t0) / A.step;
    int64_t g = 0;  // (a NaN goes to 0)
    if (x >= 1.0) g = x < 2147483647.0 ? (int64_t)x - 1 : (int64_t)A.n_steps;
    for (int s = 0; s < A.n_scan; s++) {
      const int64_t i = g + s;
      if (i >= A.n_steps) break;
      const double tl = (double)i * A.step - t0;
      if (tl > tc) break;
      if (tl >= tp) {
        if (ni == 0) i0 = (int)i;
        ni++;
      }
    }
  }

  unsigned int blocked_row = 0;
  for (int64_t j0 = 0; j0 < S; j0 += SP) {
    const int64_t j = j0 + jl, e = k * S + j;
    const bool mine = j < S;
    int a = -1;
    bool looked = false;
    if (row_ok && mine && j < cnt) {
      a = A.action[e];
      looked = __builtin_isfinite(A.cost[e]) && a >= 0 && a < A.nU;
    }
    double seg[5 * D + 2];
    {
      const double *up = A.U + (int64_t)(looked ? a : 0) * A.udim;  // (row 0 of a table that has one: nothing of it is used)
      pair::Axis<K> ax[D];
      traj::chain_segment<D, K>(ps, up, 0.0, 0.0, ax, seg, 1);
    }
    long long key = kNoHit;
    if (!horizon) {
      for (int ii = 0; ii < ni; ii++) {
        if (__ballot(looked && key == kNoHit) == 0ull) break;  // nobody looks for a conflict any more
        const int i = i0 + ii;
        const double tl = (double)i * A.step - t0;
        traj::Sample<D> sm;
        traj::eval_segment<D, true, false>(seg, 1, tl - tp, sm);
        const bool cand = looked && key == kNoHit;
        for (int64_t b0 = 0; b0 < A.B; b0 += kTile) {
          const int nb = A.B - b0 < kTile ? (int)(A.B - b0) : kTile;
          __syncthreads();  // the previous tile has been read
          for (int t = lane; t < nb; t += kWave) {
            const int64_t b = b0 + t, at = (int64_t)i * A.B + b;
#pragma unroll
            for (int d = 0; d < D; d++) s_pos[d][t] = A.pos[(int64_t)d * A.n_steps * A.B + at];
            const bool on = A.incl[b] != 0 && A.act[at] != 0 && A.group[b] != ign;
            s_r[t] = on ? A.r[b] : NAN;
          }
          __syncthreads();
          if (cand) {
            for (int t = slice; t < nb; t += P) {
              const double dx = sm.pos[0] - s_pos[0][t], dy = sm.pos[1] - s_pos[1][t];
              double d2 = (dx * dx) + dy * dy;
              if (D == 3) {
                const double dz = sm.pos[D - 1] - s_pos[D - 1][t];
                d2 = d2 + dz * dz;
              }
              const double rr = rq + s_r[t];
              if (d2 < rr * rr && key == kNoHit) key = ((long long)i << 32) | (long long)(b0 + t);
            }
          }
        }
        // the slices of an entry: the smallest key of the instant
        for (int m = SP; m < kWave; m <<= 1) {
          const long long o = __shfl_xor(key, m);
          key = o < key ? o : key;
        }
      }
    }
    const bool blocked = looked && (horizon || key != kNoHit);
    if (mine && slice == 0) {
      if (A.hit) A.hit[e] = blocked ? (horizon ? -2LL : key) : -1LL;
      if (blocked) A.cost[e] = INFINITY;
    }
    blocked_row += (unsigned int)__popcll(__ballot(blocked && slice == 0));
  }
  if (A.n_blocked && lane == 0 && blocked_row) atomicAdd(A.n_blocked, (unsigned long long)blocked_row);
}

template <int D>
hipError_t check_dim(int order, const ReserveArgs &a, hipStream_t s) {
  const dim3 grid((unsigned)a.n_rows), block(kWave);
  switch (order) {
    case 1: hipLaunchKernelGGL((reserve_check_kernel<D, 1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((reserve_check_kernel<D, 2>), grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL((reserve_check_kernel<D, 3>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((reserve_check_kernel<D, 4>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_reserve_check(int dim, int control, const ReserveArgs &a, hipStream_t s) {
  if (a.n_rows <= 0) return hipSuccess;
  if (a.n_rows > 0x7fffffffLL || a.sp_log2 < 0 || a.sp_log2 > 6) return hipErrorInvalidValue;
  const int ctl = control & 0x0f;
  const int order = ctl == 0x01 ? 1 : ctl == 0x03 ? 2 : ctl == 0x07 ? 3 : ctl == 0x0f ? 4 : 0;
  if (dim == 2) return check_dim<2>(order, a, s);
  if (dim == 3) return check_dim<3>(order, a, s);
  return hipErrorInvalidValue;
}

}  // namespace mplx
