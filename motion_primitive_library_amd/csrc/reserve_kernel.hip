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
//
// reserve_park_kernel<D> (mplx_reserve_park_device, park-safe goals) is described where it stands, below the check.
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
      dev::Ax<K> ax[D];
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

// reserve_park_kernel<D>: the goal-region rows of a pushed frontier against the table from the row's t on
// (mplx_reserve_park_device).  Goal rows are few among the rows of a frontier, so a wave takes 64 rows: each lane reads
// its row's id and the node's flag, a ballot gathers the rows to look at and the wave walks them together, one after
// the other.  For one row the lanes stride over the reservations (coalesced reads of pos[d][i][.] and active[i][.]),
// kParkInst instants per pass so that the reads of a pass are in flight together; a lane keeps the smallest
// (i << 32 | b) it meets, a wave minimum makes the pass's smallest, and since instants ascend the first pass with a hit
// ends the row.  What a lane needs of its first kParkKeep reservations (radius sum,
// or NaN where the reservation is excluded or of the ignored group) is computed once per row and kept in registers.
// The first instant at or after the row's t is found from a guess, (t + t0) / step, and a scan of at most n_scan
// instants (tl_i is monotone in i).  Loops are bounded by 64, n_scan, n_steps and B; no workgroup waits for another;
// the node's flag is cleared by the one lane that owns the row.
constexpr int kParkKeep = 4;
constexpr int kParkInst = 8;  // instants per pass
constexpr unsigned kIsGoalBit = 2;  // MPLX_OPEN_IS_GOAL

template <int D>
__global__ __launch_bounds__(kWave) void reserve_park_kernel(const ParkArgs P) {
  const ReserveArgs &A = P.res;
  const int lane = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kWave + lane;
  int64_t n = *P.f_count;
  n = n < P.n_max ? n : P.n_max;
  n = n < P.f_cap ? n : P.f_cap;
  int64_t n_nodes = *P.t_n_nodes;
  n_nodes = n_nodes < 0 ? 0 : (n_nodes < A.node_cap ? n_nodes : A.node_cap);
  constexpr int F = 4 * D + 2;

  // ---- this lane's row
  const bool walked = r < n;
  int32_t id = -1, q = 0;
  bool look = false;
  if (walked) {
    id = P.f_id[r];
    if (id >= 0 && (int64_t)id < n_nodes) {
      look = (P.flags[id] & kIsGoalBit) != 0;
      if (look && A.node_query) q = A.node_query[id];
      if (q < 0 || q >= A.Q) {
        look = false;
        q = 0;
      }
    }
  }
  long long my_hit = -1;
  unsigned long long todo = __ballot(look);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    // ---- the row (wave-uniform: every lane reads the owner's row)
    const int64_t ro = (int64_t)blockIdx.x * kWave + owner;
    const int32_t qo = __shfl(q, owner);
    const double t0 = A.q_t0[qo], rq = A.q_r[qo];
    const int32_t ign = A.q_ignore[qo];
    double p[D];
#pragma unroll
    for (int d = 0; d < D; d++) p[d] = P.f_state[(int64_t)d * P.f_stride + ro];
    const double tn = P.f_state[(int64_t)(F - 1) * P.f_stride + ro];
    // the first instant with tl_i >= tn; n_steps: none (a NaN or a t past the horizon)
    int i_first = A.n_steps;
    {
      const double x = (tn + t0) / A.step;
      int64_t g = 0;  // (a NaN goes to 0)
      if (x >= 1.0) g = x < 2147483647.0 ? (int64_t)x - 1 : (int64_t)A.n_steps;
      for (int s = 0; s < P.n_scan; s++) {
        const int64_t i = g + s;
        if (i >= A.n_steps) break;
        if ((double)i * A.step - t0 >= tn) {
          i_first = (int)i;
          break;
        }
      }
    }
    double rrk[kParkKeep];
#pragma unroll
    for (int j = 0; j < kParkKeep; j++) {
      const int64_t b = (int64_t)j * kWave + lane;
      rrk[j] = NAN;
      if (b < A.B && A.incl[b] != 0 && A.group[b] != ign) rrk[j] = rq + A.r[b];
    }
    long long key = kNoHit;
    for (int i = i_first; i < A.n_steps && key == kNoHit; i += kParkInst) {
      long long mine = kNoHit;
      int j = 0;
      for (int64_t b = lane; b < A.B; b += kWave, j++) {
        double rr;
        if (j < kParkKeep) {
          rr = j == 0 ? rrk[0] : j == 1 ? rrk[1] : j == 2 ? rrk[2] : rrk[3];
        } else {
          rr = (A.incl[b] != 0 && A.group[b] != ign) ? rq + A.r[b] : NAN;
        }
        const double rr2 = rr * rr;
        // kParkInst instants at once, without a branch that depends on a load: their reads are in flight together
#pragma unroll
        for (int u = 0; u < kParkInst; u++) {
          const int iu = i + u;
          if (iu < A.n_steps) {  // (wave-uniform)
            const int64_t at = (int64_t)iu * A.B + b;
            const bool on = A.act[at] != 0;
            const double dx = p[0] - A.pos[at], dy = p[1] - A.pos[(int64_t)A.n_steps * A.B + at];
            double d2 = (dx * dx) + dy * dy;
            if (D == 3) {
              const double dz = p[D - 1] - A.pos[(int64_t)(D - 1) * A.n_steps * A.B + at];
              d2 = d2 + dz * dz;
            }
            const long long cand = ((long long)iu << 32) | (long long)b;
            if (on && d2 < rr2 && cand < mine) mine = cand;  // (a NaN on either side compares false)
          }
        }
      }
      // instants and reservations both ascend in the key: the minimum over the block is the row's smallest
      if (__ballot(mine != kNoHit) != 0ull) {
        for (int m = 1; m < kWave; m <<= 1) {
          const long long o = __shfl_xor(mine, m);
          mine = o < mine ? o : mine;
        }
        key = mine;
      }
    }
    if (lane == owner && key != kNoHit) {
      my_hit = key;
      P.flags[id] = (uint8_t)(P.flags[id] & ~kIsGoalBit);
    }
  }
  if (walked && P.hit) P.hit[r] = my_hit;
  const unsigned long long vetoed = __ballot(my_hit != -1);
  if (P.n_vetoed && lane == 0 && vetoed) atomicAdd(P.n_vetoed, (unsigned long long)__popcll(vetoed));
}

}  // namespace

hipError_t launch_reserve_park(int dim, const ParkArgs &a, int64_t rows, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int64_t blocks = (rows + kWave - 1) / kWave;
  if (blocks > 0x7fffffffLL || a.n_scan < 1) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kWave);
  if (dim == 2) hipLaunchKernelGGL((reserve_park_kernel<2>), grid, block, 0, s, a);
  else if (dim == 3) hipLaunchKernelGGL((reserve_park_kernel<3>), grid, block, 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

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
