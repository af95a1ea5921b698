// body_kernel.hip -- the ellipsoid body against a point cloud, for gfx950 (MI355X)
// (include/mplx_body.h states the semantics; tests/body_model.py restates them sequentially).
//
// The cloud's grid.  The included points (all coordinates finite) are binned into a uniform grid over their bounding
// box, on the device and without a host read: body_box_kernel reduces the box (per-wave minima and maxima of the
// coordinates' order-preserving integer images, then integer atomics), body_grid_kernel (one lane) derives the grid --
// cell edge edge0, doubled until the box needs at most kBodyMaxCells cells --, body_count_kernel counts per cell,
// body_scan_kernel (one workgroup) makes the exclusive scan and body_scatter_kernel moves the points into
// cell-contiguous rows pts[d][slot] with their original index idx[slot].  The order inside a cell is whatever the
// atomics give: every result is a minimum over keys that carry the original index.  Cell c = (z * dims[1] + y) *
// dims[0] + x, so the three x neighbours of a cell are ONE contiguous range of slots and a sample reads 3^(D-1) ranges.
// A box whose extent overflows falls back to one cell, which every sample visits.
//
// Why 3^D cells suffice (DESIGN.md 4.29 has the argument in full): dd <= RR bounds |p_d - c_d| by sqrt(RR) (1 + 2^-51) per
// axis; the edge is at least sqrt(RR) (1 + 1e-7); the computed quotients (x - origin) / edge carry at most 2^-30 of
// absolute error inside a grid of at most 2^22 cells per axis; so the floors differ by at most one.
//
// body_check_kernel<D, K>: one wave (a workgroup of 64 lanes) per list row, modelled on reserve_check_kernel.  The row's
// parent is wave-uniform.  The lanes are 2^sp_log2 entries x P = 64 >> sp_log2 slices: a lane holds its entry's segment
// in registers (traj::chain_segment with N = 1), evaluates centre and acceleration once per sample (traj::eval_segment,
// Command form) and, where the attitude is good, its slice strides over the slots of the sample's ranges.  After every
// sample the slices of an entry are folded with __shfl_xor; an entry that holds a key skips the later samples (keys
// ascend with the sample) and a sample at which no lane still looks ends the pass.  The point test orders its
// conjuncts dd <= RR first, so the three divisions run only for points in reach.
//
// body_poly_kernel<D, LAMBDA>: one wave per problem of a solved or loaded set; the lanes are 64 consecutive samples, each
// lane evaluates its own (the glue of traj_sample_kernel: scale::sample_tau, traj::find_segment, traj::eval_segment) and
// walks its ranges alone; samples ascend from block to block, so the first block with a key ends the problem and a wave
// minimum is its answer.
//
// Every output is a minimum or a sum of integers.  No workgroup waits for another, no LDS but the scan's, no scratch;
// every loop is bounded by S, n_samp (the poly kernel: total / step), the cell count or a cell's population.
#include "mplx_body_args.h"
#include "mplx_pair_device.h"
#include "mplx_scale_math.h"
#include "mplx_traj_device.h"

#include <math.h>

namespace mplx {
namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kScanBlock = 1024;
constexpr long long kNoHit = 0x7fffffffffffffffLL;
constexpr long long kBadAttitude = 0x7fffffffLL;
constexpr long long kMaxSample = 0x7ffffffeLL;

// ---------------------------------------------------------------------------------------------------- the grid
__device__ __forceinline__ unsigned long long ord_of(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double ord_back(unsigned long long u) {
  u = (u >> 63) ? (u & ~(1ull << 63)) : ~u;
  return __longlong_as_double((long long)u);
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  return (unsigned long long)__shfl_xor((long long)v, m);
}

template <int D>
__device__ __forceinline__ bool included(const double *p) {
  bool ok = true;
#pragma unroll
  for (int d = 0; d < D; d++) ok = ok && __builtin_isfinite(p[d]);
  return ok;
}

// the cell of an included point along one axis: floor((x - origin) / edge); x >= origin, and rounding is monotone, so
// the quotient never exceeds the one that made `dim` (the clamp is for the one-cell fallback, where nothing is divided)
__device__ __forceinline__ int cell_axis(double x, double o, double edge, int dim) {
  const double q = (x - o) / edge;
  return q >= 1.0 ? (q < (double)dim ? (int)q : dim - 1) : 0;
}

template <int D>
__device__ __forceinline__ int cell_of_point(const BodyGrid &G, const double *p) {
  if (G.n_cells == 1) return 0;
  int c = 0;
#pragma unroll
  for (int d = D - 1; d >= 0; d--) c = c * G.dims[d] + cell_axis(p[d], G.origin[d], G.edge, G.dims[d]);
  return c;
}

__global__ void body_box_init_kernel(BodyBox *B) {
  for (int d = 0; d < 3; d++) {
    B->lo[d] = ~0ull;
    B->hi[d] = 0ull;
  }
  B->n_incl = 0;
}

template <int D>
__global__ __launch_bounds__(kBlock) void body_box_kernel(const BodyBuildArgs A) {
  unsigned long long lo[D], hi[D];
#pragma unroll
  for (int d = 0; d < D; d++) {
    lo[d] = ~0ull;
    hi[d] = 0ull;
  }
  int cnt = 0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < A.n; p += stride) {
    double x[D];
#pragma unroll
    for (int d = 0; d < D; d++) x[d] = A.xyz[p * D + d];
    if (!included<D>(x)) continue;
    cnt++;
#pragma unroll
    for (int d = 0; d < D; d++) {
      const unsigned long long u = ord_of(x[d]);
      lo[d] = u < lo[d] ? u : lo[d];
      hi[d] = u > hi[d] ? u : hi[d];
    }
  }
  for (int m = 1; m < kWave; m <<= 1) {
#pragma unroll
    for (int d = 0; d < D; d++) {
      const unsigned long long a = shfl_xor_u64(lo[d], m), b = shfl_xor_u64(hi[d], m);
      lo[d] = a < lo[d] ? a : lo[d];
      hi[d] = b > hi[d] ? b : hi[d];
    }
    cnt += __shfl_xor(cnt, m);
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && cnt > 0) {
#pragma unroll
    for (int d = 0; d < D; d++) {
      atomicMin(&A.box->lo[d], lo[d]);
      atomicMax(&A.box->hi[d], hi[d]);
    }
    atomicAdd(&A.box->n_incl, cnt);
  }
}

template <int D>
__global__ void body_grid_kernel(const BodyBuildArgs A) {
  BodyGrid G;
  for (int d = 0; d < 3; d++) {
    G.origin[d] = 0.0;
    G.dims[d] = 1;
  }
  G.edge = A.edge0;
  G.n_cells = 1;
  G.n_incl = A.box->n_incl;
  G.pad = 0;
  if (G.n_incl > 0) {
    double ext[D];
    for (int d = 0; d < D; d++) {
      G.origin[d] = ord_back(A.box->lo[d]);
      ext[d] = ord_back(A.box->hi[d]) - G.origin[d];
    }
    double c = A.edge0;
    bool ok = false;
    int dims[D];
    for (int it = 0; it < 2200 && !ok; it++) {  // (2^2200 overflows every double: the loop ends with ok or with the fallback)
      ok = true;
      int64_t prod = 1;
      for (int d = 0; d < D && ok; d++) {
        const double q = ext[d] / c;
        if (!(q < (double)kBodyMaxCells)) {
          ok = false;
        } else {
          dims[d] = (int)q + 1;
          prod *= dims[d];
          ok = prod <= kBodyMaxCells;
        }
      }
      if (!ok) c = c * 2.0;
    }
    if (ok) {
      G.edge = c;
      G.n_cells = 1;
      for (int d = 0; d < D; d++) {
        G.dims[d] = dims[d];
        G.n_cells *= dims[d];
      }
    }
  }
  *A.grid = G;
}

__global__ __launch_bounds__(kBlock) void body_zero_kernel(const BodyBuildArgs A) {
  const int64_t n = (int64_t)A.grid->n_cells + 1, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) A.cell_start[i] = 0;
}

template <int D>
__global__ __launch_bounds__(kBlock) void body_count_kernel(const BodyBuildArgs A) {
  const BodyGrid G = *A.grid;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < A.n; p += stride) {
    double x[D];
#pragma unroll
    for (int d = 0; d < D; d++) x[d] = A.xyz[p * D + d];
    int c = -1;
    if (included<D>(x)) {
      c = cell_of_point<D>(G, x);
      atomicAdd(&A.cell_start[c + 1], 1);
    }
    A.cell_of_point[p] = c;
  }
}

// cell_start[1 ..] holds the counts; afterwards cell_start[c + 1] = the first slot of cell c (the scatter advances it to
// the first slot of cell c + 1, and cell_start[0] stays 0)
__global__ __launch_bounds__(kScanBlock) void body_scan_kernel(const BodyBuildArgs A) {
  __shared__ int s_sum[kScanBlock];
  const int n = A.grid->n_cells, t = threadIdx.x;
  int32_t *a = A.cell_start + 1;
  const int chunk = (n + kScanBlock - 1) / kScanBlock;
  const int lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  int sum = 0;
  for (int i = lo; i < hi; i++) sum += a[i];
  s_sum[t] = sum;
  __syncthreads();
  for (int m = 1; m < kScanBlock; m <<= 1) {
    const int v = t >= m ? s_sum[t - m] : 0;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  int run = s_sum[t] - sum;
  for (int i = lo; i < hi; i++) {
    const int v = a[i];
    a[i] = run;
    run += v;
  }
}

template <int D>
__global__ __launch_bounds__(kBlock) void body_scatter_kernel(const BodyBuildArgs A) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < A.n; p += stride) {
    const int c = A.cell_of_point[p];
    if (c < 0) continue;
    const int slot = atomicAdd(&A.cell_start[c + 1], 1);
#pragma unroll
    for (int d = 0; d < D; d++) A.pts[(int64_t)d * A.n + slot] = A.xyz[p * D + d];
    A.idx[slot] = (int32_t)p;
  }
}

// ---------------------------------------------------------------------------------------------------- the pair test
struct Attitude {
  double n[3], nn;
  bool bad;
};

template <int D>
__device__ __forceinline__ Attitude attitude_of(const BodyShape &sh, const double *acc) {
  Attitude t;
  t.n[0] = acc[0];
  t.n[1] = acc[1];
  t.n[2] = (D == 3 ? acc[D - 1] : 0.0) + sh.g;
  t.nn = (t.n[0] * t.n[0] + t.n[1] * t.n[1]) + t.n[2] * t.n[2];
  t.bad = !(t.n[2] > 0.0) || t.n[2] * t.n[2] < sh.mct2 * t.nn;
  return t;
}

template <int D>
__device__ __forceinline__ bool inside(const BodyShape &sh, const Attitude &t, const double *c, const double *p) {
  const double dx = p[0] - c[0], dy = p[1] - c[1], dz = D == 3 ? p[D - 1] - c[D - 1] : 0.0;
  const double dd = (dx * dx + dy * dy) + dz * dz;
  if (!(dd <= sh.RR)) return false;
  const double dn = (dx * t.n[0] + dy * t.n[1]) + dz * t.n[2];
  const double a2 = dn * dn / t.nn;
  const double perp2 = dd - a2;
  const double e = perp2 / sh.rr + a2 / sh.hh;
  return e <= 1.0;
}

// The smallest original index among the points inside at centre c, from the slots first, first + step, ... of the
// sample's ranges; 0x7fffffff without one.
template <int D>
__device__ __forceinline__ int32_t visit(const BodyShape &sh, const BodyCloud &C, const BodyGrid &G, const Attitude &t,
                                         const double *c, int first, int step) {
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (G.n_cells != 1) {
#pragma unroll
    for (int d = 0; d < D; d++) {
      const double q = (c[d] - G.origin[d]) / G.edge;
      if (!(q >= -1.0) || !(q < (double)G.dims[d] + 1.0)) return 0x7fffffff;  // (a NaN too)
      int f = (int)q;
      if ((double)f > q) f--;
      lo[d] = f - 1 > 0 ? f - 1 : 0;
      hi[d] = f + 1 < G.dims[d] - 1 ? f + 1 : G.dims[d] - 1;
    }
  }
  int32_t best = 0x7fffffff;
  for (int z = lo[2]; z <= hi[2]; z++) {
    for (int y = lo[1]; y <= hi[1]; y++) {
      const int64_t base = ((int64_t)z * G.dims[1] + y) * G.dims[0];
      const int b = C.cell_start[base + lo[0]], e = C.cell_start[base + hi[0] + 1];
      for (int s = b + first; s < e; s += step) {
        double p[D];
#pragma unroll
        for (int d = 0; d < D; d++) p[d] = C.pts[(int64_t)d * C.n + s];
        if (inside<D>(sh, t, c, p)) {
          const int32_t id = C.idx[s];
          best = id < best ? id : best;
        }
      }
    }
  }
  return best;
}

// ---------------------------------------------------------------------------------------------------- the list check
template <int D, int K>
__global__ __launch_bounds__(kWave) void body_check_kernel(const BodyCheckArgs A) {
  const int64_t k = blockIdx.x;
  const int lane = threadIdx.x;
  const int SP = 1 << A.sp_log2, P = kWave >> A.sp_log2;
  const int jl = lane & (SP - 1), slice = lane >> A.sp_log2;
  const int64_t S = A.S;
  const BodyGrid G = *A.cloud.grid;

  // ---- the row (wave-uniform)
  const int32_t pid = A.parent_id[k];
  const int cnt = A.count[k];
  const bool row_ok = pid >= 0;
  double ps[4 * D];
#pragma unroll
  for (int f = 0; f < 4 * D; f++) ps[f] = A.parent_state[(int64_t)f * A.parent_stride + k];

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
    for (int i = 0; i <= A.n_samp; i++) {
      if (__ballot(looked && key == kNoHit) == 0ull) break;  // nobody looks for a key any more
      const double s = i < A.n_samp ? (double)i * A.ds : A.dt;
      traj::Sample<D> sm;
      traj::eval_segment<D, true, true>(seg, 1, s, sm);
      if (looked && key == kNoHit) {
        const Attitude t = attitude_of<D>(A.shape, sm.acc);
        if (t.bad) {
          key = ((long long)i << 32) | kBadAttitude;
        } else {
          const int32_t id = visit<D>(A.shape, A.cloud, G, t, sm.pos, slice, P);
          if (id != 0x7fffffff) key = ((long long)i << 32) | (long long)id;
        }
      }
      // the slices of an entry: the smallest key of the sample
      for (int m = SP; m < kWave; m <<= 1) {
        const long long o = __shfl_xor(key, m);
        key = o < key ? o : key;
      }
    }
    const bool blocked = looked && key != kNoHit;
    if (mine && slice == 0) {
      if (A.hit) A.hit[e] = blocked ? key : -1LL;
      if (blocked) A.cost[e] = INFINITY;
    }
    blocked_row += (unsigned int)__popcll(__ballot(blocked && slice == 0));
  }
  if (A.n_blocked && lane == 0 && blocked_row) atomicAdd(A.n_blocked, (unsigned long long)blocked_row);
}

template <int D>
hipError_t check_dim(int order, const BodyCheckArgs &a, hipStream_t s) {
  const dim3 grid((unsigned)a.n_rows), block(kWave);
  switch (order) {
    case 1: hipLaunchKernelGGL((body_check_kernel<D, 1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((body_check_kernel<D, 2>), grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL((body_check_kernel<D, 3>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((body_check_kernel<D, 4>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- the set check
template <int D, bool LAMBDA>
__global__ __launch_bounds__(kWave) void body_poly_kernel(const BodyPolyArgs P) {
  const TrajArgs &R = P.traj;
  const int64_t k = blockIdx.x, N = P.K;
  const int lane = threadIdx.x;
  const BodyGrid G = *P.cloud.grid;

  // ---- the problem (wave-uniform)
  const uint8_t st = R.tab_status[k];
  const int S = R.tab_S[k];
  long long out = -1;
  if (S > 0 && st == 0) {
    const double T = R.tab_T[k];
    const int nl = LAMBDA ? R.lam_n[k] : 0;
    const double total = nl > 0 ? R.lam_total[k] : T;
    long long key = kNoHit;
    for (int64_t ib = 0; ib <= kMaxSample; ib += kWave) {
      const int64_t il = ib + lane;
      const double tl = (double)il * P.step;
      const bool in = il < kMaxSample && tl <= total;
      const int nv = __popcll(__ballot(in));  // (tl is monotone: the samples i * step of the block are its first nv lanes)
      const bool last = lane == nv;           // the sample at `total`, one past the largest i
      long long mine = kNoHit;
      if (in || last) {
        const double time = in ? tl : total;
        traj::Sample<D> sm;
        if (!isfinite(time)) {
#pragma unroll
          for (int d = 0; d < D; d++) sm.pos[d] = sm.acc[d] = NAN;
        } else {
          // traj_sample_kernel, Command form, on a solved set
          double tau = time, lambda = 1.0, lambda_dot = 0.0;
          if (nl > 0) {
            const scale::TableLoader ld{R.lam_seg + k, N};
            double raw;
            bool found;
            tau = scale::sample_tau(ld, nl, R.lam == 2, time, R.lam_total[k], T, &raw, &found, &lambda, &lambda_dot);
          } else {
            if (tau < 0) tau = 0;
            if (tau > T) tau = T;
          }
          const double *taus = R.tab_tau + k;
          const int id = traj::find_segment<true, true>(taus, N, S, tau, R.env.dt);
          tau -= taus[(int64_t)id * N];
          traj::eval_segment<D, true, true, true>(R.tab_seg + (int64_t)id * (6 * D + 2) * N + k, N, tau, sm, lambda, lambda_dot);
        }
        const Attitude t = attitude_of<D>(P.shape, sm.acc);
        if (t.bad) {
          mine = (il << 32) | kBadAttitude;
        } else {
          const int32_t id = visit<D>(P.shape, P.cloud, G, t, sm.pos, 0, 1);
          if (id != 0x7fffffff) mine = (il << 32) | (long long)id;
        }
      }
      // samples ascend from block to block: the minimum over the block is the problem's smallest
      if (__ballot(mine != kNoHit) != 0ull) {
        for (int m = 1; m < kWave; m <<= 1) {
          const long long o = __shfl_xor(mine, m);
          mine = o < mine ? o : mine;
        }
        key = mine;
        break;
      }
      if (nv < kWave) break;  // the last sample lay in this block
    }
    if (key != kNoHit) out = key;
  }
  if (lane == 0) {
    if (P.hit) P.hit[k] = out;
    if (P.status) P.status[k] = st;
    if (P.n_hit && out != -1) atomicAdd(P.n_hit, 1ull);
  }
}

int blocks_of(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

template <int D>
hipError_t build_dim(const BodyBuildArgs &a, hipStream_t s) {
  const dim3 pts(blocks_of(a.n)), block(kBlock);
  hipLaunchKernelGGL(body_box_init_kernel, dim3(1), dim3(1), 0, s, a.box);
  hipLaunchKernelGGL((body_box_kernel<D>), pts, block, 0, s, a);
  hipLaunchKernelGGL((body_grid_kernel<D>), dim3(1), dim3(1), 0, s, a);
  hipLaunchKernelGGL(body_zero_kernel, dim3(blocks_of((int64_t)kBodyMaxCells / 16)), block, 0, s, a);
  hipLaunchKernelGGL((body_count_kernel<D>), pts, block, 0, s, a);
  hipLaunchKernelGGL(body_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, a);
  hipLaunchKernelGGL((body_scatter_kernel<D>), pts, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_body_build(int dim, const BodyBuildArgs &a, hipStream_t s) {
  if (a.n < 0 || a.n > 0x7ffffffeLL) return hipErrorInvalidValue;
  if (dim == 2) return build_dim<2>(a, s);
  if (dim == 3) return build_dim<3>(a, s);
  return hipErrorInvalidValue;
}

hipError_t launch_body_check(int dim, int control, const BodyCheckArgs &a, hipStream_t s) {
  if (a.n_rows <= 0) return hipSuccess;
  if (a.n_rows > 0x7fffffffLL || a.sp_log2 < 0 || a.sp_log2 > 6 || a.n_samp < 1) return hipErrorInvalidValue;
  const int ctl = control & 0x0f;
  const int order = ctl == 0x01 ? 1 : ctl == 0x03 ? 2 : ctl == 0x07 ? 3 : ctl == 0x0f ? 4 : 0;
  if (dim == 2) return check_dim<2>(order, a, s);
  if (dim == 3) return check_dim<3>(order, a, s);
  return hipErrorInvalidValue;
}

hipError_t launch_body_check_poly(int dim, const BodyPolyArgs &a, hipStream_t s) {
  if (a.K <= 0) return hipSuccess;
  if (a.K > 0x7fffffffLL || !a.traj.poly) return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.K), block(kWave);
  if (dim == 2) {
    if (a.traj.lam) hipLaunchKernelGGL((body_poly_kernel<2, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((body_poly_kernel<2, false>), grid, block, 0, s, a);
  } else if (dim == 3) {
    if (a.traj.lam) hipLaunchKernelGGL((body_poly_kernel<3, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((body_poly_kernel<3, false>), grid, block, 0, s, a);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace mplx
