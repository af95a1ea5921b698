// conflict_kernel.hip -- conflicts between the K trajectories of one set on a common clock, for gfx950 (MI355X)
// (include/mplx_conflict.h states the semantics; tests/conflict_model.py restates them sequentially).
//
// conflict_init_kernel: one lane per trajectory: who is included, its radius, t0, group and rank in scratch, the two
// accumulators at their neutral values.  conflict_pairs_init_kernel: -1 into the K x K block of pair_first.
//
// Per chunk of instants, two launches:
// conflict_pos_kernel<D, POLY, LAMBDA>: one lane per (instant of the chunk, trajectory), consecutive lanes consecutive
//   trajectories: the segment rows and the stores are coalesced.  The position is what traj_sample_kernel writes in
//   Command form -- the same clamp, traj::find_segment / traj::eval_segment, scale::sample_tau under the Lambda's mode --,
//   the active bit is 1 (PARK) or tl >= 0 && tl <= total (GONE).
// conflict_pair_kernel<D>: a workgroup takes kTA trajectories a x kBlock trajectories b.  The a side of kSub instants is
//   staged in LDS and read at a wave-uniform address (a broadcast: no bank conflict); the b side is one trajectory per
//   lane, its position of the instant in registers.  Each lane keeps the first conflicting instant and the smallest d2
//   of its kTA pairs across the chunk in registers.  Only pairs a < b are looked at (workgroups wholly above the
//   diagonal leave at once): d2 and rr are symmetric, so the pair feeds both trajectories and both halves of
//   pair_first.  At the end of the chunk: for trajectory b the lane folds its pairs and issues at most one 64-bit
//   atomicMin per accumulator; for trajectory a the wave reduces over its lanes (__shfl_xor) and lane 0 issues it.
//   pair_first[a][b] has one owner per launch and launches are ordered on the stream: a plain read-min-write.
//
// conflict_final_kernel: unpacks the accumulators into the caller's rows.
//
// Every result is a minimum over (pair, instant) -- of (i << 32 | partner), of the bit pattern of d2 (non-negative
// doubles order like uint64), of i -- hence a pure function of the inputs whatever the tiling, the chunking or the order
// in which workgroups arrive.  A launch boundary is the only ordering; no workgroup waits for another; every loop is
// bounded by the chunk, kTA or S.
//
// Traffic per pair-instant: the b position of an instant (8 D + 1 bytes from L2 / HBM) serves kTA pairs, the staged a side
// serves kBlock: (8 D + 1) (1 / kTA + 1 / kBlock) bytes, 1.7 at D = 3; 8 D bytes of LDS broadcast per pair-instant per wave.
#include "mplx_internal.h"
#include "mplx_scale_math.h"
#include "mplx_traj_device.h"

#include <math.h>

namespace mplx {
namespace {

using traj::Sample;
using traj::eval_segment;
using traj::find_segment;

constexpr int kBlock = 256;
constexpr int kTA = 16;   // a-side trajectories of a workgroup: the pairs a lane keeps in registers
constexpr int kSub = 32;  // instants staged in LDS at a time
constexpr unsigned long long kNone = ~0ull;
constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;
constexpr int kNoStep = 0x7fffffff;

__global__ __launch_bounds__(kBlock) void conflict_init_kernel(const ConflictArgs C) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= C.K) return;
  const uint8_t st = C.traj.tab_status[k];
  const double t0 = C.t0 ? C.t0[k] : 0.0;
  const double r = C.radius ? C.radius[k] : C.radius_all;
  const bool bad = !isfinite(t0) || !(r >= 0.0) || !isfinite(r);
  C.m_incl[k] = (C.traj.tab_S[k] > 0 && st == 0 && !bad) ? 1 : 0;
  C.m_status[k] = (uint8_t)(st | (bad ? 128 : 0));  // MPLX_CONFLICT_BAD_INPUT
  C.m_r[k] = bad ? 0.0 : r;
  C.m_t0[k] = bad ? 0.0 : t0;
  C.m_group[k] = C.group ? C.group[k] : (int32_t)k;
  C.m_rank[k] = C.rank ? C.rank[k] : 0;
  C.acc_first[k] = kNone;
  C.acc_min[k] = kInfBits;
}

__global__ __launch_bounds__(kBlock) void conflict_pairs_init_kernel(const ConflictArgs C) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= C.K * C.K) return;
  const int64_t a = g / C.K, b = g - a * C.K;
  C.pair_first[a * C.pair_stride + b] = -1;
}

template <int D, bool POLY, bool LAMBDA>
__global__ __launch_bounds__(kBlock) void conflict_pos_kernel(const ConflictArgs C) {
  const TrajArgs &R = C.traj;
  const int64_t N = C.K;
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N * C.cn) return;
  const int64_t j = g / N, k = g - j * N;
  double *o = C.pos + j * N + k;
  const int64_t row = (int64_t)C.chunk * N;
  uint8_t active = 0;
  double p[D];
#pragma unroll
  for (int d = 0; d < D; d++) p[d] = 0.0;
  if (C.m_incl[k]) {
    const int S = R.tab_S[k];
    const double T = R.tab_T[k];
    const int nl = LAMBDA ? R.lam_n[k] : 0;
    const double ti = (double)(C.c0 + (int32_t)j) * C.step;
    const double time = ti - C.m_t0[k];
    const double total = nl > 0 ? R.lam_total[k] : T;
    active = C.gone ? ((time >= 0.0 && time <= total) ? 1 : 0) : 1;
    if (!isfinite(time)) {
#pragma unroll
      for (int d = 0; d < D; d++) p[d] = NAN;
    } else {
      // traj_sample_kernel, Command form
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
      const int id = find_segment<true, POLY>(taus, N, S, tau, R.env.dt);
      tau -= taus[(int64_t)id * N];
      Sample<D> sm;
      eval_segment<D, true, false, POLY>(R.tab_seg + (int64_t)id * ((POLY ? 6 : 5) * D + 2) * N + k, N, tau, sm);
#pragma unroll
      for (int d = 0; d < D; d++) p[d] = sm.pos[d];
    }
  }
#pragma unroll
  for (int d = 0; d < D; d++) o[(int64_t)d * row] = p[d];
  C.act[j * N + k] = active;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m);
    v = o < v ? o : v;
  }
  return v;
}

template <int D>
__global__ __launch_bounds__(kBlock) void conflict_pair_kernel(const ConflictArgs C) {
  const int64_t K = C.K;
  const int64_t a0 = (int64_t)blockIdx.x * kTA, b0 = (int64_t)blockIdx.y * kBlock;
  if (a0 >= b0 + kBlock - 1) return;  // no pair a < b in this tile (uniform: before any barrier)

  __shared__ double sa_pos[kSub * kTA * D];
  __shared__ double sa_r[kTA];
  __shared__ int32_t sa_group[kTA], sa_rank[kTA];
  __shared__ uint8_t sa_act[kSub * kTA];
  __shared__ uint8_t sa_incl[kTA];

  const int tid = threadIdx.x;
  if (tid < kTA) {
    const int64_t ka = a0 + tid;
    const bool have = ka < K;
    sa_incl[tid] = have ? C.m_incl[ka] : 0;
    sa_r[tid] = have ? C.m_r[ka] : 0.0;
    sa_group[tid] = have ? C.m_group[ka] : 0;
    sa_rank[tid] = have ? C.m_rank[ka] : 0;
  }
  const int64_t b = b0 + tid;
  const bool haveb = b < K;
  const int64_t bq = haveb ? b : 0;  // a lane past K reads trajectory 0 and uses nothing of it
  const bool bincl = haveb && C.m_incl[bq] != 0;
  const double rb = C.m_r[bq];
  const int32_t gb = C.m_group[bq], rkb = C.m_rank[bq];
  __syncthreads();

  uint32_t elig = 0;  // bit a: the pair (a0 + a, b) is looked at by this lane
#pragma unroll
  for (int a = 0; a < kTA; a++)
    if (bincl && a0 + a < b && sa_incl[a] && sa_group[a] != gb) elig |= 1u << a;

  int32_t first[kTA];
  double dmin[kTA];
#pragma unroll
  for (int a = 0; a < kTA; a++) {
    first[a] = kNoStep;
    dmin[a] = INFINITY;
  }

  const int64_t row = (int64_t)C.chunk * K;
  for (int sub = 0; sub < C.cn; sub += kSub) {
    const int ns = C.cn - sub < kSub ? C.cn - sub : kSub;
    __syncthreads();  // the previous pass has been read
    for (int idx = tid; idx < ns * kTA; idx += kBlock) {
      const int j = idx / kTA, a = idx - j * kTA;
      const int64_t ka = a0 + a;
      const bool have = ka < K;
      const int64_t at = (int64_t)(sub + j) * K + (have ? ka : 0);
#pragma unroll
      for (int d = 0; d < D; d++) sa_pos[idx * D + d] = have ? C.pos[(int64_t)d * row + at] : 0.0;
      sa_act[idx] = have ? C.act[at] : 0;
    }
    __syncthreads();
    for (int j = 0; j < ns; j++) {
      const int64_t at = (int64_t)(sub + j) * K + bq;
      double pb[D];
#pragma unroll
      for (int d = 0; d < D; d++) pb[d] = C.pos[(int64_t)d * row + at];
      const bool ab = C.act[at] != 0;
      const int32_t step = C.c0 + sub + j;
#pragma unroll
      for (int a = 0; a < kTA; a++) {
        const double *pa = sa_pos + (j * kTA + a) * D;  // wave-uniform
        double d2;
        {
          const double dx = pa[0] - pb[0], dy = pa[1] - pb[1];
          d2 = (dx * dx) + dy * dy;
          if (D == 3) {
            const double dz = pa[D - 1] - pb[D - 1];
            d2 = d2 + dz * dz;
          }
        }
        const double rr = sa_r[a] + rb;
        const bool ok = ((elig >> a) & 1u) && ab && sa_act[j * kTA + a] != 0;
        if (ok && d2 < dmin[a]) dmin[a] = d2;  // (a NaN is no candidate)
        if (ok && d2 < rr * rr && first[a] == kNoStep) first[a] = step;
      }
    }
  }

  // trajectory b: this lane's pairs charged to b (rank[a] <= rank[b])
  {
    unsigned long long key = kNone, bits = kInfBits;
#pragma unroll
    for (int a = 0; a < kTA; a++) {
      if (!((elig >> a) & 1u) || !(sa_rank[a] <= rkb)) continue;
      const unsigned long long mb = (unsigned long long)__double_as_longlong(dmin[a]);
      bits = mb < bits ? mb : bits;
      if (first[a] != kNoStep) {
        const unsigned long long ky = ((unsigned long long)(uint32_t)first[a] << 32) | (uint32_t)(a0 + a);
        key = ky < key ? ky : key;
      }
    }
    if (key != kNone) atomicMin(&C.acc_first[bq], key);
    // the accumulator only falls: a value read that is already no larger makes the atomic pointless
    if (bits < kInfBits && bits < __hip_atomic_load(&C.acc_min[bq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(&C.acc_min[bq], bits);
  }
  // trajectory a: the wave's pairs charged to a (rank[b] <= rank[a]), reduced over its lanes
  const int lane = tid & 63;
#pragma unroll
  for (int a = 0; a < kTA; a++) {
    const bool charged = ((elig >> a) & 1u) && rkb <= sa_rank[a];
    unsigned long long key = kNone, bits = kInfBits;
    if (charged) {
      bits = (unsigned long long)__double_as_longlong(dmin[a]);
      if (first[a] != kNoStep) key = ((unsigned long long)(uint32_t)first[a] << 32) | (uint32_t)b;
    }
    if (__ballot(key != kNone) != 0ull) {
      key = wave_min_u64(key);
      if (lane == 0) atomicMin(&C.acc_first[a0 + a], key);
    }
    if (__ballot(bits < kInfBits) != 0ull) {
      bits = wave_min_u64(bits);
      if (lane == 0 && bits < __hip_atomic_load(&C.acc_min[a0 + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&C.acc_min[a0 + a], bits);
    }
  }
  // the pair itself, regardless of rank: one owner per launch
  if (C.pair_first) {
#pragma unroll
    for (int a = 0; a < kTA; a++) {
      if (first[a] == kNoStep) continue;  // (set only for a pair this lane looks at: a0 + a < b < K)
      int32_t *p1 = C.pair_first + (a0 + a) * C.pair_stride + b, *p2 = C.pair_first + b * C.pair_stride + (a0 + a);
      const int32_t cur = *p1;
      const int32_t v = (cur < 0 || first[a] < cur) ? first[a] : cur;
      *p1 = v;
      *p2 = v;
    }
  }
}

__global__ __launch_bounds__(kBlock) void conflict_final_kernel(const ConflictArgs C) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= C.K) return;
  const bool incl = C.m_incl[k] != 0;
  const unsigned long long key = incl ? C.acc_first[k] : kNone, bits = incl ? C.acc_min[k] : kInfBits;
  if (C.first_step) C.first_step[k] = key == kNone ? -1 : (int32_t)(key >> 32);
  if (C.first_partner) C.first_partner[k] = key == kNone ? -1 : (int32_t)(key & 0xffffffffull);
  if (C.min_d2) C.min_d2[k] = __longlong_as_double((long long)bits);
  if (C.status) C.status[k] = C.m_status[k];
}

inline bool blocks_of(int64_t n, unsigned *out) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  if (b > 0x7fffffffLL) return false;
  *out = (unsigned)b;
  return true;
}

template <int D>
hipError_t chunk_dim(const ConflictArgs &a, hipStream_t s) {
  unsigned pb;
  if (!blocks_of(a.K * a.cn, &pb)) return hipErrorInvalidValue;
  const int64_t na = (a.K + kTA - 1) / kTA, nb = (a.K + kBlock - 1) / kBlock;
  if (na > 0x7fffffffLL || nb > 65535) return hipErrorInvalidValue;
  if (a.traj.poly && a.traj.lam)
    hipLaunchKernelGGL((conflict_pos_kernel<D, true, true>), dim3(pb), dim3(kBlock), 0, s, a);
  else if (a.traj.poly)
    hipLaunchKernelGGL((conflict_pos_kernel<D, true, false>), dim3(pb), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((conflict_pos_kernel<D, false, false>), dim3(pb), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL((conflict_pair_kernel<D>), dim3((unsigned)na, (unsigned)nb), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_conflict_init(const ConflictArgs &a, hipStream_t s) {
  if (a.K == 0) return hipSuccess;
  unsigned nb;
  if (!blocks_of(a.K, &nb)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(conflict_init_kernel, dim3(nb), dim3(kBlock), 0, s, a);
  if (a.pair_first) {
    if (a.K > 0x7fffffffLL || !blocks_of(a.K * a.K, &nb)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conflict_pairs_init_kernel, dim3(nb), dim3(kBlock), 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_conflict_chunk(int dim, const ConflictArgs &a, hipStream_t s) {
  if (a.K == 0 || a.cn == 0) return hipSuccess;
  if (dim == 2) return chunk_dim<2>(a, s);
  if (dim == 3) return chunk_dim<3>(a, s);
  return hipErrorInvalidValue;
}

hipError_t launch_conflict_positions(int dim, const ConflictArgs &a, hipStream_t s) {
  if (a.K == 0 || a.cn == 0) return hipSuccess;
  if (dim != 2 && dim != 3) return hipErrorInvalidValue;
  unsigned nb, pb;
  if (!blocks_of(a.K, &nb) || !blocks_of(a.K * a.cn, &pb)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(conflict_init_kernel, dim3(nb), dim3(kBlock), 0, s, a);
  const int v = (a.traj.poly && a.traj.lam) ? 2 : a.traj.poly ? 1 : 0;
  if (dim == 2) {
    if (v == 2) hipLaunchKernelGGL((conflict_pos_kernel<2, true, true>), dim3(pb), dim3(kBlock), 0, s, a);
    else if (v == 1) hipLaunchKernelGGL((conflict_pos_kernel<2, true, false>), dim3(pb), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((conflict_pos_kernel<2, false, false>), dim3(pb), dim3(kBlock), 0, s, a);
  } else {
    if (v == 2) hipLaunchKernelGGL((conflict_pos_kernel<3, true, true>), dim3(pb), dim3(kBlock), 0, s, a);
    else if (v == 1) hipLaunchKernelGGL((conflict_pos_kernel<3, true, false>), dim3(pb), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((conflict_pos_kernel<3, false, false>), dim3(pb), dim3(kBlock), 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_conflict_final(const ConflictArgs &a, hipStream_t s) {
  if (a.K == 0) return hipSuccess;
  unsigned nb;
  if (!blocks_of(a.K, &nb)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(conflict_final_kernel, dim3(nb), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace mplx
