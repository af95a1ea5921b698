// ray_kernel.hip -- MapUtil<Dim>::rayTrace for gfx950 (MI355X) on the int8 map the context holds, and the ray trace
// of env_map::is_goal over successor lists (include/mplx_ray.h).
//
// The cell of step n depends on (p1, p2, n) alone, so G consecutive lanes of a wavefront own ONE ray and take G steps
// of it per round (64 / G rays per wave, G in {4, 16, 64}): round r gives lane l of the group the step
// n = r G + 1 + l.  Every lane computes its cell with the reference's arithmetic (map_util.h:117-134, :103-108;
// -ffp-contract=off, true divisions, one multiply and one add per coordinate) and, when the cell is inside, loads its
// map byte: the G loads of a round are independent, where one lane per ray would wait for one load per step.  What
// couples the steps -- the stop at the first outside cell and the de-duplication against the cell of step n - 1 --
// is done with ballots cut down to the group's lanes: the first outside step truncates the round, the "new" bit
// compares with the neighbouring lane's cell (lane 0: the last cell of the previous round), popcounts give n_cells and
// the position of every emitted cell (a group's stores are contiguous), the lowest bit of new & occupied the first
// hit.  A group leaves when it met an outside step or ran out of steps, a wave when all its groups have.
//
// The goal pass scans the flag bytes of the lists (one byte per slot), appends the list indices of the candidates
// (emitted, bit 0 set) to a worklist with one atomic per wave, and a second launch traces the candidates in a
// grid-stride loop over a count that never leaves the device; it stops a ray at its first hit.  State rows of slots
// without bit 0 are never read.
#include "mplx_internal.h"

#include <math.h>

namespace mplx {
namespace {

constexpr int kBlock = 256;

struct RayResult {
  int n_cells;    // emitted cells (up to the first hit when STOP_AT_HIT)
  int first_hit;  // getIndex of the first occupied emitted cell, or -1
  bool left;      // met an outside step
  bool bad;       // non-finite coordinate or linf / 0.8 >= 2^31: nothing traced
};

// One ray per group of G lanes; all 64 lanes of the wave call this together (have = the group owns a ray; p1 / p2
// are the same in every lane of a group).  cells_row: where the ray's emitted cells go (first cell_cap of them), or
// null.
template <int D, int G, bool STOP_AT_HIT>
__device__ __forceinline__ RayResult trace_group(const RayArgs &A, bool have, const double (&p1)[D], const double (&p2)[D],
                                                 int32_t *cells_row, int32_t cell_cap) {
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1), gbase = lane & ~(G - 1);
  const uint64_t group_bits = G == 64 ? ~0ull : ((1ull << G) - 1);
  const uint64_t below_me = (1ull << gl) - 1;
  const int32_t mdim[3] = {A.dim0, A.dim1, A.dim2};
  const double org[3] = {A.org0, A.org1, A.org2};

  double diff[D], step[D], linf = 0.0;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < D; i++) {
    finite = finite && isfinite(p1[i]) && isfinite(p2[i]);
    diff[i] = p2[i] - p1[i];
    const double q = fabs(diff[i] / A.res);
    linf = q > linf ? q : linf;
  }
  const double md = linf / 0.8;
  RayResult R;
  R.bad = have && !(finite && md < 2147483648.0);
  const int max_diff = (have && !R.bad) ? (int)md : 0;
  const double s = 1.0 / (double)max_diff;
#pragma unroll
  for (int i = 0; i < D; i++) step[i] = diff[i] * s;

  R.n_cells = 0;
  R.first_hit = -1;
  R.left = false;
  int carry = -1;          // the cell of the last step of the previous round (the reference's prev_pn: none is outside)
  int64_t n = 1 + gl;      // this lane's step of the round
  bool done = max_diff <= 1;
  while (__ballot(!done) != 0ull) {
    const bool has = !done && n < (int64_t)max_diff;
    bool inside = has;
    int idx = 0, mul = 1;
#pragma unroll
    for (int i = 0; i < D; i++) {
      const double pt = p1[i] + step[i] * (double)n;
      const double c = round((pt - org[i]) / A.res - 0.5);
      const bool in = c >= 0.0 && c < (double)mdim[i];  // compared as a double: NaN and huge values are outside
      inside = inside && in;
      idx += (in ? (int)c : 0) * mul;
      mul *= mdim[i];
    }
    int8_t v = 0;
    if (inside) v = A.map[idx];
    const uint64_t out_b = (__ballot(has && !inside) >> gbase) & group_bits;
    const int first_out = out_b ? __builtin_ctzll(out_b) : G;
    const bool valid = has && gl < first_out;
    int prev = __shfl_up(idx, 1);
    if (gl == 0) prev = carry;
    const bool fresh = valid && idx != prev;
    const uint64_t new_b = (__ballot(fresh) >> gbase) & group_bits;
    const uint64_t hit_b = (__ballot(fresh && v == 100) >> gbase) & group_bits;
    if (cells_row && fresh) {
      const int pos = R.n_cells + __popcll(new_b & below_me);
      if (pos < cell_cap) cells_row[pos] = idx;
    }
    const int hit_idx = __shfl(idx, gbase + (hit_b ? __builtin_ctzll(hit_b) : 0));
    if (hit_b && R.first_hit < 0) {
      R.first_hit = hit_idx;
      // (the cells up to the hit; the goal pass reads neither the list nor the count)
      if (STOP_AT_HIT) done = true;
    }
    R.n_cells += __popcll(new_b);
    carry = __shfl(idx, gbase + G - 1);
    if (first_out < G) {
      R.left = true;
      done = true;
    }
    n += G;
    if (n - gl >= (int64_t)max_diff) done = true;  // the next round's first step is past the last one
  }
  return R;
}

template <int D, int G>
__global__ __launch_bounds__(kBlock) void ray_kernel(const RayArgs A) {
  constexpr int kRays = kBlock / G;
  const int64_t ray = (int64_t)blockIdx.x * kRays + threadIdx.x / G;
  const bool have = ray < A.n;
  double p1[D], p2[D];
#pragma unroll
  for (int i = 0; i < D; i++) {
    p1[i] = have ? A.p1[(int64_t)i * A.stride + ray] : 0.0;
    p2[i] = !have ? 0.0 : A.p2_stride == 0 ? A.p2[i] : A.p2[(int64_t)i * A.p2_stride + ray];
  }
  int32_t *row = (have && A.cells) ? A.cells + ray * A.cell_cap : nullptr;
  const RayResult R = trace_group<D, G, false>(A, have, p1, p2, row, A.cell_cap);
  if (!have || (threadIdx.x & (G - 1)) != 0) return;
  A.status[ray] = (uint8_t)((R.left ? 1 : 0) | (R.first_hit >= 0 ? 2 : 0) | (R.bad ? 4 : 0) |
                            ((A.cells && R.n_cells > A.cell_cap) ? 8 : 0));
  if (A.n_cells) A.n_cells[ray] = R.n_cells;
  if (A.first_hit) A.first_hit[ray] = R.first_hit;
}

// Candidates of the goal pass: emitted slots with bit 0.  The flag row is read 16 bytes per lane (1 KiB per wave
// instruction) from its first 16-byte boundary on; a wave whose 1 024 slots hold no bit 0 goes on at once, and count[]
// is read only for slots with the bit.  The bytes before the boundary and after the last full vector (fewer than 32)
// are one wave's work.  Candidates are appended with one atomic per wave and ballot.
__device__ __forceinline__ void push_candidates(const GoalSightArgs &A, bool bit0, int64_t i, int lane) {
  bool cand = false;
  if (bit0) {
    const int64_t k = i / A.nstride;
    cand = i - k * A.nstride < (int64_t)A.count[k];
  }
  const uint64_t b = __ballot(cand);
  if (b == 0ull) return;
  const int leader = __builtin_ctzll(b);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(A.work_count, (uint32_t)__popcll(b));
  base = (uint32_t)__shfl((int)base, leader);
  if (cand) A.work[base + (uint32_t)__popcll(b & ((1ull << lane) - 1))] = (int32_t)i;
}

__global__ __launch_bounds__(kBlock) void goal_scan_kernel(const GoalSightArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t total = A.n_nodes * A.nstride, stride = (int64_t)gridDim.x * kBlock;
  int64_t head = (int64_t)((16 - ((uintptr_t)A.flags & 15)) & 15);
  if (head > total) head = total;
  const int64_t n_vec = (total - head) >> 4;
  const uint4 *vec = (const uint4 *)(A.flags + head);
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j - lane < n_vec; j += stride) {
    uint4 w = make_uint4(0, 0, 0, 0);
    if (j < n_vec) w = vec[j];
    const uint32_t bits[4] = {w.x & 0x01010101u, w.y & 0x01010101u, w.z & 0x01010101u, w.w & 0x01010101u};
    if (__ballot((bits[0] | bits[1] | bits[2] | bits[3]) != 0u) == 0ull) continue;
#pragma unroll
    for (int b = 0; b < 16; b++)
      push_candidates(A, ((bits[b >> 2] >> (8 * (b & 3))) & 1u) != 0u, head + (j << 4) + b, lane);
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const int64_t tail = head + (n_vec << 4);  // lanes [0, head): the first bytes; the next total - tail lanes: the last
    const int64_t i = lane < head ? (int64_t)lane : tail + (lane - head);
    const bool mine = lane < head + (total - tail);
    push_candidates(A, mine && (A.flags[mine ? i : 0] & 1) != 0, i, lane);
  }
}

// ROWS: the goal per list entry, goals[row_query[i]] (the open set of a table with several queries)
template <int D, int G, bool ROWS>
__global__ __launch_bounds__(kBlock) void goal_trace_kernel(const GoalSightArgs A) {
  constexpr int kRays = kBlock / G;
  const int64_t m = (int64_t)*A.work_count, stride = (int64_t)gridDim.x * kRays;
  const int in_wave = (threadIdx.x & 63) / G;  // this group's place among the wave's
  for (int64_t w = (int64_t)blockIdx.x * kRays + threadIdx.x / G; w - in_wave < m; w += stride) {
    const bool have = w < m;
    const int64_t i = have ? (int64_t)A.work[w] : 0;
    double p1[D], p2[D];
    const PostFuse *goal = nullptr;
    if (ROWS && have) goal = A.goals + A.row_query[i];  // (a candidate: its row counted, its query is one)
#pragma unroll
    for (int d = 0; d < D; d++) {
      p1[d] = have ? A.state[(int64_t)d * A.sstride + i] : 0.0;
      p2[d] = ROWS ? (have ? goal->goal[d] : 0.0) : A.goal[d];
    }
    const RayResult R = trace_group<D, G, true>(A.ray, have, p1, p2, nullptr, 0);
    if (have && (threadIdx.x & (G - 1)) == 0 && R.first_hit >= 0) A.flags[i] = (uint8_t)(A.flags[i] | 8);
  }
}

template <int D, int G>
hipError_t launch_query(const RayArgs &a, hipStream_t s) {
  const int64_t blocks = (a.n + kBlock / G - 1) / (kBlock / G);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((ray_kernel<D, G>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <int D, int G>
hipError_t launch_goal(int n_cus, const GoalSightArgs &a, hipStream_t s) {
  const int64_t total = a.n_nodes * a.nstride;
  int64_t blocks = (total / 16 + kBlock - 1) / kBlock + 1;  // 16 slots per lane and pass
  const int64_t cap = (int64_t)n_cus * 8;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(goal_scan_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  if (hipError_t e = hipGetLastError()) return e;
  // at most one group per slot is ever needed; the loop bound is the device's count
  int64_t tblocks = (total + kBlock / G - 1) / (kBlock / G);
  if (tblocks > cap) tblocks = cap;
  if (a.goals) hipLaunchKernelGGL((goal_trace_kernel<D, G, true>), dim3((unsigned)tblocks), dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL((goal_trace_kernel<D, G, false>), dim3((unsigned)tblocks), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_ray_trace(int dim, int lanes, const RayArgs &a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (dim == 2) {
    if (lanes == 4) return launch_query<2, 4>(a, s);
    if (lanes == 16) return launch_query<2, 16>(a, s);
    if (lanes == 64) return launch_query<2, 64>(a, s);
  } else if (dim == 3) {
    if (lanes == 4) return launch_query<3, 4>(a, s);
    if (lanes == 16) return launch_query<3, 16>(a, s);
    if (lanes == 64) return launch_query<3, 64>(a, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_goal_sight(int dim, int lanes, int n_cus, const GoalSightArgs &a, hipStream_t s) {
  if (a.n_nodes * a.nstride == 0) return hipSuccess;
  if (dim == 2) {
    if (lanes == 4) return launch_goal<2, 4>(n_cus, a, s);
    if (lanes == 16) return launch_goal<2, 16>(n_cus, a, s);
    if (lanes == 64) return launch_goal<2, 64>(n_cus, a, s);
  } else if (dim == 3) {
    if (lanes == 4) return launch_goal<3, 4>(n_cus, a, s);
    if (lanes == 16) return launch_goal<3, 16>(n_cus, a, s);
    if (lanes == 64) return launch_goal<3, 64>(n_cus, a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace mplx
