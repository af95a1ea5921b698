// field_kernel.hip -- goal distance fields (include/mplx_field.h): dist[f][c] = the length of the shortest chain of
// traversable cells from c to a seed cell of field f, 8 / 26 neighbours, -1 where there is none.
//
// Tiled chaotic relaxation, not a level-synchronous BFS (which costs a launch per level, thousands of them on a long
// map).  One workgroup takes one (field, tile) -- 32 x 32 cells in 2-D, 8 x 8 x 8 in 3-D -- and leaves at once unless
// the tile's byte in the active map of this pass is set.  An active tile
//   1. stages its dist with a one-cell halo in LDS (34 x 34 or 10 x 10 x 10 words); the blocked bit of a cell (the
//      context's map, or with a potential map the field's own: field_pot_bits_kernel) stays in a register of its lane
//   2. relaxes in LDS, d = min(d, 1 + min over the neighbours) on traversable cells, until an iteration changes nothing;
//      the loop is bounded by the tile's cell count (an iteration that changes something fixes one more cell for good)
//   3. writes back the cells that fell
//   4. where a cell on the tile's border fell, sets the byte of the neighbouring tile in the active map of the NEXT pass
//      (plain stores of 1; the two maps alternate) and counts the tile once in a counter the host reads after the pass
// The host stops at the first pass that adds nothing to the counter.
//
// The table's discipline holds: a launch boundary is the only ordering between passes, no
// workgroup waits for another, nothing spins.  Values only fall and every stored value is the length of a real chain, so
// a halo read that races with the neighbour's write-back (aligned 32-bit loads and stores, never torn) sees a valid upper
// bound; the neighbour then marks this tile for the next pass, and the fixed point is the one the header states whatever
// the order of work.  -1 is kept as it is and compared unsigned: it is the largest value, "no chain yet".
#include "mplx_internal.h"

namespace mplx {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNone = 0xffffffffu;  // -1

// With a potential map installed the context's blocked bits are a pre-screen of the expansion, not its blocking rule: they
// are set for every cell that blocks OR costs (value > 0).  A primitive ends only at a value >= 100 (env_map.h:113-118);
// values 1 .. 99 are crossed at an added cost.  A field over the pre-screen would call a cost cell a wall and overestimate,
// so for such a context the field has bits of its own: value >= 100, or outside the search region, or past the last cell.
__global__ __launch_bounds__(kBlock) void field_pot_bits_kernel(const int8_t *pot, const uint32_t *region, int64_t n_cells, int64_t n_words,
                                                                uint32_t *out) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n_words) return;
  const uint32_t reg = region ? region[g] : 0xffffffffu;
  uint32_t bits = 0;
  for (int b = 0; b < 32; b++) {
    const int64_t idx = g * 32 + b;
    const bool blocked = idx >= n_cells || pot[idx] >= 100 || !((reg >> b) & 1u);
    bits |= (blocked ? 1u : 0u) << b;
  }
  out[g] = bits;
}

__global__ __launch_bounds__(kBlock) void field_init_kernel(const FieldArgs A) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= (int64_t)A.F * A.n_cells) return;
  const int32_t f = (int32_t)(g / A.n_cells);
  const int64_t c = g - (int64_t)f * A.n_cells;
  int32_t x[3];
  x[0] = (int32_t)(c % A.mdim[0]);
  x[1] = (int32_t)((c / A.mdim[0]) % A.mdim[1]);
  x[2] = (int32_t)(c / ((int64_t)A.mdim[0] * A.mdim[1]));
  const int32_t *b = A.box + (int64_t)f * 6;
  bool seed = true;
  for (int i = 0; i < 3; i++) seed = seed && x[i] >= b[i] && x[i] <= b[3 + i];
  A.dist[g] = seed ? 0 : -1;
  if (!seed) return;
  // the seed's tile and its neighbours start active: the neighbours see the seed in their halo
  const int ts = A.dim == 2 ? kFieldTile2 : kFieldTile3;
  const int32_t t0 = x[0] / ts, t1 = x[1] / ts, t2 = A.dim == 2 ? 0 : x[2] / ts;
  for (int dz = -1; dz <= 1; dz++)
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int32_t u0 = t0 + dx, u1 = t1 + dy, u2 = t2 + dz;
        if (u0 < 0 || u0 >= A.tiles[0] || u1 < 0 || u1 >= A.tiles[1] || u2 < 0 || u2 >= A.tiles[2]) continue;
        A.active_cur[(int64_t)f * A.n_tiles + ((int64_t)u2 * A.tiles[1] + u1) * A.tiles[0] + u0] = 1;
      }
}

template <int D>
__global__ __launch_bounds__(kBlock) void field_pass_kernel(const FieldArgs A) {
  constexpr int TS = D == 2 ? kFieldTile2 : kFieldTile3;
  constexpr int HS = TS + 2;
  constexpr int TZ = D == 2 ? 1 : TS, HZ = D == 2 ? 1 : HS;
  constexpr int CELLS = TS * TS * TZ, HALO = HS * HS * HZ, PER = CELLS / kBlock;
  __shared__ uint32_t s_d[HALO];
  __shared__ unsigned int s_mask, s_any;
  const int64_t ft = blockIdx.x;  // < F * n_tiles: the grid
  if (A.active_cur[ft] == 0) return;  // (uniform: only this workgroup writes the byte in this pass, and only behind the barrier)
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_mask = 0;
    s_any = 0;
  }
  __syncthreads();
  if (tid == 0) A.active_cur[ft] = 0;  // the map is all zero again when it becomes the next pass's `next`
  const int32_t f = (int32_t)(ft / A.n_tiles);
  const int64_t t = ft - (int64_t)f * A.n_tiles;
  const int32_t tx = (int32_t)(t % A.tiles[0]), ty = (int32_t)((t / A.tiles[0]) % A.tiles[1]), tz = (int32_t)(t / ((int64_t)A.tiles[0] * A.tiles[1]));
  const int32_t bx = tx * TS, by = ty * TS, bz = D == 2 ? 0 : tz * TS;
  int32_t *dist = A.dist + (int64_t)f * A.n_cells;
  // 1. the tile and its halo; a cell outside the map is "no chain"
  for (int h = tid; h < HALO; h += kBlock) {
    const int hx = h % HS, hy = (h / HS) % HS, hz = h / (HS * HS);
    const int32_t gx = bx + hx - 1, gy = by + hy - 1, gz = D == 2 ? 0 : bz + hz - 1;
    uint32_t v = kNone;
    if (gx >= 0 && gx < A.mdim[0] && gy >= 0 && gy < A.mdim[1] && gz >= 0 && gz < A.mdim[2])
      v = (uint32_t)dist[((int64_t)gz * A.mdim[1] + gy) * A.mdim[0] + gx];
    s_d[h] = v;
  }
  // this lane's cells: the index in the map, in the halo block, the value it was staged with, is it traversable
  int64_t cell[PER];
  int hid[PER];
  uint32_t d0[PER], d[PER];
  bool trav[PER];
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int k = tid + j * kBlock;
    const int lx = k % TS, ly = (k / TS) % TS, lz = k / (TS * TS);
    const int32_t gx = bx + lx, gy = by + ly, gz = bz + lz;
    hid[j] = ((D == 2 ? 0 : lz + 1) * HS + ly + 1) * HS + lx + 1;
    trav[j] = false;
    cell[j] = 0;
    if (gx < A.mdim[0] && gy < A.mdim[1] && gz < A.mdim[2]) {
      cell[j] = ((int64_t)gz * A.mdim[1] + gy) * A.mdim[0] + gx;
      trav[j] = ((A.blk[cell[j] >> 5] >> (cell[j] & 31)) & 1u) == 0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PER; j++) d0[j] = d[j] = s_d[hid[j]];
  // 2. relax until nothing changes.  Reads and writes of one iteration race on purpose: a value is a valid upper bound at
  // every moment, and an iteration in which no lane wrote read the final state.
  for (int it = 0; it < CELLS; it++) {
    int changed = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
      if (!trav[j]) continue;
      uint32_t m = kNone;
#pragma unroll
      for (int dz = (D == 2 ? 0 : -1); dz <= (D == 2 ? 0 : 1); dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
          for (int dx = -1; dx <= 1; dx++) {
            if (dx == 0 && dy == 0 && dz == 0) continue;
            const uint32_t v = s_d[hid[j] + (dz * HS + dy) * HS + dx];
            m = v < m ? v : m;
          }
      if (m != kNone && m + 1u < d[j]) {
        d[j] = m + 1u;
        s_d[hid[j]] = d[j];
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  // 3. the cells that fell; 4. the faces, edges and corners they lie on: bit (dx + 1) + 3 (dy + 1) + 9 (dz + 1)
  unsigned int mask = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    if (!(d[j] < d0[j])) continue;
    dist[cell[j]] = (int32_t)d[j];
    const int k = tid + j * kBlock;
    const int l[3] = {k % TS, (k / TS) % TS, k / (TS * TS)};
#pragma unroll
    for (int b = 0; b < (D == 2 ? 9 : 27); b++) {
      const int dd[3] = {b % 3 - 1, (b / 3) % 3 - 1, b / 9 - 1 + (D == 2 ? 1 : 0)};
      bool on = b != (D == 2 ? 4 : 13);
#pragma unroll
      for (int i = 0; i < D; i++) on = on && (dd[i] == 0 || l[i] == (dd[i] < 0 ? 0 : TS - 1));
      if (on) mask |= 1u << b;
    }
  }
  if (mask) atomicOr(&s_mask, mask);  // (LDS)
  __syncthreads();
  if (tid < (D == 2 ? 9 : 27) && ((s_mask >> tid) & 1u)) {
    const int32_t ux = tx + tid % 3 - 1, uy = ty + (tid / 3) % 3 - 1, uz = D == 2 ? 0 : tz + tid / 9 - 1;
    if (ux >= 0 && ux < A.tiles[0] && uy >= 0 && uy < A.tiles[1] && uz >= 0 && uz < A.tiles[2]) {
      A.active_next[(int64_t)f * A.n_tiles + ((int64_t)uz * A.tiles[1] + uy) * A.tiles[0] + ux] = 1;
      s_any = 1;
    }
  }
  __syncthreads();
  if (tid == 0 && s_any) atomicAdd(A.counter, 1ull);
}

}  // namespace

hipError_t launch_field_pot_bits(const int8_t *pot, const uint32_t *region, int64_t n_cells, uint32_t *out, hipStream_t s) {
  const int64_t n_words = (n_cells + 31) >> 5;
  if (n_words <= 0) return hipSuccess;
  hipLaunchKernelGGL(field_pot_bits_kernel, dim3((unsigned)((n_words + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, pot, region, n_cells, n_words, out);
  return hipGetLastError();
}

hipError_t launch_field_init(const FieldArgs &a, hipStream_t s) {
  const int64_t n = (int64_t)a.F * a.n_cells;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(field_init_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_field_pass(const FieldArgs &a, hipStream_t s) {
  const int64_t n = (int64_t)a.F * a.n_tiles;
  if (n <= 0) return hipSuccess;
  if (a.dim != 2 && a.dim != 3) return hipErrorInvalidValue;
  if (a.dim == 2) hipLaunchKernelGGL(field_pass_kernel<2>, dim3((unsigned)n), dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL(field_pass_kernel<3>, dim3((unsigned)n), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace mplx
