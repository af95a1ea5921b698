// map_util_kernel.hip -- the MapUtil<Dim> calls a user makes on the map before planning
// (reference include/mpl_collision/map_util.h), on the device map:
//   dilate          :220-256   obstacle inflation by a list of cell offsets
//   freeUnknown     :258-276   -1 -> 0
//   freeAll         :278-296   (a memset on the host side)
//   getCloud / getFreeCloud / getUnknownCloud   :136-218   cells of one class as points
//
// dilate.  The reference copies the map and, for every cell occupied in the ORIGINAL
// map and every offset o with n + o inside, writes 100 into the copy: a scatter of
// occupied x |offsets| guarded byte writes.  As a gather,
//   out[m] = 100  if some o has m - o inside and map[m - o] == 100,  else map[m].
// Occupancy is packed into a bit plane first (one word = 32 cells of an x row, rows
// padded to whole words, padding bits zero).  A shift by (dy, dz) is then a row
// offset and a shift by dx a funnel shift of neighbouring words; a run of consecutive
// dx values [b - L + 1, b] (what boxes and balls are made of) is ONE 64-bit window of
// the source row OR-ed with itself at doubling distances: ceil(log2 L) shift-ORs per
// run instead of L.  Words outside the source row read as zero, so sources outside
// the map contribute nothing and no shift pulls bits from the next row.  The same
// thread then knows which of its 32 cells change (hit and not already 100) and
// touches the int8 map only there: the map is read once by the packing pass and
// written where it changes.
//
// clouds.  The reference returns the cells in its loop order, x outermost and z
// (2D: y) innermost -- the transpose of memory order.  One thread per (x, y) column
// (2D: per x) walks z, neighbouring threads on neighbouring x, so every step is a
// coalesced row read; a count pass, an exclusive scan of the column counts in key
// order x * d1 + y (launch_scan_counts), and a fill pass that writes each column's
// points from its scanned offset: the order comes from the scan, no atomics.
// Positions are intToFloat (:110-114): ((double)n + 0.5) * res + origin, two IEEE
// operations per axis (-ffp-contract=off, build.py).
#include "mplx_internal.h"

namespace mplx {
namespace {

constexpr int8_t kOcc = 100;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

// bit x % 32 of word x / 32 of row (y, z) = map[x + d0 * (y + d1 * z)] == 100
__global__ __launch_bounds__(256) void pack_occupancy_kernel(const int8_t *__restrict__ map, int64_t d0, int64_t words,
                                                             int64_t n_words, uint32_t *__restrict__ bits) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_words) return;
  const int64_t row = g / words;
  const int64_t x0 = (g - row * words) * 32;
  const int8_t *src = map + row * d0 + x0;
  uint32_t v = 0;
  if ((d0 & 15) == 0) {  // rows start on 16-byte boundaries: two 16-byte loads per word
    const uint4 *s4 = (const uint4 *)src;
    const int halves = (d0 - x0) >= 32 ? 2 : 1;  // d0 % 16 == 0: a row ends on a half word
    for (int h = 0; h < halves; h++) {
      const uint4 q = s4[h];
      const uint32_t part[4] = {q.x, q.y, q.z, q.w};
      for (int k = 0; k < 16; k++)
        if ((int8_t)(part[k >> 2] >> (8 * (k & 3))) == kOcc) v |= 1u << (16 * h + k);
    }
  } else {
    const int n = (int)((d0 - x0) < 32 ? (d0 - x0) : 32);
    for (int k = 0; k < n; k++)
      if (src[k] == kOcc) v |= 1u << k;
  }
  bits[g] = v;
}

// One offset run: the dx values [b - len + 1, b] of one (dy, dz), 1 <= len <= 33.
struct Run {
  int32_t dy, dz, b, len;
};

// One thread per word of the output bit plane: the OR over every run of the shifted source rows, then the cells that
// become 100 written into the map.
__global__ __launch_bounds__(256) void dilate_apply_kernel(const uint32_t *__restrict__ bits, const Run *__restrict__ runs,
                                                           int n_runs, int64_t d0, int64_t d1, int64_t d2, int64_t words,
                                                           int8_t *__restrict__ map) {
  const int64_t n_words = words * d1 * d2;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_words) return;
  const int64_t row = g / words;
  const int64_t w = g - row * words;
  const int64_t y = row % d1, z = row / d1;
  uint32_t hit = 0;
  for (int i = 0; i < n_runs; i++) {
    const Run R = runs[i];
    const int64_t ys = y - R.dy, zs = z - R.dz;
    if (ys < 0 || ys >= d1 || zs < 0 || zs >= d2) continue;  // the source row lies outside the map
    const uint32_t *src = bits + (zs * d1 + ys) * words;
    // window bit k = source bit p0 + k, p0 = 32 w - b; output bit j needs window bits j .. j + len - 1
    const int64_t p0 = 32 * w - R.b;
    const int r = (int)(p0 & 31);
    const int64_t q = (p0 - r) / 32;
    uint32_t s[3];
    for (int k = 0; k < 3; k++) s[k] = (q + k >= 0 && q + k < words) ? src[q + k] : 0u;
    uint64_t win = (uint64_t)s[0] | ((uint64_t)s[1] << 32);
    if (r) win = (win >> r) | ((uint64_t)s[2] << (64 - r));
    for (int cov = 1; cov < R.len;) {
      const int sh = cov < R.len - cov ? cov : R.len - cov;
      win |= win >> sh;
      cov += sh;
    }
    hit |= (uint32_t)win;
  }
  const int64_t x0 = 32 * w;
  if (d0 - x0 < 32) hit &= (1u << (d0 - x0)) - 1u;  // padding bits of the row's last word
  const uint32_t need = hit & ~bits[g];               // hit and not already 100
  if (!need) return;
  int8_t *dst = map + row * d0 + x0;
  if ((d0 & 15) == 0) {  // 16-byte read-modify-write where one of its cells changes
    uint4 *d4 = (uint4 *)dst;
    for (int h = 0; h < 2; h++) {
      const uint32_t m = (need >> (16 * h)) & 0xffffu;
      if (!m) continue;
      uint4 q = d4[h];
      uint32_t part[4] = {q.x, q.y, q.z, q.w};
      for (int k = 0; k < 16; k++)
        if ((m >> k) & 1u) part[k >> 2] = (part[k >> 2] & ~(0xffu << (8 * (k & 3)))) | ((uint32_t)(uint8_t)kOcc << (8 * (k & 3)));
      q.x = part[0]; q.y = part[1]; q.z = part[2]; q.w = part[3];
      d4[h] = q;
    }
  } else {
    for (int k = 0; k < 32; k++)
      if ((need >> k) & 1u) dst[k] = kOcc;
  }
}

// -1 -> 0 over the whole map, 16 cells per thread; a 16-byte vector with no unknown cell is not stored
__global__ __launch_bounds__(256) void free_unknown_kernel(int8_t *__restrict__ map, int64_t n_cells) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t c0 = g * 16;
  if (c0 >= n_cells) return;
  if (c0 + 16 <= n_cells) {
    uint4 *p = (uint4 *)(map + c0);
    uint4 q = *p;
    uint32_t part[4] = {q.x, q.y, q.z, q.w};
    bool changed = false;
    for (int k = 0; k < 16; k++) {
      const uint32_t sh = 8 * (k & 3);
      if (((part[k >> 2] >> sh) & 0xffu) == 0xffu) {
        part[k >> 2] &= ~(0xffu << sh);
        changed = true;
      }
    }
    if (changed) {
      q.x = part[0]; q.y = part[1]; q.z = part[2]; q.w = part[3];
      *p = q;
    }
  } else {
    for (int64_t c = c0; c < n_cells; c++)
      if (map[c] == -1) map[c] = 0;
  }
}

// Cell classes of MapUtil (map_util.h:44-48): 0 occupied (== 100), 1 free (0 <= v < 100), 2 unknown (== -1)
__device__ inline bool in_class(int8_t v, int kind) {
  return kind == 0 ? v == kOcc : kind == 1 ? (v >= 0 && v < kOcc) : v == -1;
}

// Column geometry: thread t -> x = t % d0, c = t / d0 (3D: y; 2D: 0); it walks `len` cells at stride `step` from
// x + d0 * c; its key in the reference's loop order is x * n_c + c.
struct Columns {
  int64_t d0, n_c, len, step;
};

__global__ __launch_bounds__(256) void cloud_count_kernel(const int8_t *__restrict__ map, Columns cl, int kind,
                                                          int32_t *__restrict__ count) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cl.d0 * cl.n_c) return;
  const int64_t x = t % cl.d0, c = t / cl.d0;
  const int8_t *p = map + x + cl.d0 * c;
  int32_t n = 0;
  for (int64_t k = 0; k < cl.len; k++) n += in_class(p[k * cl.step], kind) ? 1 : 0;
  count[x * cl.n_c + c] = n;
}

// Points [lo, hi) of the cloud, into xyz[(pos - lo) * dim]: only the columns whose scanned range meets the window walk.
__global__ __launch_bounds__(256) void cloud_fill_kernel(const int8_t *__restrict__ map, Columns cl, int kind, int dim,
                                                         const int64_t *__restrict__ offs, int64_t lo, int64_t hi,
                                                         double res, double o0, double o1, double o2,
                                                         double *__restrict__ xyz) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cl.d0 * cl.n_c) return;
  const int64_t x = t % cl.d0, c = t / cl.d0;
  const int64_t key = x * cl.n_c + c;
  int64_t pos = offs[key];
  if (pos >= hi || offs[key + 1] <= lo) return;
  const int8_t *p = map + x + cl.d0 * c;
  const double fx = ((double)x + 0.5) * res + o0;
  const double fc = ((double)c + 0.5) * res + o1;  // 3D: y
  for (int64_t k = 0; k < cl.len && pos < hi; k++) {
    if (!in_class(p[k * cl.step], kind)) continue;
    if (pos >= lo) {
      const double fk = ((double)k + 0.5) * res + (dim == 3 ? o2 : o1);
      if (dim == 3) {
        double *q = xyz + (pos - lo) * 3;
        q[0] = fx; q[1] = fc; q[2] = fk;
      } else {
        *(double2 *)(xyz + (pos - lo) * 2) = make_double2(fx, fk);
      }
    }
    pos++;
  }
}

Columns columns_of(int dim, const int32_t *d) {
  Columns cl;
  cl.d0 = d[0];
  cl.n_c = dim == 3 ? d[1] : 1;
  cl.len = dim == 3 ? d[2] : d[1];
  cl.step = dim == 3 ? (int64_t)d[0] * d[1] : (int64_t)d[0];
  return cl;
}

}  // namespace

int64_t dilate_words_per_row(int32_t d0) { return ((int64_t)d0 + 31) / 32; }

hipError_t launch_dilate(int8_t *map, const int32_t *d, const void *runs, int n_runs, uint32_t *bits, hipStream_t s) {
  if (n_runs <= 0) return hipSuccess;
  const int64_t words = dilate_words_per_row(d[0]);
  const int64_t n_words = words * d[1] * d[2];
  hipLaunchKernelGGL(pack_occupancy_kernel, dim3(blocks_for(n_words)), dim3(256), 0, s, map, (int64_t)d[0], words,
                     n_words, bits);
  hipLaunchKernelGGL(dilate_apply_kernel, dim3(blocks_for(n_words)), dim3(256), 0, s, bits, (const Run *)runs, n_runs,
                     (int64_t)d[0], (int64_t)d[1], (int64_t)d[2], words, map);
  return hipGetLastError();
}

hipError_t launch_free_unknown(int8_t *map, int64_t n_cells, hipStream_t s) {
  if (n_cells <= 0) return hipSuccess;
  hipLaunchKernelGGL(free_unknown_kernel, dim3(blocks_for((n_cells + 15) / 16)), dim3(256), 0, s, map, n_cells);
  return hipGetLastError();
}

hipError_t launch_cloud_count(const int8_t *map, int dim, const int32_t *d, int kind, int32_t *count, int64_t *offs,
                              hipStream_t s) {
  const Columns cl = columns_of(dim, d);
  const int64_t n_col = cl.d0 * cl.n_c;
  hipLaunchKernelGGL(cloud_count_kernel, dim3(blocks_for(n_col)), dim3(256), 0, s, map, cl, kind, count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_scan_counts(count, n_col, offs, s);
}

hipError_t launch_cloud_fill(const int8_t *map, int dim, const int32_t *d, int kind, const int64_t *offs, int64_t lo,
                             int64_t hi, double res, const double *origin, double *xyz, hipStream_t s) {
  if (hi <= lo) return hipSuccess;
  const Columns cl = columns_of(dim, d);
  const int64_t n_col = cl.d0 * cl.n_c;
  hipLaunchKernelGGL(cloud_fill_kernel, dim3(blocks_for(n_col)), dim3(256), 0, s, map, cl, kind, dim, offs, lo, hi, res,
                     origin[0], origin[1], dim == 3 ? origin[2] : 0.0, xyz);
  return hipGetLastError();
}

}  // namespace mplx
