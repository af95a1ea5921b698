// open_best_kernel.hip -- the k best open nodes per query (include/mplx_best.h): what a priority queue does when it
// hands out its k smallest keys, for the open set of open_kernel.hip.  The discipline is that file's: a launch boundary is
// the only ordering between passes, no workgroup waits for another, only integer adds and mins decide anything, every
// index is checked where it is formed, and a table with a status bit makes every pass return at its first instruction.
//
// Between the reduce pass and the tail (scan, emit, finish) of a select -- both open_kernel.hip's own kernels, untouched --
//   hist x 8   one lane per node id.  Pass p histograms digit p (8 bits, from the highest bit in which f_min and
//              T = f_min + delta differ downwards) of the candidates (open, f <= T) that match the prefix found so far:
//              hist[p][query][256], 32-bit adds, one per (wave, query, digit).  Pass p > 0 first derives its prefix from
//              the finished histogram of pass p - 1 -- in every wave, for every query the wave holds a candidate of: 4 bins
//              a lane and one wave scan -- and every such wave stores the same state.  A query is finished when its
//              candidates are no more than k (all are taken), when a bucket boundary falls on k, or at its last digit; a
//              pass no query needs returns at its first, uniform instruction (active[p - 1] == 0).
//   classify   per tile of 4096 ids: goal_id as open_mark_kernel finds it; every candidate is below its query's threshold
//              (mark 1), at it (mark 2) or above; tot[tile] = the nodes below; eqc[query][segment] = the nodes at the
//              threshold per segment of 1024 ids (a wave's share of the tile, walked in id order)
//   rank       per query, one wave: exclusive prefix sums of eqc over the segments
//   pick       per tile: a node at the threshold is taken iff its rank among its query's equals in id order is below
//              `ties`; the marks become 0 / 1 and tot[tile] the nodes taken.  rank and pick return at once when no node
//              lies at a threshold with a remainder (classify's marks are then final).
// The ranks are prefix sums in id order and the histograms integer sums: every output is a pure function of the inputs.
#include "mplx_internal.h"
#include "mplx_device_common.h"

namespace mplx {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunks = kBestSeg / 64;  // 64-id chunks a wave walks in order
static_assert(kWaves * kBestSeg == kTableTile, "a tile is one segment per wave");
static_assert(kBestBins == 4 * 64, "a lane scans 4 bins");
constexpr uint8_t kIsOpen = 1, kIsGoal = 2;  // MPLX_OPEN_* of include/mplx_open.h
constexpr int32_t kSelected = 0, kFound = 1, kEmpty = 2;

__device__ __forceinline__ int64_t node_count(const OpenArgs &A) {
  const int64_t n = A.t_ctl->n_nodes;
  return n < 0 ? 0 : (n < A.cap ? n : A.cap);
}

__device__ __forceinline__ int32_t query_of(const OpenArgs &A, int64_t id) {
  if (!A.t_query) return 0;
  const int32_t q = A.t_query[id];
  return (q >= 0 && q < A.n_queries) ? q : 0;  // (the column holds only queries: no index leaves the per-query arrays)
}

// open_kernel.hip's decide(): what the control block says once the reduce pass is complete
struct Decision {
  int32_t status;
  unsigned long long fmin_bits, goalf_bits, T_bits;
  double T;
};
__device__ __forceinline__ Decision decide(const OpenCtl *c, double delta) {
  Decision d;
  d.fmin_bits = c->fmin_bits;
  d.goalf_bits = c->goalf_bits;
  const double f_min = __longlong_as_double((long long)d.fmin_bits), goal_f = __longlong_as_double((long long)d.goalf_bits);
  d.status = (c->n_goal != 0 && goal_f <= f_min) ? kFound : c->n_open == 0 ? kEmpty : kSelected;
  d.T = f_min + delta;
  d.T_bits = (unsigned long long)__double_as_longlong(d.T);
  return d;
}

struct St {
  bool live;
  uint32_t shift, krem;
  unsigned long long prefix;
};
struct Fin {
  bool any, all;  // any: the query selects; all: every candidate
  uint32_t sh, ties;
  unsigned long long F;
};

// Pass 0's state: the candidates lie in [f_min, T], so the bits above the highest one in which the two differ are common
// to all of them and the first digit is the one that holds that bit (equal patterns: the lowest digit, for the count).
__device__ __forceinline__ St first_state(const BestArgs &B, int32_t q) {
  const Decision d = decide(B.o.ctl + q, B.o.delta);
  St s;
  s.live = d.status == kSelected;
  const unsigned long long x = d.fmin_bits ^ d.T_bits;
  const int nb = x ? 64 - __builtin_clzll(x) : 0;
  const int np = nb ? (nb + kBestBits - 1) / kBestBits : 1;
  s.shift = (uint32_t)(kBestBits * (np - 1));
  s.prefix = s.shift + kBestBits >= 64 ? 0ull : d.fmin_bits & ~((1ull << (s.shift + kBestBits)) - 1ull);
  s.krem = B.k;
  return s;
}

__device__ __forceinline__ bool matches(const St &s, unsigned long long v) {
  const uint32_t up = s.shift + kBestBits;
  return up >= 64 || (v >> up) == (s.prefix >> up);
}

// The finished histogram h[256] of the digit at s.shift -> the bucket of the s.krem-th candidate.  Every lane of the wave
// calls this with the same arguments and gets the same answer.  first: h counts every candidate of the query.
__device__ __forceinline__ bool resolve(const St &s, const uint32_t *h, bool first, uint32_t k, St *next, Fin *fin) {
  const int lane = threadIdx.x & 63;
  uint32_t c[4];
#pragma unroll
  for (int j = 0; j < 4; j++) c[j] = h[4 * lane + j];
  const uint32_t sum = c[0] + c[1] + c[2] + c[3];
  uint32_t inc = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
    if (lane >= d) inc += t;
  }
  const uint32_t total = (uint32_t)__shfl((int)inc, 63), exc = inc - sum;
  fin->any = true;
  fin->all = false;
  fin->sh = s.shift;
  fin->ties = 0;
  fin->F = s.prefix;
  if (first && total <= k) {
    fin->all = true;
    return true;
  }
  const bool owner = exc < s.krem && s.krem <= inc;  // one lane, as krem <= total
  const unsigned long long bal = __ballot(owner);
  if (!bal) return true;  // (never: nothing at the threshold, everything below the prefix)
  uint32_t r = s.krem - exc, b = 0, hb = c[0];
#pragma unroll
  for (int j = 0; j < 3; j++)
    if (b == (uint32_t)j && r > c[j]) {
      r -= c[j];
      b = j + 1;
      hb = c[j + 1];
    }
  const int src = __builtin_ctzll(bal);
  b = (uint32_t)__shfl((int)(4 * lane + b), src);
  r = (uint32_t)__shfl((int)r, src);
  hb = (uint32_t)__shfl((int)hb, src);
  const unsigned long long prefix = s.prefix | ((unsigned long long)b << s.shift);
  if (r == hb || s.shift == 0) {  // the bucket's end falls on k: all of it; or the last digit: prefix is the key
    fin->F = prefix;
    fin->ties = r;
    return true;
  }
  next->live = true;
  next->shift = s.shift - kBestBits;
  next->krem = r;
  next->prefix = prefix;
  return false;
}

__device__ __forceinline__ St load_state(const BestArgs &B, int p, int32_t q) {
  const BestState *m = B.state + (int64_t)p * B.o.n_queries + q;
  St s;
  s.live = m->live != 0;
  s.shift = m->shift < 64 ? m->shift : 0;
  s.krem = m->krem;
  s.prefix = m->prefix;
  return s;
}

__device__ __forceinline__ void store_final(BestFinal *m, const Fin &f) {
  m->all = f.all ? 1 : 0;
  m->sh = f.sh;
  m->ties = f.ties;
  m->F = f.F;
  m->valid = 1;
}

__device__ __forceinline__ Fin load_final(const BestFinal *m) {
  Fin f;
  f.any = m->valid != 0;
  f.all = m->all != 0;
  f.sh = m->sh < 64 ? m->sh : 0;
  f.ties = m->ties;
  f.F = m->F;
  return f;
}

// The state pass p histograms query q with (wave-uniform q, every lane calls).  Every wave that asks stores the same
// values: to state[p], which only the next launch reads, and to fin, which only classify and pick read.
__device__ __forceinline__ St pass_state(const BestArgs &B, int p, int32_t q) {
  const bool lane0 = (threadIdx.x & 63) == 0;
  St dead;
  dead.live = false;
  dead.shift = 0;
  dead.krem = 0;
  dead.prefix = 0;
  if (p == 0) {
    const St s = first_state(B, q);
    if (s.live && lane0) B.active[0] = 1;
    return s;
  }
  const St prev = p == 1 ? first_state(B, q) : load_state(B, p - 1, q);
  if (!prev.live) return dead;
  St next = dead;
  Fin fin;
  const bool done = resolve(prev, B.hist + ((int64_t)(p - 1) * B.o.n_queries + q) * kBestBins, p == 1, B.k, &next, &fin);
  if (done) {
    if (lane0) store_final(B.fin + q, fin);
    return dead;
  }
  if (lane0) {
    BestState *m = B.state + (int64_t)p * B.o.n_queries + q;
    m->shift = next.shift;
    m->krem = next.krem;
    m->prefix = next.prefix;
    m->live = 1;
    B.active[p] = 1;
  }
  return next;
}

__global__ __launch_bounds__(kBlock) void open_best_hist_kernel(const BestArgs B, int p) {
  const OpenArgs &A = B.o;
  if (A.t_ctl->status) return;               // (uniform)
  if (p > 0 && B.active[p - 1] == 0) return;  // (uniform) no query histogrammed in the pass before: all are finished
  const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool on = false;
  unsigned long long v = 0;
  int32_t q = 0;
  if (id < node_count(A) && (A.flags[id] & kIsOpen)) {
    v = A.f[id];
    q = query_of(A, id);
    const Decision d = decide(A.ctl + q, A.delta);
    on = d.status == kSelected && __longlong_as_double((long long)v) <= d.T;
  }
  unsigned long long left = __ballot(on);
  while (left) {  // one round per distinct query among the wave's candidates (one, when the wave holds one query)
    const int32_t qq = __shfl(q, __builtin_ctzll(left));
    const bool mine = on && q == qq;
    const St s = pass_state(B, p, qq);
    if (s.live) {
      const bool m = mine && matches(s, v);
      const uint32_t digit = (uint32_t)(v >> s.shift) & (kBestBins - 1);
      uint32_t *h = B.hist + ((int64_t)p * A.n_queries + qq) * kBestBins;
      unsigned long long rest = __ballot(m);
      while (rest) {  // one add per distinct digit
        const uint32_t d0 = (uint32_t)__shfl((int)digit, __builtin_ctzll(rest));
        const unsigned long long same = __ballot(m && digit == d0);
        if (lane == 0) atomicAdd(h + d0, (uint32_t)__popcll(same));
        rest &= ~same;
      }
    }
    left &= ~__ballot(mine);
  }
}

// The threshold of query q once the last histogram is complete (wave-uniform q, every lane calls).
__device__ __forceinline__ Fin query_final(const BestArgs &B, int32_t q) {
  Fin f = load_final(B.fin + q);
  if (f.any) return f;
  const St prev = load_state(B, kBestPasses - 1, q);
  if (!prev.live) return f;  // the query selects nothing
  St next = prev;
  if (!resolve(prev, B.hist + ((int64_t)(kBestPasses - 1) * B.o.n_queries + q) * kBestBins, false, B.k, &next, &f)) {
    f.sh = next.shift + kBestBits;  // (never: the last pass is at shift 0)
    f.F = next.prefix;
    f.ties = next.krem;
  }
  if ((threadIdx.x & 63) == 0) store_final(B.fin2 + q, f);
  return f;
}

__global__ __launch_bounds__(kBlock) void open_best_classify_kernel(const BestArgs B) {
  const OpenArgs &A = B.o;
  if (A.t_ctl->status) return;  // (uniform: nothing below is skipped by part of a workgroup)
  __shared__ uint32_t wsum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = node_count(A), base = (int64_t)blockIdx.x * kTableTile + (int64_t)wave * kBestSeg;
  const int64_t sg = (int64_t)blockIdx.x * kWaves + wave;
  uint32_t cnt = 0;
  int32_t have = -1;
  Fin fin;
  fin.any = fin.all = false;
  fin.sh = fin.ties = 0;
  fin.F = 0;
  for (int i = 0; i < kChunks; i++) {
    const int64_t id = base + (int64_t)i * 64 + lane;
    bool on = false;
    unsigned long long v = 0;
    int32_t q = 0;
    uint8_t cls = 0;
    if (id < n) {
      const uint8_t fl = A.flags[id];
      if (fl & (kIsOpen | kIsGoal)) {
        q = query_of(A, id);
        const Decision d = decide(A.ctl + q, A.delta);  // the node's own query decides
        v = A.f[id];
        if ((fl & kIsGoal) && v == d.goalf_bits) atomicMin(&A.ctl[q].goal_id, (int32_t)id);
        on = d.status == kSelected && (fl & kIsOpen) && __longlong_as_double((long long)v) <= d.T;
      }
    }
    unsigned long long left = __ballot(on);
    while (left) {  // one round per distinct query among the chunk's candidates
      const int32_t qq = __shfl(q, __builtin_ctzll(left));
      if (qq != have) {  // (uniform)
        fin = query_final(B, qq);
        have = qq;
      }
      const bool mine = on && q == qq;
      if (mine && fin.any) {
        const unsigned long long a = v >> fin.sh, b = fin.F >> fin.sh;
        cls = fin.all || a < b ? 1 : a == b ? 2 : 0;
      }
      const unsigned long long eq = __ballot(mine && cls == 2);
      if (eq && lane == 0 && sg < B.seg_stride) {
        B.eqc[(int64_t)qq * B.seg_stride + sg] += (uint32_t)__popcll(eq);  // this wave's own entry
        B.active[kBestPasses] = 1;
      }
      left &= ~__ballot(mine);
    }
    if (id < n) A.mark[id] = cls;
    cnt += (uint32_t)__popcll(__ballot(cls == 1));  // the wave's count, in every lane
  }
  if (lane == 0) wsum[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kWaves; w++) t += wsum[w];
    A.tot[blockIdx.x] = t;
  }
}

// One wave per query: eqc[q][0 .. n_seg) -> its exclusive prefix sums.
__global__ __launch_bounds__(kBlock) void open_best_rank_kernel(const BestArgs B) {
  const OpenArgs &A = B.o;
  if (A.t_ctl->status || B.active[kBestPasses] == 0) return;  // (uniform)
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (q >= A.n_queries) return;  // (wave-uniform)
  int64_t n_seg = A.n_tiles * kWaves;
  n_seg = n_seg < B.seg_stride ? n_seg : B.seg_stride;
  uint32_t *e = B.eqc + q * B.seg_stride;
  const int64_t per = (n_seg + 63) / 64;
  const int64_t a = (int64_t)lane * per < n_seg ? (int64_t)lane * per : n_seg, b = a + per < n_seg ? a + per : n_seg;
  uint32_t sum = 0;
  for (int64_t s = a; s < b; s++) sum += e[s];
  uint32_t inc = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
    if (lane >= d) inc += t;
  }
  uint32_t run = inc - sum;
  for (int64_t s = a; s < b; s++) {
    const uint32_t c = e[s];
    e[s] = run;
    run += c;
  }
}

__global__ __launch_bounds__(kBlock) void open_best_pick_kernel(const BestArgs B) {
  const OpenArgs &A = B.o;
  if (A.t_ctl->status || B.active[kBestPasses] == 0) return;  // (uniform)
  __shared__ uint32_t wsum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = node_count(A), base = (int64_t)blockIdx.x * kTableTile + (int64_t)wave * kBestSeg;
  const int64_t sg = (int64_t)blockIdx.x * kWaves + wave;
  uint32_t cnt = 0, ties = 0;
  int32_t have = -1;
  for (int i = 0; i < kChunks; i++) {
    const int64_t id = base + (int64_t)i * 64 + lane;
    const uint8_t cls = id < n ? A.mark[id] : 0;
    const bool eq = cls == 2;
    const int32_t q = eq ? query_of(A, id) : 0;
    bool take = cls == 1;
    unsigned long long left = __ballot(eq);
    while (left) {  // one round per distinct query among the chunk's nodes at a threshold
      const int32_t qq = __shfl(q, __builtin_ctzll(left));
      if (qq != have) {  // (uniform)
        Fin f = load_final(B.fin + qq);
        if (!f.any) f = load_final(B.fin2 + qq);
        ties = f.any ? f.ties : 0;
        have = qq;
      }
      const bool mine = eq && q == qq;
      const unsigned long long bm = __ballot(mine);
      uint32_t before = 0;
      if (lane == 0 && sg < B.seg_stride) {  // the equals of qq in front of this chunk; this wave's own entry
        uint32_t *e = B.eqc + (int64_t)qq * B.seg_stride + sg;
        before = *e;
        *e = before + (uint32_t)__popcll(bm);
      }
      before = (uint32_t)__shfl((int)before, 0);
      if (mine) take = before + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull)) < ties;
      left &= ~bm;
    }
    if (eq) A.mark[id] = take ? 1 : 0;
    cnt += (uint32_t)__popcll(__ballot(take));
  }
  if (lane == 0) wsum[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kWaves; w++) t += wsum[w];
    A.tot[blockIdx.x] = t;
  }
}

}  // namespace

hipError_t launch_open_best(const BestArgs &b, hipStream_t s) {
  const OpenArgs &a = b.o;
  const int64_t n = a.n_bound > 0 ? a.n_bound : 1;
  const dim3 per_node((unsigned)((n + kBlock - 1) / kBlock)), per_tile((unsigned)a.n_tiles), block(kBlock);
  for (int p = 0; p < kBestPasses; p++) hipLaunchKernelGGL(open_best_hist_kernel, per_node, block, 0, s, b, p);
  hipLaunchKernelGGL(open_best_classify_kernel, per_tile, block, 0, s, b);
  hipLaunchKernelGGL(open_best_rank_kernel, dim3((unsigned)((a.n_queries + kWaves - 1) / kWaves)), block, 0, s, b);
  hipLaunchKernelGGL(open_best_pick_kernel, per_tile, block, 0, s, b);
  return hipGetLastError();
}

}  // namespace mplx
