// Internal declarations shared by the C-ABI layer (mplx_api.cpp and the units beside it) and the HIP
// kernels (expand_kernel.hip).  Not installed; the public surface is
// include/mplx.h.
#ifndef MPLX_INTERNAL_H
#define MPLX_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mplx {

// validate_yaw (reference include/mpl_basis/primitive.h:504-525) compares d = v_hat . (cos yaw, sin yaw) with
// cos(yaw_max), and the reference's cos / sin are the HOST libm's.  The device's (OCML) differ from glibc's in the
// last place on a few per cent of arguments, so a decision within rounding noise of the threshold could come out
// differently.  Pinning: the detection pass (amb != null) flags every node with a decision closer to the threshold
// than `margin` (a bound on what the two libraries' rounding can move d - cos(yaw_max); decisions farther away are
// the same under either library) and the host then re-expands exactly those nodes in an override pass (tab != null)
// in which every cos / sin of a heading-limit decision and cos(yaw_max) come from a table the HOST filled with its
// libm, so the decision is the reference's own arithmetic on the reference's own values.  The per-sample heading
// COST (env_map.h:121-129) keeps device trig: it is continuous and held to north_star's 1e-6.
struct YawPin {
  int32_t *amb;               // detection: [0] = number of flagged nodes, [1 .. cap] their indices; null = off
  int32_t *any_host;          // detection: a word of pinned host memory set to 1 by any flagging wave (plain store), so
                              // that the host learns "nothing flagged" from its own memory, without a copy
  int32_t amb_cap;
  double margin;
  double tie_yaw;             // detection: yaw_max when the "velocity along x, |yaw| == yaw_max" tie is exact under the host's
                              // libm too (mplx_device_common.h near_limit), NaN when it is not (then no decision is exempt)
  const int32_t *node_list;   // override pass: the nodes to re-expand (kernel node k -> node_list[k]); null = all
  const double *tab;          // override pass: per listed node the host's trig values (layout per kernel); null = off
  int32_t tab_stride;         // doubles per listed node
  double cos_lim;             // override pass: the host's cos(yaw_max)
};

// Everything one expansion launch needs, passed by value as the kernel
// argument block (lives in SGPRs / constant cache: wave-uniform).
struct ExpandArgs {
  // voxel / occupancy grid, row-major with x fastest (reference
  // include/mpl_collision/map_util.h:34-41)
  const int8_t *map;
  const int8_t *pot;       // potential cells or nullptr (env_map.h:113-118)
  const uint32_t *region;  // search region, 1 bit per cell, or nullptr
  int32_t dim0, dim1, dim2;
  double org0, org1, org2;
  double res;
  // env parameters (env_base.h:368-392, env_map.h:294-296)
  double dt, w, wyaw;
  double v_max, a_max, j_max, yaw_max;
  double pot_w, grad_w;
  // controls [nU][udim]
  const double *U;
  int32_t nU, udim;
  // frontier, field-major [4D+2][node_stride]
  const double *nodes;
  int64_t n_nodes, node_stride;
  // dense successor slots (any may be nullptr)
  uint8_t *status;
  double *cost;
  uint64_t *hash;
  double *state;
  int64_t state_stride;
  int32_t *iters;
  int32_t stream_out;  // 1: the slots are final outputs (non-temporal stores); 0: scratch that is re-read soon
  YawPin yaw;          // heading-limit decisions pinned to the host libm (see YawPin)
};

// Arguments of the tiled, list-producing kernel (expand_tile_kernel.hip).
// Completion of a small synchronous launch seen through a word the KERNEL writes into pinned host memory when its last
// wave (workgroup) is through, instead of through hipStreamSynchronize: 8.2 us per empty launch + completion against
// 12.8 us (profiles/micro/mailbox_latency.hip).  flag == nullptr: no signalling (every launch the caller does not wait
// for on the spot).
struct DoneSignal {
  uint64_t *flag;   // pinned host memory; receives `seq` (system-scope release) after every store of the launch
  uint32_t *count;  // device memory, 0 between launches: waves (workgroups) that have finished
  uint64_t seq;
};

// What the graph search computes for every successor right after get_succ (graph_search.h:84-88),
// fused into the list stores of the expansion kernels: default heuristic (env_base.h:46-64) and goal flags
// (env_map.h:25-37, bit 0; env_base.h:47, bit 1).  Null pointers = off.  Same arithmetic as post_kernel.hip.
struct PostFuse {
  double *heur;     // [n_nodes * l_nstride] or null
  uint8_t *flags;   // [n_nodes * l_nstride] or null
  double goal[14];  // the goal waypoint's rows (pos, vel, acc, jrk, yaw, t)
  uint64_t goal_hash;
  double w, v_max, tol_pos, tol_vel, tol_acc, tol_yaw;
};

// Mailbox of the resident (service) form of the tiled kernel, in pinned host memory; every word on its own line.
struct SvcMailbox {
  uint64_t doorbell;  // host -> device: (seq << 32) | n_nodes of the request in the landing block
  uint64_t pad0[7];
  uint64_t done;      // device -> host: seq of the last request whose lists are complete in the landing block
  uint64_t pad1[7];
  uint32_t quit;      // host -> device: leave now
  uint32_t pad2[15];
  uint32_t alive;     // device -> host: 0 once the coordinator has decided to leave (the stream then drains)
  uint32_t pad3[15];
};

struct TileArgs {
  const int8_t *map;
  const uint32_t *region;
  int32_t dim0, dim1, dim2;
  double org0, org1, org2;
  double res;
  double dt, w;
  double v_max, a_max, j_max;
  const double *U;
  int32_t nU, udim;
  float inv_nU;
  const double *nodes;
  int64_t n_nodes, node_stride;
  // tiling
  int32_t npb;         // whole nodes per workgroup
  int32_t tile_pairs;  // npb * nU  (<= 1024)
  int32_t wl_cap;      // work-list capacity in samples
  int32_t n_max;       // largest sample count n served by the work list (<= 63)
  int32_t dbg;         // timing ablations (env MPLX_TILE_DBG); 0 in production
  int32_t lds_u_offset;  // byte offset of the control table inside the dynamic LDS
  int32_t grid_limit;  // persistent workgroups to launch (CUs x workgroups per CU)
  // tables made by launch_make_tables
  const double *ttab;          // [64][64] accumulated sample times
  const unsigned char *tcnt;   // [64] loop iteration counts
  double Rres, R001, R01;      // refined reciprocals of res, 0.01, 0.1
  // per-node successor lists: node k owns entries [k*nU, k*nU + l_count[k])
  int32_t *l_count;
  int32_t *l_action;
  double *l_cost;
  uint64_t *l_hash;
  double *l_state;
  int64_t l_stride;
  int32_t *l_iters;
  int64_t l_nstride;  // entries reserved per node (>= nU)
  int32_t l_pad;      // 1: complete the last 128-byte line of every list row (node stride is a multiple of 32)
  PostFuse post;      // heuristic / goal flags per successor, same indexing as the lists
  // service mode (expand_tile_kernel.hip): null / 0 for an ordinary launch
  SvcMailbox *svc_mb;   // pinned host memory
  uint64_t *svc_dev;    // device memory, zeroed before the launch: [0] = command, [1 + g] = last request workgroup g finished
  uint64_t svc_seq0;    // seq of the last request served before this launch
  uint64_t svc_idle;    // ticks of the 100 MHz clock without a request after which the kernel leaves
  DoneSignal done;      // ordinary launches of small synchronous batches
};

size_t tile_lds_bytes(int tile_pairs, int npb, int wl_cap, int n_max, int n_fields, int u_doubles,
                      int *u_offset);
hipError_t launch_make_tables(double T, double res, double *ttab, unsigned char *tcnt, double *recips,
                              hipStream_t stream);
hipError_t launch_expand_tile(int dim, int control, const TileArgs &args, hipStream_t stream);
int tile_service_resident_workgroups(int dim, int control, const TileArgs &a);  // 0: unknown

// Arguments of the factorised list-producing kernel (expand_grid_kernel.hip):
// the control table is given per axis as its distinct values plus, per control,
// the packed indices of its entries (j0 | j1 << 8 | j2 << 16).
struct GridArgs {
  const uint32_t *blk;   // blocked-bit map, 1 bit per cell, x fastest (launch_build_blocked_bits)
  int64_t blk_words;
  const int8_t *pot;     // potential map (then blk / sat describe "potential > 0 or outside the region") or null
  const uint32_t *region; // search region bits (read by the potential path only; folded into blk otherwise)
  double pot_w, grad_w;  // env_map.h:115-116: potential_weight, gradient_weight
  const uint32_t *sat;   // summed-area table of blk, sizes dim+1 with a zero border (launch_build_sat), or null
  int32_t dim0, dim1, dim2;
  double org0, org1, org2;
  double res;
  double dt, w;
  double v_max, a_max, j_max;
  double yaw_max, wyaw;  // yaw controls only
  const double *uvals;   // [4][16] distinct control values of each axis; row 3 = yaw rates (expand_lex_kernel: [3][uval_stride])
  int32_t uval_stride;   // 16, or 32 for the wide tables only expand_lex_kernel.hip takes (17 .. 32 values on an axis)
  const uint32_t *uidx;  // [nU] packed per-axis value indices
  int32_t nd0, nd1, nd2; // number of distinct values per axis
  int32_t ndy;           // distinct yaw rates (yaw controls)
  int32_t ulex;          // 1: control i is the i-th combination of the per-axis values in lexicographic order
  int32_t ndp;           // table stride over values (max nd)
  int32_t nU;
  const double *nodes;
  int64_t n_nodes, node_stride;
  int32_t n_max;         // largest sample count n (<= 61)
  int32_t rmax;          // sample counts handled per round (rows of cell codes per axis entry)
  int32_t boxcap;        // dwords of LDS per wave for the staged blocked bits
  int32_t gather;        // 1: no box staging, the sample loops read the blocked-bit map directly (small control tables)
  int32_t lex;           // host side only: 1 = this launch goes to expand_lex_kernel.hip (same arguments, its own LDS carve-up)
  // Dynamic node assignment (work == null: static striding).  Nodes differ a lot in work (dead at t = 0, free box, one
  // or several passes), and with a static assignment the waves lived only 46 % (C5) - 83 % (C4) of the kernel's
  // duration (SQ_WAVE_CYCLES against SQ_BUSY_CYCLES).  Chunks of work_chunk nodes: chunk w < W (the waves launched)
  // belongs to wave w, the others are claimed from kWorkCounters counters (a single counter serialises at ~15 ns per
  // claim: measured 3 x slower than static), counter blockIdx % kWorkCounters owning an equal share of them; each
  // counter sits on its own 128-byte line.  `work` is zero when the launch begins; the launch zeroes `work_zero`, the
  // set the NEXT launch of the stream will use (ping-pong: no memset, no bookkeeping between launches).
  unsigned int *work;
  unsigned int *work_zero;
  int32_t work_chunk;
  int32_t work_blocked;  // 1: every counter owns one contiguous block of chunks; 0: the chunks are dealt round-robin
  int32_t dbg;           // timing ablations (env MPLX_TILE_DBG); 0 in production
  int32_t grid_limit;    // persistent workgroups to launch
  const double *ttab;    // tables of launch_make_tables
  const unsigned char *tcnt;
  double Rres, R001, R01;
  int32_t *l_count;
  int32_t *l_action;
  double *l_cost;
  uint64_t *l_hash;
  double *l_state;
  int64_t l_stride;
  int32_t *l_iters;
  int64_t l_nstride;  // entries reserved per node (>= nU)
  int32_t l_pad;      // 1: complete the last 128-byte line of every list row (node stride is a multiple of 32)
  // State rows this launch does not store to (bit f = row f of l_state): rows the caller vouches hold +0.0 in every
  // entry AND that this control can only fill with the literal +0.0 (mplx_expand_lists_device_z, include/mplx.h).
  // Padding lanes of such a row are skipped as well.  0: every row is written.
  uint32_t l_zrows;
  PostFuse post;      // heuristic / goal flags per successor, same indexing as the lists
  YawPin yaw;        // heading-limit decisions pinned to the host libm (see YawPin); tab row: [c0, s0, cT[16], sT[16]]
  // Pre-screen of yaw controls (grid_prescreen_kernel): the nodes whose own heading passes validate_yaw at t = 0, in
  // frontier order, and their number (device memory, written by the pre-screen launch that precedes this one on the
  // stream).  Null: the kernel walks [0, n_nodes) and tests every node itself.
  const int32_t *live;
  const uint32_t *live_n;
  DoneSignal done;      // small synchronous batches: see DoneSignal
};
// expand_pair_kernel.hip: yaw controls on a potential map over a pre-screened frontier, two nodes per wave (same
// arguments as expand_grid_kernel; GridArgs::live / live_n must be set, grid_limit = workgroups to launch)
size_t pair_lds_bytes(int dim, int order, int nU, int ndp, int n_max, int rmax, bool ycost, int ndy);
int pair_waves_per_block();
int pair_nodes_per_wave();
int pair_max_yaw_rates();   // yaw rates a lane of it carries through its sample loop
bool pair_covers(int dim, int control);
hipError_t launch_expand_pair(int dim, int control, const GridArgs &a, hipStream_t s);
int pair_resident_blocks(int dim, int control, int ndy, size_t lds);
constexpr int kWorkCounters = 64;
// list rows are completed to whole 128-byte lines only for control tables of at least this many entries (line_pad, mplx_ctx.h)
constexpr int kLinePadMinControls = 256;
// lane-per-node validate_yaw(t = 0) over a whole frontier (expand_grid_kernel.hip); fills live / live_n of `a`'s launch
// (live_n is zero when the launch begins; the launch zeroes live_zero, the counter of the NEXT pre-screen of the stream)
hipError_t launch_grid_prescreen(int dim, int control, const GridArgs &a, int32_t *live, uint32_t *live_n, uint32_t *live_zero,
                                 hipStream_t s);
// Packing of the used list prefixes for the copy back to the host (pack_kernel.hip).
constexpr int kPackRows = 24;
struct PackArgs {
  const void *src[kPackRows];   // device rows, [n_nodes * node_stride] elements each
  int64_t dst_off[kPackRows];   // byte offset of the row's packed block inside dst
  int32_t es[kPackRows];        // element size, 4 or 8
  int32_t n_rows;
  int64_t node_stride;
  const int32_t *count;         // [n_nodes]
  const int64_t *offs;          // [n_nodes] exclusive prefix sum of count
  int64_t node0, off0;          // first node of the chunk and its offs
  char *dst;
};
hipError_t launch_pack_rows(const PackArgs &args, int64_t n_nodes, hipStream_t stream);
// offs[0..n] = exclusive prefix sums of count[0..n) (offs[n] = total); device pointers
hipError_t launch_scan_counts(const int32_t *count, int64_t n, int64_t *offs, hipStream_t stream);
size_t grid_lds_bytes(int dim, int order, int nU, int ndp, int n_max, int rmax, int boxcap, int yaw_mode, int ndy,
                      int ulex);
int grid_waves_per_block();
// workgroups of the (dim, control, potential) instantiation resident per CU with `lds` bytes each; 0 = unknown
int grid_resident_blocks(int dim, int control, bool pot, size_t lds);
hipError_t launch_expand_grid(int dim, int control, const GridArgs &args, hipStream_t stream);
// expand_lex_kernel.hip: the same function for lexicographic control tables without yaw on an occupancy map (GridArgs
// with ulex == 1, pot == null, live == null, yaw unused); its own LDS carve-up
bool lex_covers(int dim, int control);
size_t lex_lds_bytes(int dim, int order, int ndp, int nU, int n_max, int rmax, int boxcap);
int lex_waves_per_block();
int lex_resident_blocks(int dim, int control, int ndp, size_t lds);
hipError_t launch_expand_lex(int dim, int control, const GridArgs &args, hipStream_t stream);
// Blocked-bit map: 1 bit per cell in map order, 1 = occupied or outside the search
// region; (n_cells + 31) / 32 dwords.
// Summed-area table of the blocked bits: (d0+1)(d1+1)(d2+1) uint32 (2D: (d0+1)(d1+1)*2).
// mplx_edit_map: cells and (blk != null) their blocked bits patched in place (map_prep_kernel.hip)
hipError_t launch_gather_cells(const int8_t *cells, const int64_t *idx, int64_t n, int8_t *out, hipStream_t s);
hipError_t launch_edit_map(const int64_t *idx, const int8_t *val, int64_t n, int64_t n_cells, int8_t *map, uint32_t *blk,
                           const uint32_t *region, hipStream_t s);
// MapUtil::dilate / freeUnknown / clouds on the device map (map_util_kernel.hip, map_util_api.cpp).
// Dilation: `runs` = n_runs records {dy, dz, b, len} (int32 each; dx in [b - len + 1, b], 1 <= len <= 33, |offset| <
// map size per axis), `bits` = scratch of dilate_words_per_row(d[0]) * d[1] * d[2] words.
int64_t dilate_words_per_row(int32_t d0);
hipError_t launch_dilate(int8_t *map, const int32_t *d, const void *runs, int n_runs, uint32_t *bits, hipStream_t s);
hipError_t launch_free_unknown(int8_t *map, int64_t n_cells, hipStream_t s);
// Clouds: count[d0 * (3D: d1, 2D: 1)] cells of class `kind` per column, offs[n + 1] their exclusive scan in the
// reference's loop order; the fill writes points [lo, hi) of the cloud to xyz ([hi - lo][dim] doubles).
hipError_t launch_cloud_count(const int8_t *map, int dim, const int32_t *d, int kind, int32_t *count, int64_t *offs,
                              hipStream_t s);
hipError_t launch_cloud_fill(const int8_t *map, int dim, const int32_t *d, int kind, const int64_t *offs, int64_t lo,
                             int64_t hi, double res, const double *origin, double *xyz, hipStream_t s);
hipError_t launch_build_sat(int dim, const uint32_t *blk, const int32_t *mdim, uint32_t *sat, hipStream_t stream);
hipError_t launch_build_blocked_bits(const int8_t *map, const uint32_t *region, int64_t n_cells, int potential,
                                     uint32_t *out, hipStream_t stream);

// store_model_kernel.hip (diagnostic): the list stores of a launch alone, into the lists themselves; bit f of skip_rows:
// state row f is left alone (GridArgs::l_zrows of the launch that is modelled)
hipError_t launch_store_model(const int32_t *count, int64_t n_nodes, int64_t S, int32_t *action, double *cost, uint64_t *hash,
                              double *state, int64_t state_stride, int n_fields, int pad, int blocks, int mode,
                              uint32_t skip_rows, hipStream_t s);

// Batched edge re-validation (edge_kernel.hip).
struct EdgeArgs {
  const int8_t *map;
  const uint32_t *region;
  int32_t dim0, dim1, dim2;
  double org0, org1, org2;
  double res;
  double dt, w;
  const double *U;
  int32_t nU, udim;
  const double *parents;   // [4D+2][stride]
  const int32_t *action;   // [n_edges]
  int64_t n_edges, stride;
  uint8_t *free_out;       // outputs, any may be null
  double *cost;
  int32_t *cells;          // [n_edges][cell_cap]
  int32_t *cell_count;
  int32_t cell_cap;
  uint8_t *outside_out;    // [n_edges] some sample outside the map, or null
};
hipError_t launch_check_edges(int dim, int control, const EdgeArgs &args, hipStream_t s);

// Successor post-processing (post_kernel.hip): heuristic, goal tolerances, node identity.
struct PostArgs {
  const int32_t *count;    // [n_nodes]
  const uint64_t *hash;    // [n_nodes * nstride]
  const double *state;     // [4D+2][sstride]
  int64_t n_nodes, nstride, sstride;
  double goal[14];         // goal waypoint, 4D+2 doubles
  uint64_t goal_hash;
  double w, v_max, tol_pos, tol_vel, tol_acc, tol_yaw;
  double *heur;            // outputs, any may be null
  uint8_t *flags;
  int32_t *canon;
  struct Slot { uint64_t key; uint32_t val; uint32_t pad; };
  Slot *keys;              // identity table: cap + 1 slots, cap a power of two; key = ~0 empty, val = smallest index
  uint64_t cap;            // (keys == null and canon != null: canon was filled by launch_identity before this launch)
};
hipError_t launch_post_lists(int dim, const PostArgs &args, hipStream_t s);
hipError_t launch_post_clear_first_flags(const PostArgs &args, hipStream_t s);  // bit 2 of every emitted entry's flags back to 0

// Node identity by radix partition + per-bucket LDS tables (identity_kernel.hip): canon[g] = smallest list index with
// the same lattice hash, for every emitted successor g.  The lists are the strided form (packed lists: n_nodes = 1,
// nstride = capacity, count = &total).
struct IdentityArgs {
  const int32_t *count;
  const uint64_t *hash;
  int64_t n_nodes, nstride;
  int32_t *canon;
  uint64_t *hk[2];   // workspace: (hash, list index) pairs after partition level 1 / 2, n_slots each
  uint32_t *gi[2];
  uint32_t *cnt[2];  // per level: (digit, tile) counters -> exclusive prefix sums inside 4096-blocks
  uint32_t *tot[2];  // per level: scanned block totals, [blocks + 1]
  uint32_t *seg;     // level-1 buckets as segments of level 2: start[nb1 + 1], tile prefix[nb1 + 1]
  uint32_t *range;   // [buckets + 1]: where every fine bucket starts in the partitioned pairs
  int64_t n_slots, tiles1, tiles2_cap;
  int b1, b2;        // digit bits of the two levels (b2 = 0: one level)
  int fill;          // distinct keys one round of a bucket's LDS table takes (identity_default_fill(); tests lower it)
  // claimed form (two levels only): buckets of fixed capacity, a tile claims its run of a bucket with one returning
  // atomic on the bucket's cursor -- no histogram passes, no prefix sums.  A bucket that overflows sets *ovf_host (pinned)
  // and the caller runs the exact form above instead.
  int claimed;
  uint32_t *cur1;      // [64 x 8 shards] level-1 cursors, kCurPad words apart
  uint32_t *cur2;      // [buckets] level-2 cursors = pairs in every fine bucket
  uint32_t *tile_seg;  // level-2 tiles: segment << 20 | tile inside the segment; [n_tiles2] behind the count at [0]
  uint32_t *ovf;       // device copy of the overflow flag: the later launches of the same call return at once
  int32_t *ovf_host;
  int64_t subcap1, cap2, tiles2_max;
};
void identity_claimed_sizes(int64_t n_slots, int b1, int b2, int64_t *subcap1, int64_t *cap2, int64_t *pairs1, int64_t *pairs2,
                            int64_t *tiles2_max, int64_t *cur_words);
int identity_default_fill();
void identity_plan(int64_t n_slots, int *b1, int *b2);
void identity_sizes(int64_t n_slots, int b1, int b2, int64_t *tiles1, int64_t *tiles2_cap, int64_t *ctr1, int64_t *ctr2);
hipError_t launch_identity(const IdentityArgs &a, int64_t ctr1, int64_t ctr2, hipStream_t s);
hipError_t launch_identity_claimed(const IdentityArgs &a, int64_t cur_words, hipStream_t s);

// Map preprocessing (map_prep_kernel.hip).  d, c1, c2: 3 entries (unused axes 1 / [0,1)).
hipError_t launch_potential_passes(const int8_t *map, const int32_t *d, const int32_t *c1, const int32_t *c2, int rn,
                                   int hn, const int8_t *lut, int8_t h_max, unsigned short *tmp_a,
                                   unsigned short *tmp_b, int8_t *out, hipStream_t s);
hipError_t launch_region_boxes(const int *cells, int n_path_cells, int dim, const int32_t *d, const int32_t *rn,
                               uint32_t *bits, hipStream_t s);
hipError_t launch_unpack_region(const uint32_t *bits, int64_t n_cells, uint8_t *bytes, hipStream_t s);

// Dense slots of a chunk of nodes -> per-node successor lists (used for the
// configurations the tiled kernel does not cover).
struct CompactArgs {
  const uint8_t *status;
  const double *cost;
  const uint64_t *hash;
  const double *state;   // [F][chunk_slots]
  const int32_t *iters;
  int64_t chunk_slots;
  int32_t nU, n_fields;
  int64_t node_offset, n_nodes_chunk;
  int32_t *l_count;
  int32_t *l_action;
  double *l_cost;
  uint64_t *l_hash;
  double *l_state;
  int64_t l_stride;
  int32_t *l_iters;
  int64_t l_nstride;  // entries reserved per node (>= nU)
  int32_t l_pad;      // 1: complete the last 128-byte line of every list row (node stride is a multiple of 32)
};
hipError_t launch_compact_lists(const CompactArgs &args, hipStream_t stream);

// Launches the successor-expansion kernel specialised for (dim, control) on
// `stream`.  Returns hipSuccess or the launch error.
hipError_t launch_expand(int dim, int control, const ExpandArgs &args, hipStream_t stream);

// Batched rollouts (rollout_kernel.hip, include/mplx_rollout.h): one lane walks one action sequence, one pair per
// step, with the pair arithmetic of expand_kernel.hip (mplx_pair_device.h).
struct RolloutArgs {
  ExpandArgs env;          // map, region, parameters and controls as expand_args() fills them; nodes / slots unused
  const double *starts;    // field-major [4D+2][start_stride]
  int64_t n_starts, start_stride;  // n_starts == 1: every rollout starts at column 0
  const int32_t *actions;  // step-major: rollout k at step h = actions[h * action_stride + k]
  int64_t n_rollouts, action_stride;
  int32_t horizon;
  int32_t u_lds;           // 1: the control table is staged in LDS (nU * udim doubles of dynamic LDS)
  int32_t band;            // 1: heading-limit decisions within env.yaw.margin of their threshold set bit 0x80 of status
  // outputs, any may be null
  uint8_t *status;
  int32_t *steps;
  double *cost, *prefix_cost;
  double *end_state;
  int64_t end_stride;
  uint64_t *end_hash;
  PostFuse post;           // goal of mplx_set_goal; heur / flags = the end_heur / end_flags rows ([n_rollouts]) or null
};
constexpr size_t kRolloutLdsControls = 32 * 1024;  // largest control table staged in LDS (C4: 729 x 3 x 8 B = 17.5 KB)
hipError_t launch_rollout(int dim, int control, const RolloutArgs &args, hipStream_t stream);

// MapUtil::rayTrace on the device map and the ray trace of env_map::is_goal (ray_kernel.hip, ray_api.cpp;
// include/mplx_ray.h).  The int8 occupancy map, never the potential copy or the blocked bits.
struct RayArgs {
  const int8_t *map;
  int32_t dim0, dim1, dim2;
  double org0, org1, org2;
  double res;
  // query: points field-major [D][stride]; p2_stride == 0: one p2 (D consecutive doubles)
  const double *p1, *p2;
  int64_t n, stride, p2_stride;
  uint8_t *status;
  int32_t *n_cells, *first_hit, *cells;
  int32_t cell_cap;
};
struct GoalSightArgs {
  RayArgs ray;             // map and geometry; the point and output fields are unused
  const int32_t *count;    // lists: [n_nodes]
  const double *state;     // lists: position rows 0 .. D-1 of [4D+2][sstride]
  int64_t n_nodes, nstride, sstride;
  double goal[3];
  // the per-row form (the open set of a table with several queries): entry i aims at goals[row_query[i]]; null: `goal`
  const struct PostFuse *goals;
  const int32_t *row_query;
  uint8_t *flags;          // [n_nodes * nstride]; bit 0 read, bit 3 ORed in
  int32_t *work;           // [n_nodes * nstride] list indices of the candidates
  uint32_t *work_count;    // their number; zero before the scan
};
// lanes in {4, 16, 64}
hipError_t launch_ray_trace(int dim, int lanes, const RayArgs &a, hipStream_t s);
hipError_t launch_goal_sight(int dim, int lanes, int n_cus, const GoalSightArgs &a, hipStream_t s);

// Trajectory<Dim> on the device (traj_kernel.hip, traj_api.cpp; include/mplx_traj.h).  The chain launch writes the
// segment table of a trajectory set into scratch memory of the context; the sample and traverse launches read it.
// Table, N = n_traj, H = horizon, NC = 5 D + 2: S[N], n[N] (samples - 1 of the traversal, -1 = BAD), status[N], T[N],
// tau[H + 1][N], seg[H][NC][N] -- per segment and axis the coefficients c1 .. c5 of primitive.h:34-50 (c0 is always 0),
// then the yaw primitive's c4 (yaw rate) and c5 (yaw); all zero-padded rows are never read.
struct TrajArgs {
  ExpandArgs env;          // map, potential, geometry, parameters and controls as expand_args() fills them
  const double *starts;    // field-major [4D+2][start_stride]
  int64_t n_starts, start_stride;
  const int32_t *actions;  // step-major
  int64_t n_traj, action_stride;
  int32_t horizon;
  int32_t yaw;             // the control flag has the yaw bit
  int32_t *tab_S, *tab_n;
  uint8_t *tab_status;
  double *tab_T, *tab_tau, *tab_seg;
  // info outputs (chain launch), any may be null
  uint8_t *status;
  int32_t *n_segs;
  double *total_time, *effort, *seg_state;
  int64_t effort_stride, seg_stride;
  // sample launch
  int32_t n_uniform;       // N, or 0: times from `times`
  const double *times;
  int64_t time_stride;     // 0: shared by all trajectories
  int64_t count;           // samples per trajectory: N + 1 or Q
  double *out;
  int64_t row_stride, sample_stride;
  // traverse launch, any may be null
  double *cost;
  int32_t *n_samples, *n_cells, *stop_sample;
  // the table of a solved set (include/mplx_solve.h; appended: every field above keeps its place).  poly == 1: a segment
  // has 6 D + 2 rows (c0 .. c5 per axis, then the yaw primitive's c4, c5) and its own duration tab_dt[s][N]; the segment
  // of a time is found by bisection of tab_tau; tab_n is not used (the traversal forms n from T); tab_wp: the waypoints,
  // [4D+2][horizon + 1][N]; horizon = w_max - 1
  int32_t poly;
  const double *tab_dt, *tab_wp;
  // the Lambda of every problem of a solved set (include/mplx_scale.h; appended).  lam: 0 none, 1 REFERENCE, 2 ROBUST;
  // lam_n[N] segments (0: the problem is unscaled), lam_seg: field f of segment s at [(s * 8 + f) * N + k], lam_total[N]
  int32_t lam;
  const int32_t *lam_n;
  const double *lam_seg, *lam_total;
};
hipError_t launch_traj_chain(int dim, int control, const TrajArgs &a, hipStream_t s);
hipError_t launch_traj_sample(int dim, int form, const TrajArgs &a, hipStream_t s);
hipError_t launch_traj_traverse(int dim, int lanes, const TrajArgs &a, hipStream_t s);  // lanes in {4, 16, 64}

// ... and on the table of a solved set (a.poly == 1): efforts / waypoints, samples, traversal
hipError_t launch_poly_info(int dim, const TrajArgs &a, hipStream_t s);

// The batched trajectory solver (solve_kernel.hip, solve_api.cpp; include/mplx_solve.h): one lane per problem, a block
// tridiagonal LDL^T over the waypoints.  Everything is problem-minor: element (row, k) of an array at [row * stride + k].
struct SolveArgs {
  int64_t n_prob, cap;       // problems of this call; the stride of the poly's own arrays (its k_cap)
  int32_t w_max;
  int32_t so;                // 0 VEL, 1 ACC, 2 JRK: smoothing order of the ends' control
  // input
  const double *waypoints;   // [(f * w_max + w) * wp_stride + k]
  int64_t wp_stride;
  const int32_t *n_wp;       // [n_prob] or null: w_max each
  const double *dts;         // [(w_max - 1)][dt_stride] or null: allocate_time
  int64_t dt_stride;
  double v;
  const double *v_arr;       // [n_prob] or null: v
  const uint8_t *wp_flags;   // [w_max][flag_stride] use_pos 1 | use_vel 2 | use_acc 4, or null: setPath mode
  int64_t flag_stride;
  // the poly: segment table (TrajArgs with poly == 1, stride cap) and the workspace of the elimination
  int32_t *tab_S;
  uint8_t *tab_status;
  double *tab_T, *tab_tau, *tab_seg, *tab_dt, *tab_wp;
  double *ws;                // per waypoint h * h + h * D rows of cap doubles: Z = G'^-1 C, z = G'^-1 b
  // outputs, any may be null
  uint8_t *status;
  int32_t *n_segs;
  double *total_time, *coeff, *yaw_coeff, *dts_out, *taus_out;
  int64_t coeff_stride, yaw_stride, dts_out_stride, taus_stride;
};
hipError_t launch_solve(int dim, const SolveArgs &a, hipStream_t s);

// Caller-given segments into a poly's table, and the dynamic limits of the set a table holds (limits_kernel.hip,
// limits_api.cpp; include/mplx_limits.h).  The table is a TrajArgs with poly == 1 and stride n_prob.
struct PolyLoadArgs {
  int64_t n_prob;
  int32_t w_max;
  const int32_t *n_segs;     // [n_prob] or null: w_max - 1 each
  const double *dts;         // [w_max - 1][dt_stride]
  int64_t dt_stride;
  const double *coeff;       // [((s (D + 1) + a) 6 + j) * coeff_stride + k]
  int64_t coeff_stride;
  // the gather form: src_index non-null; the source table (stride src_n) holds src_n problems
  const int32_t *src_index;
  int64_t index_stride, src_n;
  const int32_t *src_S;
  const double *src_seg, *src_dt;
  int32_t *tab_S;
  uint8_t *tab_status;
  double *tab_T, *tab_tau, *tab_seg, *tab_dt, *tab_wp;
  // outputs, any may be null
  uint8_t *status;
  int32_t *n_segs_out;
  double *total_time, *taus_out;
  int64_t taus_stride;
};
hipError_t launch_poly_load(int dim, const PolyLoadArgs &a, hipStream_t s);

struct LimitsArgs {
  int64_t n_prob;            // the stride of the table and of seg_max
  int32_t s_max;             // w_max - 1 of the set
  int32_t control, all_roots;
  double mv, ma, mj;
  const int32_t *tab_S;
  const double *tab_seg, *tab_dt;
  double *seg_max;           // scratch [s_max][3 D][n_prob]: per segment the axis maxima of vel, acc, jrk
  // outputs, any may be null
  double *max_vel, *max_acc, *max_jrk;
  int64_t max_stride;
  uint8_t *exceed, *valid;
  int32_t *first_bad;
};
hipError_t launch_poly_limits(int dim, const LimitsArgs &a, hipStream_t s);

// Time scaling of the set a table holds (scale_kernel.hip, scale_api.cpp; include/mplx_scale.h).  Every array is
// problem-minor with stride n_prob unless it names its own.
struct ScaleArgs {
  int64_t n_prob;
  int32_t w_max;             // of the set: S_k <= w_max - 1
  int32_t robust;
  const int32_t *tab_S;
  const double *tab_T, *tab_tau, *tab_seg, *tab_dt;
  // the poly's Lambda table
  int32_t *lam_n;            // [n_prob]
  uint8_t *lam_status;       // [n_prob]
  double *lam_seg;           // [8][8][n_prob]
  double *lam_Ts;            // [w_max][n_prob]
  double *lam_total;         // [n_prob]
  // virtual points the build reads: the caller's, or the scratch rows a scale / scale_down launch filled
  const double *pts;         // [9][3][pts_stride]
  int64_t pts_stride;
  const int32_t *n_pts;      // [n_prob] or null: 9 each
  const uint8_t *only;       // [n_prob] or null; 0: this problem gets no Lambda and writes nothing
  // scale / scale_down: what fills the scratch points
  double ri, rf;
  const double *ri_arr, *rf_arr;
  double mv, ma;
  double *w_pts;             // [9][3][n_prob]
  int32_t *w_npts;           // [n_prob]
  uint8_t *w_scaled;         // [n_prob]
  double *down_seg;          // [w_max - 1][3][n_prob]: max_l (0: no record), t_lo, t_hi of a segment
  double *w_res;             // [3][n_prob]: max_l, t_lo, t_hi of a scaled problem
  uint8_t *scaled;
  double *max_l, *t_lo, *t_hi;
  // outputs of the build, any may be null
  uint8_t *status;
  int32_t *n_lseg;
  double *total, *Ts, *segs;
  int64_t ts_stride, seg_stride;
  // the inverse map: one lane per (problem, time)
  int32_t n_uniform;
  const double *times;
  int64_t time_stride, count;
  double *tau, *lam, *lam_dot;
  uint8_t *found;
  int64_t out_stride;
  // info on a scaled set: total_time[k] = lam_total[k] where the problem holds a Lambda
  double *total_time;
};
hipError_t launch_lambda_build(const ScaleArgs &a, hipStream_t s);
hipError_t launch_lambda_scale(const ScaleArgs &a, hipStream_t s);              // points of scale(ri, rf), then the build
hipError_t launch_lambda_scale_down(int dim, const ScaleArgs &a, hipStream_t s);  // records, points, then the build
hipError_t launch_lambda_tau(const ScaleArgs &a, hipStream_t s);
hipError_t launch_lambda_total(const ScaleArgs &a, hipStream_t s);

// Conflicts between the trajectories of one set (conflict_kernel.hip, conflict_api.cpp; include/mplx_conflict.h).  traj:
// the segment table (an action chain's or a poly's, with its Lambda).  Every scratch array is trajectory-minor.
struct ConflictArgs {
  TrajArgs traj;
  int64_t K;                 // traj.n_traj
  double step;
  int32_t n_steps, gone;     // gone: MPLX_CONFLICT_GONE
  const double *t0, *radius; // [K] or null
  double radius_all;
  const int32_t *group, *rank;  // [K] or null
  // scratch: what the init launch derives per trajectory, the accumulators, the positions of one chunk of instants
  uint8_t *m_incl, *m_status;   // [K] included; status bits
  double *m_r, *m_t0;           // [K]
  int32_t *m_group, *m_rank;    // [K] (k / 0 where the caller gave none)
  unsigned long long *acc_first, *acc_min;  // [K] (step << 32 | partner); the bit pattern of min d2
  double *pos;                  // [D][chunk][K]
  uint8_t *act;                 // [chunk][K]
  int32_t c0, cn, chunk;        // the chunk: instants c0 .. c0 + cn - 1; the stride `chunk` of pos / act
  // outputs, any may be null
  int32_t *first_step, *first_partner;
  double *min_d2;
  uint8_t *status;
  int32_t *pair_first;
  int64_t pair_stride;
};
hipError_t launch_conflict_init(const ConflictArgs &a, hipStream_t s);
hipError_t launch_conflict_chunk(int dim, const ConflictArgs &a, hipStream_t s);  // positions of the chunk, then the pairs
hipError_t launch_conflict_final(const ConflictArgs &a, hipStream_t s);
// the init launch and the position launch of ONE chunk (c0, cn, chunk), without the pairs: what a reservation table keeps
hipError_t launch_conflict_positions(int dim, const ConflictArgs &a, hipStream_t s);

// Reservation table and the check of successor lists against it (reserve_kernel.hip, reserve_api.cpp;
// include/mplx_reserve.h).  The table is what launch_conflict_positions left: pos [D][n_steps][B], act [n_steps][B].
struct ReserveArgs {
  const double *pos;
  const uint8_t *act;
  const uint8_t *incl;          // [B]
  const double *r;              // [B]
  const int32_t *group;         // [B]
  int64_t B;
  int32_t n_steps;
  double step;
  // the queries
  const double *q_t0, *q_r;     // [Q]
  const int32_t *q_ignore;      // [Q]
  int32_t Q;
  const int32_t *node_query;    // per node of the table its query, or null: every row is query 0
  int64_t node_cap;             // entries of node_query
  // the lists and their parents
  const int32_t *count, *action;
  double *cost;
  int64_t n_rows, S;
  const int32_t *parent_id;
  const double *parent_state;   // [4D+2][parent_stride]
  int64_t parent_stride;
  const double *U;
  int32_t nU, udim;
  double dt;
  int32_t n_scan;               // ceil(dt / step) + 3: the instants a row looks through
  int32_t sp_log2;              // 2^sp_log2 lanes of a wave over a row's entries, the 64 >> sp_log2 groups split the reservations
  // outputs, either may be null
  long long *hit;               // [n_rows * S]
  unsigned long long *n_blocked;
};
hipError_t launch_reserve_check(int dim, int control, const ReserveArgs &a, hipStream_t s);

// Park-safe goals (reserve_kernel.hip; mplx_reserve_park_device of include/mplx_reserve.h): the goal-region rows of a
// pushed frontier against the table from the row's t on.  The table and query fields of `res` are used; its lists are not.
struct ParkArgs {
  ReserveArgs res;
  const int32_t *t_n_nodes;     // the open set's table: its node count (TableCtl::n_nodes, device memory)
  uint8_t *flags;               // the open set's flags, [node capacity]
  const int32_t *f_id;          // the frontier
  const double *f_state;        // [4D+2][f_stride]
  int64_t f_stride, f_cap;
  const int64_t *f_count;
  int64_t n_max;
  int32_t n_scan;               // instants looked through for the first one at or after a row's t
  long long *hit;               // [f_cap] or null
  unsigned long long *n_vetoed; // or null
};
hipError_t launch_reserve_park(int dim, const ParkArgs &a, int64_t rows, hipStream_t s);

// Polynomial trajectories against a reservation table (reserve_poly_kernel.hip, reserve_poly_api.cpp;
// include/mplx_reserve_poly.h).  The table fields of `res` are used (and its query fields by the pair rows); traj: the
// segment table of the poly, with its Lambda.
struct ReservePolyArgs {
  ReserveArgs res;
  TrajArgs traj;
  int64_t K;                    // traj.n_traj
  const double *t_start;        // [K]
  const double *radius;         // [K] or null: radius_all
  double radius_all;
  const int32_t *ignore;        // [K] or null: -1
  // outputs, any may be null
  long long *hit;               // [K]
  uint8_t *status;              // [K]
  unsigned long long *n_hit;
};
hipError_t launch_reserve_check_poly(int dim, const ReservePolyArgs &a, hipStream_t s);

// The [P] rows of a timed shortcut's pair set, one lane per pair p = (k (w_max - 1) + i) max_hop + h:
// t_start = q_t0[k] + t_i, radius = q_r[k], ignore = q_ignore[k].
struct PairRowsArgs {
  int64_t n_query;
  int32_t w_max, max_hop;
  const double *t_row;          // the t row of the chain states: [w_max][stride]
  int64_t stride;
  const double *q_t0, *q_r;     // [Q]
  const int32_t *q_ignore;      // [Q]
  double *t_start, *radius;     // [P]
  int32_t *ignore;              // [P]
};
hipError_t launch_reserve_pair_rows(const PairRowsArgs &a, hipStream_t s);

// Wait edges (wait_kernel.hip, wait_api.cpp; include/mplx_wait.h): one lane per list row appends the zero control's entry.
struct WaitArgs {
  ExpandArgs env;               // parameters and controls as expand_args() fills them; map, nodes and slots unused
  int32_t a0;                   // the zero row of the control table
  int32_t *count, *action;
  double *cost;
  uint64_t *hash;
  double *state;
  int64_t state_stride;
  int32_t *iters;
  int64_t n_rows, S;
  const int32_t *parent_id;     // or null
  const double *parent_state;   // [4D+2][parent_stride]
  int64_t parent_stride;
  PostFuse post;                // goal of mplx_set_goal; heur / flags = the lists' rows or null
  unsigned long long *n_added;  // or null
};
hipError_t launch_lists_add_wait(int dim, int control, const WaitArgs &a, hipStream_t s);

// Shortcutting (include/mplx_limits.h): the pair problems of Q chains, and the dynamic programme over their costs.
struct ShortcutArgs {
  int64_t n_query;
  int32_t w_max, max_hop, order;  // order: 1 VEL, 2 ACC, 3 JRK
  double w;                       // the context's time weight
  const double *states;           // [(f w_max + w) * stride + k]
  int64_t stride;
  const int32_t *n_wp;            // [Q] or null
  // pair problems, P = Q (w_max - 1) max_hop, every array [row][P]
  double *pair_wp;                // [4D+2][2][P]
  double *pair_dt;                // [1][P]
  int32_t *pair_nwp;              // [P] 2 or 0
  uint8_t *pair_flags;            // [2][P]
  // what the evaluation of the pairs left
  const uint8_t *pair_status, *pair_valid;
  const double *pair_T, *pair_effort, *pair_trav;  // effort [5][P]
  // the programme
  double *dist;                   // [w_max][Q]
  int32_t *pred;                  // [w_max][Q]
  int32_t *src_index;             // [w_max - 1][Q]
  uint8_t *status;
  int32_t *n_keep, *keep;
  int64_t keep_stride;
  double *cost, *chain_cost, *edge_cost;
  // the timed shortcut (include/mplx_reserve_poly.h; appended), both null without a reservation table
  const long long *pair_hit;      // [P] hit of the pair set's check: a non-adjacent edge needs -1
  long long *chain_hit;           // [Q] or null
};
hipError_t launch_shortcut_pairs(int dim, const ShortcutArgs &a, hipStream_t s);
hipError_t launch_shortcut_dp(const ShortcutArgs &a, hipStream_t s);

// The prior table of an open set (traj_kernel.hip, open_api.cpp; include/mplx_prior.h), built on the segment table of a
// chain launch with the prior's controls and the `cost` of a traverse launch.
struct PriorArgs {
  TrajArgs traj;           // env (the searching context's but U / nU / udim / dt: the prior's), n_traj, the segment table
  double dt;               // the searching context's dt
  const double *traverse;  // [n_traj] cost of launch_traj_traverse
  // scratch: per sample of a trajectory its cell index and its term of the potential sum
  int32_t *s_idx;          // [n_traj][s_cap]
  double *s_term;          // [n_traj][s_cap]
  double *costs;           // [n_traj][k_cap]
  int64_t s_cap, k_cap;
  // the table
  int32_t *n_steps;        // [n_traj]
  double *pos, *togo;      // [n_traj][k_cap][D], [n_traj][k_cap]
  uint8_t *status;         // [n_traj] MPLX_TRAJ_* bits
  // goals: the open set's (goals0: as mplx_open_set_goals left them), and the effective rows for the view
  const PostFuse *goals0;
  PostFuse *goals;
  double *goal_row;        // [n_traj][14]
  uint64_t *goal_hash;     // [n_traj]
};
hipError_t launch_prior_build(int dim, int control, const PriorArgs &a, hipStream_t s);

// Persistent node table (table_kernel.hip, table_api.cpp; include/mplx_table.h).
struct TableSlot { uint64_t key; int32_t id; uint32_t first_e; };  // all bytes 0xff: empty, no id, no claimant
struct TableCtl {      // device memory
  int32_t n_nodes;     // nodes in the table
  int32_t base;        // ... before the call in flight (the ids of its new nodes start here)
  uint32_t status;     // MPLX_TABLE_* bits, sticky
  int32_t emit;        // the call in flight got as far as its frontier
};
struct TableMirror { int64_t n_nodes; uint32_t status; };  // pinned host memory: what the last finished call left in TableCtl
struct TableArgs {
  // the table: n_queries regions of q_slots (a power of two) slots, n_slots in all, then one slot per query for the hash
  // equal to the empty marker.  One query: a single region, n_slots + 1 slots
  TableSlot *slots;
  uint64_t n_slots, q_slots;
  int32_t n_queries;
  int32_t *query;            // per node its query; null for a table of one query (no kernel then looks a query up)
  const int32_t *src_query;  // seeds of a table with several queries: the query per entry; a relax takes query[parent_id[k]]
  uint64_t *hash;
  unsigned long long *g;     // the doubles' bit patterns: non-negative doubles order like uint64 (atomicMin)
  int32_t *pred, *pred_action;
  double *state;             // [n_fields][cap]
  unsigned long long *pick;  // per node (tag << 32 | e): improved in the call `tag` belongs to, by entry e at the earliest
  int64_t cap;
  int32_t n_fields;
  uint32_t tag;              // 0xffffffff - epoch of the call: later calls carry SMALLER tags, so atomicMin prefers them
  TableCtl *ctl;
  TableMirror *mirror;
  // the entries: n_rows lists of S entries.  Seeds: S = 1, count / action / cost / parent_id null (cand = parent_g[k], or 0)
  const int32_t *count, *action;
  const double *cost;
  const uint64_t *src_hash;
  const double *src_state;
  int64_t src_sstride;
  int64_t n_rows, S;
  const int32_t *parent_id;
  const double *parent_g;
  double g_max;
  // scratch of the table: per entry its slot, then its node id; per entry a mark; per tile of 4096 entries a count
  uint32_t *ent;
  uint8_t *mark;
  uint32_t *tot;
  int64_t n_tiles;
  // outputs
  int32_t *f_id;
  double *f_g, *f_state;
  int64_t f_stride, f_cap;
  int64_t *f_count;
  int32_t *entry_id;  // or null
};
constexpr int kTableTile = 4096;
hipError_t launch_table_relax(const TableArgs &a, hipStream_t s);
hipError_t launch_table_clear(const TableArgs &a, hipStream_t s);  // slots, control block and mirror
hipError_t launch_table_hash(int dim, int control, const double *states, int64_t n, int64_t stride, uint64_t *hash, hipStream_t s);
// time keys (mplx_table_set_time_keys): key[e] = hash_combine(hash[e], (int)round(t[e] / 0.1)) for the entries within
// their count (count null: all n); key may be hash (in place)
hipError_t launch_table_time_keys(const int32_t *count, int64_t S, int64_t n, const uint64_t *hash, const double *t, uint64_t *key,
                                  hipStream_t s);
// query: per hash its query (outside [0, n_queries): -1), or null on a table of one query
hipError_t launch_table_find(const TableArgs &a, const uint64_t *hash, const int32_t *query, int64_t n, int32_t *id, hipStream_t s);
// leaf first: ids[0 .. len], actions[0 .. len); *len < 0: -1 more than cap edges, -2 bad id, -3 no seed within n_nodes steps
hipError_t launch_table_path(const TableArgs &a, int32_t id, int32_t *ids, int32_t *actions, int64_t cap, int64_t *len, hipStream_t s);

// Open set of a node table (open_kernel.hip, open_api.cpp; include/mplx_open.h).
struct OpenResult { int32_t status, goal_id; int64_t count, n_open; double f_min, goal_f, goal_g; };  // mplx_open_result
struct OpenCtl {                   // device memory; two of them, used by alternate selects: a select's scan resets the other
  unsigned long long fmin_bits;    // min over the open nodes of f's bit pattern (+inf: none)
  unsigned long long goalf_bits;   // ... over the goal-region nodes
  uint32_t n_open, n_goal;
  int32_t goal_id;                 // smallest id among the goal-region nodes with f == goal_f (INT32_MAX: none yet)
  int32_t emit;                    // the select in flight is SELECTED and got as far as its frontier
  uint32_t n_sel;                  // select_multi: rows of this query below the frontier's capacity (the emit pass counts)
  uint32_t pad;
};
struct OpenArgs {
  // the table (read only)
  const TableCtl *t_ctl;
  const uint64_t *t_hash;
  const unsigned long long *t_g;
  const double *t_state;           // [n_fields][cap]
  const int32_t *t_query;          // per node its query; null for a table of one query
  int32_t n_queries;
  int64_t cap;
  int32_t n_fields;
  // the open set
  unsigned long long *f;           // the doubles' bit patterns: non-negative doubles order like uint64
  uint8_t *flags;
  OpenCtl *ctl, *ctl_next;
  OpenResult *mirror;              // pinned host memory: the result of the last finished select
  int64_t n_bound;                 // host-known upper bound of the table's n_nodes: sizes the grids
  // push: rows [0, min(*f_count, n_max, f_cap)) of the frontier; row_flags != null: the two-pass form around the ray trace
  int64_t n_max;
  double eps;
  PostFuse goal;                   // goal of mplx_set_goal (output pointers unused)
  const PostFuse *goals;           // mplx_open_set_goals: [n_queries] in device memory, or null: `goal`
  int32_t *row_query;              // [rows] with goals and row_flags: the query of every row, for the per-row ray trace
  uint8_t *row_flags;              // [rows] bit 0 inside the tolerances, bit 3 ray blocked (goal_trace_kernel), bit 7 the row counts
  int32_t *row_count;              // [rows] all 1: the frontier as lists of stride 1
  // select
  double delta;
  uint8_t *mark;                   // [n_bound]
  uint32_t *tot;                   // [n_tiles]
  int64_t n_tiles;
  OpenResult *result;              // device memory of the caller, or null
  // the frontier: read by push, written by select
  int32_t *f_id;
  double *f_g, *f_state;
  int64_t f_stride, f_cap;
  int64_t *f_count;
  // push with priors (include/mplx_prior.h; appended: every field above keeps its place): null = no prior in force
  const int32_t *prior_n;          // [n_queries] steps per query, 0 = none
  const double *prior_pos;         // [n_queries][prior_cap][D]
  const double *prior_togo;        // [n_queries][prior_cap]
  int64_t prior_cap;
  double prior_dt;                 // the searching context's dt
  // push with a goal field (include/mplx_field.h; appended): null = no field in force
  const int32_t *field_dist;       // [F][field_cells]
  const int32_t *field_of_query;   // [n_queries] in device memory: the field of a query, or -1
  int32_t field_F;
  int64_t field_cells;
  int32_t field_dim[3];
  double field_org[3], field_res;
  // push with the dynamics-aware heuristic (include/mplx_heur.h; appended): dyn == 0 = the default heuristic
  int32_t dyn;                     // MPLX_HEUR_ROBUST, or 0
  int32_t dyn_control[2];          // control and goal_control of `goal`
  const int32_t *dyn_controls;     // [n_queries][2] in device memory: those of `goals`
};

// The dynamics-aware heuristic of a batch of resident states (heur_kernel.hip, heur_api.cpp; include/mplx_heur.h).
struct HeurArgs {
  const double *states;            // [4D+2][stride]
  int64_t n, stride;
  double *out;                     // [n]
  double goal[14];                 // the goal waypoint's rows
  uint64_t goal_hash;              // under the goal's own flag
  int32_t control, goal_control;   // the states' flag; the goal's, 0 = the states'
  int32_t mode;                    // MPLX_HEUR_DEFAULT or MPLX_HEUR_ROBUST
  double w, v_max;
};
hipError_t launch_heur_eval(int dim, const HeurArgs &a, hipStream_t s);

// Goal distance fields (field_kernel.hip, field_api.cpp; include/mplx_field.h).  Tiles: 32 x 32 cells in 2-D, 8 x 8 x 8 in 3-D.
struct FieldArgs {
  int32_t *dist;                   // [F][n_cells]
  const uint32_t *blk;             // the context's blocked-bit map
  const int32_t *box;              // [F][6]: lo[3], hi[3], clipped to the map (lo > hi on an axis: no seed)
  int32_t F, dim;
  int32_t mdim[3];
  int32_t tiles[3];                // tiles per axis
  int64_t n_cells, n_tiles;        // n_tiles = tiles[0] * tiles[1] * tiles[2]
  uint8_t *active_cur, *active_next;  // [F * n_tiles] each: a byte per (field, tile)
  unsigned long long *counter;     // (field, tile)s that marked a neighbour, summed over the passes so far
};
constexpr int kFieldTile2 = 32, kFieldTile3 = 8;
// blocked bits of a context WITH a potential map, for the field: value >= 100 (env_map.h:117), outside the region, padding
hipError_t launch_field_pot_bits(const int8_t *pot, const uint32_t *region, int64_t n_cells, uint32_t *out, hipStream_t s);
hipError_t launch_field_init(const FieldArgs &a, hipStream_t s);
hipError_t launch_field_pass(const FieldArgs &a, hipStream_t s);
hipError_t launch_open_clear(const OpenArgs &a, hipStream_t s);  // ctl: 2 * n_queries control blocks
// closed: the push of include/mplx_replan.h -- the rows get SEEN (and IS_GOAL) but not IS_OPEN
hipError_t launch_open_push(int dim, int pass, const OpenArgs &a, int64_t rows, hipStream_t s, bool closed = false);  // pass 0: all (or up to the row flags); 1: after the ray trace
hipError_t launch_open_select(const OpenArgs &a, hipStream_t s);
// select_multi: ctl / ctl_next / mirror / result are arrays of n_queries
hipError_t launch_open_select_multi(const OpenArgs &a, hipStream_t s);

// The k best open nodes per query (open_best_kernel.hip; include/mplx_best.h): a radix select over the keys' bit patterns
// between the reduce pass and the tail (scan, emit, finish) of select_multi, which it shares with open_kernel.hip.
constexpr int kBestBits = 8, kBestPasses = 8, kBestBins = 1 << kBestBits;  // 8 digits of 8 bits: the 64 bits of a key
constexpr int kBestSeg = 1024;                                            // ids a wave ranks in order: kTableTile / 4
struct BestState { uint32_t live, shift, krem, pad; unsigned long long prefix, pad2; };  // what a pass histograms with
struct BestFinal { uint32_t valid, all, sh, ties; unsigned long long F, pad; };          // the threshold of a query
struct BestArgs {
  OpenArgs o;                      // as for select_multi
  uint32_t k;                      // clamped to INT32_MAX by the host
  // the scratch of the open set, zeroed in front of every best-select
  uint32_t *active;                // [kBestPasses] a query histogrammed in that pass; [kBestPasses]: a node lies at a threshold
  BestFinal *fin, *fin2;           // [n_queries] found by a histogram pass; by the classify pass from the last histogram
  BestState *state;                // [kBestPasses][n_queries]
  uint32_t *hist;                  // [kBestPasses][n_queries][kBestBins]
  uint32_t *eqc;                   // [n_queries][seg_stride] nodes at the threshold per segment of kBestSeg ids, then their ranks
  int64_t seg_stride;
};
inline size_t best_scratch_bytes(int64_t n_queries, int64_t cap) {
  const size_t Q = (size_t)n_queries, segs = ((size_t)cap + kTableTile - 1) / kTableTile * (kTableTile / kBestSeg);
  return 64 + Q * (2 * sizeof(BestFinal) + kBestPasses * (sizeof(BestState) + kBestBins * 4) + segs * 4);
}
hipError_t launch_open_reduce_only(const OpenArgs &a, bool multi, hipStream_t s);  // the first launch of a select
hipError_t launch_open_tail_multi(const OpenArgs &a, hipStream_t s);               // scan, emit and finish of select_multi
hipError_t launch_open_best(const BestArgs &b, hipStream_t s);                     // histograms, classify, rank, pick

// Re-key of an open set and the lower bound of its open nodes (open_rekey_kernel.hip; include/mplx_anytime.h).
struct OpenBound { double lower; int64_t n_open, n_pruned, n_rekeyed; };  // mplx_open_bound
struct RekeyCtl {                  // device memory, one per query; reset by the first launch of every re-key
  unsigned long long lower_bits;   // min over the open nodes of the bit pattern of g + h (+inf: none)
  unsigned long long n_open, n_pruned, n_rekeyed;
};
struct RekeyArgs {
  OpenArgs o;                      // the table, f, flags, eps and the heuristic's modes as for a push (no frontier)
  int32_t write;                   // 0: the bound alone
  const double *cut;               // [n_queries] in device memory, or null: nothing is pruned
  RekeyCtl *rctl;                  // [n_queries]
  OpenBound *d_bound;              // [n_queries] device memory of the caller, or null
  OpenBound *mirror;               // [n_queries] pinned host memory
};
hipError_t launch_open_rekey(int dim, const RekeyArgs &r, hipStream_t s);  // reset, re-key, finish

// Re-rooting and repair of a node table after a map edit (replan_kernel.hip, replan_api.cpp; include/mplx_replan.h).
struct ReplanResult { int64_t n_kept, n_bad_edges, n_roots; };  // mplx_rebase_result
struct ReplanArgs {
  ExpandArgs env;            // map, potential, region, parameters and controls as expand_args() fills them (check_edges only)
  int32_t band;              // 1: a heading-limit decision within env.yaw.margin of its threshold makes the edge bad
  int32_t check_edges;
  // the table
  TableCtl *ctl;
  TableMirror *mirror;
  const uint64_t *hash;
  unsigned long long *g;
  int32_t *pred, *pred_action;
  const double *state;       // [n_fields][cap]
  const int32_t *query;      // per node its query; null for a table of one query
  int32_t n_queries, n_fields;
  int64_t cap;
  int64_t n_bound;           // host-known upper bound of n_nodes: sizes the grids and the number of resolve passes
  // the roots: root_of_query ([n_queries], device memory) or, when it is null, root_id for the one query
  int32_t root_id;
  const int32_t *root_of_query;
  // scratch of the table, sized by its capacity
  uint8_t *bad;              // [cap] the edge (pred, pred_action) of a non-root node no longer holds
  uint8_t *dec[2];           // [cap] each: 0 unknown, 1 keep, 2 drop; a resolve pass reads one and writes the other
  int32_t *jump[2];          // [cap] each: the ancestor an unknown node looks at next
  uint8_t *mark;             // [cap] kept
  uint32_t *tot;             // [n_tiles] kept nodes per tile of kTableTile ids, then their exclusive prefix sums
  int64_t n_tiles;
  ReplanResult *counters;    // zero before the call: the result, summed by order-free integer atomics
  // the frontier of kept nodes
  int32_t *f_id;
  double *f_g, *f_state;
  int64_t f_stride, f_cap;
  int64_t *f_count;
};
hipError_t launch_replan_rebase(int dim, int control, const ReplanArgs &a, int passes, hipStream_t s);
// The timed rebase (include/mplx_replan_timed.h): the rebase above with the edge pass's key fold and wait rule, and with
// the kept edges tested against a reservation table.  A struct of its own: the launches of the untimed rebase take the
// arguments they took.
struct ReplanTimedArgs {
  ReplanArgs R;              // check_edges: the edge pass runs
  int32_t time_keys;         // the hash column holds mplx_time_key(h_next, tp + dt)
  int32_t allow_wait;
  int32_t a0;                // the zero action of include/mplx_wait.h, or -1: the control table has none
  int32_t use_res;           // the reservation pass runs: the table, query, control and scan fields of `res`
  ReserveArgs res;           // (its lists are not used)
  long long *hit;            // [node capacity] or null
  unsigned long long *n_blocked;  // or null
};
hipError_t launch_replan_rebase_timed(int dim, int control, const ReplanTimedArgs &a, int passes, hipStream_t s);
// table_kernel.hip: the scan of tile counts tot[n_tiles] in place, the frontier count (FRONTIER_FULL when it exceeds
// f_cap), ctl->emit and the pinned mirror -- the second scan of a relax, for a pass that marked per tile itself
hipError_t launch_table_scan_frontier(const TableArgs &a, hipStream_t s);

// Element-wise math probe (see mplx_selftest_math in mplx.h).
hipError_t launch_math_probe(int op, const double *a, const double *b, double *out, int64_t n,
                             hipStream_t stream);

// Packs a byte-per-cell mask into 1 bit per cell (word = cell >> 5).
hipError_t launch_pack_region(const uint8_t *bytes, uint32_t *bits, int64_t n_cells,
                              hipStream_t stream);

}  // namespace mplx
#endif
