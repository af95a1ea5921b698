// field_api.cpp -- C ABI of include/mplx_field.h: the goal distance fields of a context (field_kernel.hip).  The dist
// array, the two active maps and the pass counter are the field's own; the boxes are staged through the context's arena
// (mplx_field_build is a host-pointer call and follows its rules).  The open set's side of the header is in open_api.cpp.
#include "mplx_ctx.h"
#include "../../include/mplx_field.h"

#include <algorithm>
#include <vector>

using namespace mplx_detail;

extern "C" {

int mplx_field_create(mplx_ctx *c, mplx_field **out) {
  if (!c) return MPLX_ERR_ARG;
  if (!out) return fail(c, MPLX_ERR_ARG, "mplx_field_create: NULL out");
  *out = nullptr;
  MPLX_GUARD_BEGIN
  mplx_field *fld = new mplx_field;
  fld->c = c;
  fld->epoch = c->blk_epoch;
  *out = fld;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

void mplx_field_destroy(mplx_field *fld) {
  if (!fld) return;
  (void)hipSetDevice(fld->c->device);
  (void)hipStreamSynchronize(fld->c->stream);
  for (mplx_open *o : fld->users) open_field_gone(o);  // (a push with a destroyed field is an error, not a read of freed memory)
  for (DevBuf *b : {&fld->dist, &fld->active, &fld->counter, &fld->bits}) release(*b);
  delete fld;
}

int mplx_field_build(mplx_field *fld, int32_t F, const int32_t *h_lo, const int32_t *h_hi) {
  if (!fld) return MPLX_ERR_ARG;
  mplx_ctx *c = fld->c;
  const char *who = "mplx_field_build";
  if (F < 0 || (F > 0 && (!h_lo || !h_hi))) return fail(c, MPLX_ERR_ARG, "%s: need F >= 0 and the boxes lo, hi [F][D]", who);
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "%s: set the map first", who);
  if (F > 0 && c->n_cells > MPLX_FIELD_MAX_BYTES / 4 / F)
    return fail(c, MPLX_ERR_ARG, "%s: %d fields of %lld cells exceed MPLX_FIELD_MAX_BYTES", who, (int)F, (long long)c->n_cells);
  MPLX_GUARD_BEGIN
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  fld->F = 0;  // (a failure below leaves an empty field)
  fld->passes = 0;
  fld->n_cells = c->n_cells;
  fld->epoch = c->blk_epoch;
  if (F == 0) return MPLX_OK;
  // without a potential map: the bits the expansion reads.  With one those are a pre-screen (value > 0); the field's own
  // say what ends a primitive (value >= 100): field_kernel.hip
  if (!c->has_pot) {
    if (int rc = ensure_blocked_bits(c)) return rc;
  } else if (int rc = ensure(c, fld->bits, (size_t)((c->n_cells + 31) >> 5) * 4)) {
    return rc;
  }
  const int D = c->dim;
  mplx::FieldArgs a{};
  a.F = F;
  a.dim = D;
  a.n_cells = c->n_cells;
  const int ts = D == 2 ? mplx::kFieldTile2 : mplx::kFieldTile3;
  a.n_tiles = 1;
  for (int i = 0; i < 3; i++) {
    a.mdim[i] = c->mdim[i];
    a.tiles[i] = i < D ? (c->mdim[i] + ts - 1) / ts : 1;
    a.n_tiles *= a.tiles[i];
  }
  // the boxes, clipped to the map; an axis with lo > hi after the clip: no seed
  std::vector<int32_t> box((size_t)F * 6, 0);
  for (int32_t f = 0; f < F; f++)
    for (int i = 0; i < D; i++) {
      box[(size_t)f * 6 + i] = std::max<int32_t>(h_lo[(size_t)f * D + i], 0);
      box[(size_t)f * 6 + 3 + i] = std::min<int32_t>(h_hi[(size_t)f * D + i], c->mdim[i] - 1);
    }
  const size_t cells = (size_t)F * (size_t)c->n_cells, ft = (size_t)F * (size_t)a.n_tiles, half = align256(ft);
  if (int rc = ensure(c, fld->dist, cells * 4)) return rc;
  if (int rc = ensure(c, fld->active, 2 * half)) return rc;
  if (int rc = ensure(c, fld->counter, 8)) return rc;
  StageRows s;  // (no output row: every pass below ends in its own read-back and synchronise)
  const auto i_box = s.in(box.data(), box.size() * 4);
  if (int rc = stage_commit(c, &s)) return rc;
  HIP_TRY(c, hipMemsetAsync(fld->active.p, 0, 2 * half, c->stream));
  HIP_TRY(c, hipMemsetAsync(fld->counter.p, 0, 8, c->stream));
  a.dist = (int32_t *)fld->dist.p;
  a.blk = (const uint32_t *)(c->has_pot ? fld->bits.p : c->blk.p);
  if (c->has_pot)
    HIP_TRY(c, mplx::launch_field_pot_bits((const int8_t *)c->pot.p, c->has_region ? (const uint32_t *)c->region_bits.p : nullptr, c->n_cells,
                                           (uint32_t *)fld->bits.p, c->stream));
  a.box = s.dev<int32_t>(i_box);
  a.counter = (unsigned long long *)fld->counter.p;
  uint8_t *act[2] = {(uint8_t *)fld->active.p, (uint8_t *)fld->active.p + half};
  a.active_cur = act[0];
  a.active_next = act[1];
  HIP_TRY(c, mplx::launch_field_init(a, c->stream));
  unsigned long long seen = 0, now = 0;
  int64_t pass = 0;
  for (;; pass++) {
    if (pass > c->n_cells + 1) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      return fail(c, MPLX_ERR_STATE, "%s: no fixed point within %lld passes", who, (long long)pass);
    }
    a.active_cur = act[pass & 1];
    a.active_next = act[1 - (pass & 1)];
    HIP_TRY(c, mplx::launch_field_pass(a, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&now, fld->counter.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the pass's only read-back
    if (now == seen) break;  // no tile marked a neighbour: the next pass would have nothing to do
    seen = now;
  }
  fld->passes = pass + 1;
  fld->F = F;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

int mplx_field_shape(mplx_field *fld, int32_t *F, int64_t *n_cells) {
  if (!fld) return MPLX_ERR_ARG;
  if (F) *F = fld->F;
  if (n_cells) *n_cells = fld->F ? fld->n_cells : 0;
  return MPLX_OK;
}

int mplx_field_view_of(mplx_field *fld, mplx_field_view *v) {
  if (!fld) return MPLX_ERR_ARG;
  if (!v) return fail(fld->c, MPLX_ERR_ARG, "mplx_field_view_of: NULL view");
  *v = mplx_field_view{};
  if (!fld->F) return MPLX_OK;
  v->dist = (const int32_t *)fld->dist.p;
  v->F = fld->F;
  v->n_cells = fld->n_cells;
  return MPLX_OK;
}

int mplx_field_download(mplx_field *fld, int32_t *h_dist) {
  if (!fld) return MPLX_ERR_ARG;
  mplx_ctx *c = fld->c;
  if (!fld->F) return MPLX_OK;
  if (!h_dist) return fail(c, MPLX_ERR_ARG, "mplx_field_download: NULL dist");
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, hipMemcpyAsync(h_dist, fld->dist.p, (size_t)fld->F * (size_t)fld->n_cells * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

int mplx_field_is_stale(mplx_field *fld) {
  if (!fld) return MPLX_ERR_ARG;
  return fld->epoch != fld->c->blk_epoch ? 1 : 0;
}

int mplx_field_passes(mplx_field *fld, int64_t *passes) {
  if (!fld || !passes) return MPLX_ERR_ARG;
  *passes = fld->passes;
  return MPLX_OK;
}

}  // extern "C"
