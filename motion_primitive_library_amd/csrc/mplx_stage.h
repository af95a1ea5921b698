// mplx_stage.h -- the layout of the rows a host-pointer call stages: offsets, sizes and host sides, no HIP.  mplx_ctx.h
// includes it and adds the copies (stage_commit, stage_fetch) and the rules of the arena the rows are carved from.
#ifndef MPLX_STAGE_H
#define MPLX_STAGE_H

#include <cstddef>
#include <cstdint>

namespace mplx_detail {

inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }  // the only rounding of staging offsets

// The raw layer: offsets only.  For a buffer the caller owns ("only the carving") and for the lists paths, whose control
// flow is not "copy in, launch, copy out, synchronise".
struct StageLayout {
  size_t total = 0;
  char *base = nullptr;       // the arena, once committed
  // offset of a row of `bytes` (0: a row that was not asked for; the caller leaves its pointer null)
  size_t add(size_t bytes) { const size_t at = total; total += align256(bytes); return at; }
};

// The rows of one host-pointer call, each declared ONCE: the declaration fixes the row's bytes, whether it exists (a null
// host pointer or 0 bytes: it was not asked for, and costs neither arena bytes nor a copy), its direction and its host
// side.  Offsets are StageLayout's, in declaration order.  stage_commit() carves and copies the inputs in, dev() gives
// the device side for the `in` / `out` structs of the _device launch (null for a row that was not asked for),
// stage_fetch() copies the outputs out and synchronises, host() gives the landing buffer of a landed row for the
// call's own scatter loop.  The object lives on the stack of the call and nothing keeps a pointer into it or the arena.
struct StageRows {
  struct Row { int i; };  // handle of a declared row
  static constexpr int kMaxRows = 24;
  struct Rec {
    size_t bytes = 0, at = 0;            // arena bytes and offset (bytes == 0: no arena row)
    const void *src = nullptr;           // host source (inputs, in-out)
    void *dst = nullptr;                 // host destination (outputs, in-out)
    const void *from = nullptr;          // landed row read from device memory outside the arena
    size_t width = 0, rows = 0, pitch = 0;  // pitch != 0: `rows` host rows of `width` bytes, `pitch` bytes apart
    size_t land = 0, land_at = 0;        // bytes and offset in the landing block (land == 0: not landed)
  };
  Rec rec[kMaxRows];
  int n = 0;
  bool overflow = false;
  StageLayout l;
  size_t land_total = 0;
  char *landing = nullptr;  // one host block for all landed rows of the call
  StageRows() = default;
  StageRows(const StageRows &) = delete;
  StageRows &operator=(const StageRows &) = delete;
  ~StageRows() { ::operator delete(landing); }

  // -- inputs
  Row in(const void *host, size_t bytes) { return add(host ? bytes : 0, host, nullptr); }
  // ... `rows` host rows of `width` bytes, `src_stride` bytes apart, packed to `width` on the device
  Row in_rows(const void *host, size_t src_stride, size_t width, size_t rows) {
    const Row r = add(host ? width * rows : 0, host, nullptr);
    if (rec[r.i].bytes) { rec[r.i].width = width; rec[r.i].rows = rows; rec[r.i].pitch = src_stride; }
    return r;
  }
  // -- outputs copied straight to the caller
  Row out(void *host, size_t bytes) { return add(host ? bytes : 0, nullptr, host); }
  Row out_rows(void *host, size_t dst_stride, size_t width, size_t rows) {
    const Row r = add(host ? width * rows : 0, nullptr, host);
    if (rec[r.i].bytes) { rec[r.i].width = width; rec[r.i].rows = rows; rec[r.i].pitch = dst_stride; }
    return r;
  }
  // ... a row the launch writes whether or not the caller asked for it
  Row out_or_scratch(void *host, size_t bytes) { return add(bytes, nullptr, host); }
  // -- copied in before the launch and out after it
  Row inout(void *host, size_t bytes) { return add(host ? bytes : 0, host, host); }
  // -- device only
  Row scratch(size_t bytes) { return add(bytes, nullptr, nullptr); }
  // -- landed: copied to the landing block, for the call to scatter under its own mask (`asked` null: not asked for)
  Row landed(size_t bytes) { return land(add(bytes, nullptr, nullptr), bytes); }
  Row landed(const void *asked, size_t bytes) { return landed(asked ? bytes : 0); }
  Row landed_or_scratch(const void *asked, size_t bytes) { return land(add(bytes, nullptr, nullptr), asked ? bytes : 0); }
  // ... from device memory that is not in the arena (no arena bytes); `dev` is the address at the declaration: the
  // buffer must exist by then
  Row landed_from(const void *dev, size_t bytes) {
    const Row r = land(add(0, nullptr, nullptr), bytes);
    rec[r.i].from = dev;
    return r;
  }

  size_t total() const { return l.total; }
  template <class T> T *dev(Row r) const { return rec[r.i].bytes ? (T *)(l.base + rec[r.i].at) : nullptr; }
  template <class T> const T *host(Row r) const { return rec[r.i].land ? (const T *)(landing + rec[r.i].land_at) : nullptr; }

 private:
  Row add(size_t bytes, const void *src, void *dst) {
    if (n == kMaxRows) { overflow = true; return Row{kMaxRows - 1}; }
    Rec &r = rec[n];
    r.bytes = bytes; r.at = l.add(bytes);
    if (bytes) { r.src = src; r.dst = dst; }
    return Row{n++};
  }
  Row land(Row r, size_t bytes) {
    rec[r.i].land = bytes;
    rec[r.i].land_at = land_total;
    land_total += (bytes + 15) & ~(size_t)15;
    return r;
  }
};

}  // namespace mplx_detail
#endif
