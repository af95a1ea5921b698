// The row layout of csrc/mplx_stage.h on the host alone: StageRows gives every row the offset the raw StageLayout gives
// the same sizes, a row that was not asked for takes neither arena bytes nor landing bytes, and dev() / host() are null
// for it.  Prints "ok" and exits 0, or says what differs.
#include "../motion_primitive_library_amd/csrc/mplx_stage.h"

#include <cstdio>
#include <cstdlib>

using namespace mplx_detail;

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
  static char arena[1 << 16];
  double host_a[8] = {0}, host_b[100] = {0};
  const size_t sizes[] = {1, 255, 256, 257, 0, 4000, 8};
  StageLayout l;
  size_t want[7];
  for (int i = 0; i < 7; i++) want[i] = l.add(sizes[i]);
  StageRows s;
  const auto r0 = s.in(host_a, 1), r1 = s.in_rows(host_b, 80, 51, 5), r2 = s.out(host_a, 256), r3 = s.landed(257),
             r4 = s.out(nullptr, 4000), r5 = s.landed_or_scratch(nullptr, 4000), r6 = s.inout(host_a, 8);
  const auto r7 = s.landed_from(arena + 100, 12), r8 = s.landed(nullptr, 64), r9 = s.scratch(0), r10 = s.out_or_scratch(nullptr, 3);
  CHECK(s.total() == l.total + align256(3) && !s.overflow && s.n == 11);
  s.l.base = arena;  // (what stage_commit does after ensure())
  s.landing = (char *)::operator new(s.land_total);
  const StageRows::Row rows[] = {r0, r1, r2, r3, r4, r5, r6};
  for (int i = 0; i < 7; i++) {
    if (sizes[i]) CHECK(s.dev<char>(rows[i]) == arena + want[i]);
    else CHECK(s.dev<char>(rows[i]) == nullptr);
  }
  CHECK(s.rec[r1.i].bytes == 255 && s.rec[r1.i].pitch == 80 && s.rec[r1.i].rows == 5 && s.rec[r1.i].width == 51);
  CHECK(s.host<char>(r3) == s.landing && s.host<char>(r7) == s.landing + 272 && s.land_total == 272 + 16);
  CHECK(!s.host<char>(r5) && !s.host<char>(r8) && !s.dev<char>(r7) && !s.dev<char>(r8) && !s.dev<char>(r9) && s.dev<char>(r10));
  CHECK(s.rec[r6.i].src == host_a && s.rec[r6.i].dst == host_a && !s.rec[r4.i].dst && !s.rec[r10.i].dst && s.rec[r7.i].from == arena + 100);
  StageRows full;
  for (int i = 0; i < StageRows::kMaxRows; i++) full.scratch(8);
  CHECK(!full.overflow);
  full.scratch(8);
  CHECK(full.overflow && full.n == StageRows::kMaxRows);
  std::printf("ok\n");
  return 0;
}
