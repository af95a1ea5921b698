// heur_math_harness.cpp -- csrc/mplx_heur_math.h as a host program: the sweeps of tests/test_heur_model.py through the
// very expressions the device compiles, built with -fsanitize=address,undefined (tests/test_heur_model.py).
//
// argv: in out.  in (doubles): D control goal_control mode w v_max K, the goal's 4D+1 rows, then K states of 4D+1 rows
// each.  mode 1: heur::reference (a JRK branch gives NaN), 2: heur::robust.  out: K doubles.
#include "../../motion_primitive_library_amd/csrc/mplx_heur_math.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace mh = mplx::heur;

template <int D>
static void run(const std::vector<double> &in, std::vector<double> &out) {
  const int control = (int)in[1], goal_control = (int)in[2], mode = (int)in[3], F = 4 * D + 1;
  const double w = in[4], v_max = in[5];
  const size_t K = (size_t)in[6];
  const double *goal = in.data() + 7, *s = goal + F;
  if (in.size() < 7 + (K + 1) * (size_t)F) std::exit(5);
  for (size_t k = 0; k < K; k++, s += F) {
    bool unsupported = false;
    out.push_back(mode == 1 ? mh::reference<D>(s, goal, control, goal_control ? goal_control : control, w, v_max, &unsupported)
                            : mh::robust<D>(s, goal, control, goal_control, w, v_max));
  }
}

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  std::vector<double> in, out;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  in.resize((size_t)std::ftell(f) / sizeof(double));
  std::fseek(f, 0, SEEK_SET);
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  if (in.size() < 7) return 5;
  if ((int)in[0] == 2) run<2>(in, out);
  else run<3>(in, out);
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
  std::fclose(f);
  std::printf("harness: ok\n");
  return 0;
}
