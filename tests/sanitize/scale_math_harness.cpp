// scale_math_harness.cpp -- csrc/mplx_scale_math.h as a host program: the sweep of tests/test_scale_model.py through the
// very expressions the device compiles, built with -fsanitize=address,undefined (tests/test_scale_model.py).
//
// argv: in out.  in (doubles): n Q, then per call: T ri rf mode, Q real times as fractions of the scaled total (the
// time is fraction * total, or i * (total / (Q - 1)) where the fraction is negative: -(i + 1)).
// out (doubles), per call: status, the 8 fields of the segment, Ts(T) = total, then per time: the time, the robust or
// reference getTau as it came, found, the clamped tau, lambda, lambda_dot.
#include "../../motion_primitive_library_amd/csrc/mplx_scale_math.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace ms = mplx::scale;

struct ArrayLoader {
  const double *seg;
  double operator()(int s, int f) const { return seg[s * 8 + f]; }
};

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  std::vector<double> in;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  in.resize((size_t)std::ftell(f) / sizeof(double));
  std::fseek(f, 0, SEEK_SET);
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  const int n = (int)in[0], Q = (int)in[1];
  std::vector<double> out;
  const double *p = in.data() + 2;
  for (int k = 0; k < n; k++, p += 4 + Q) {
    const double T = p[0], ri = p[1], rf = p[2];
    const bool robust = p[3] != 0;
    double seg[8];
    const int status = ms::build_seg(1.0 / ri, 0.0, 0.0, 1.0 / rf, 0.0, T, robust, seg);
    const ArrayLoader ld{seg};
    const double total = ms::lambda_getT(ld, 1, T);
    out.push_back((double)status);
    for (int i = 0; i < 8; i++) out.push_back(seg[i]);
    out.push_back(total);
    for (int q = 0; q < Q; q++) {
      const double fr = p[4 + q];
      const double t = fr < 0 ? (double)(int)(-fr - 1) * (total / (double)(Q - 1)) : fr * total;
      double raw = 0, lam = 0, dot = 0;
      bool found = false;
      const double tau = status ? 0.0 : ms::sample_tau(ld, 1, robust, t, total, T, &raw, &found, &lam, &dot);
      out.push_back(t);
      out.push_back(raw);
      out.push_back(found ? 1.0 : 0.0);
      out.push_back(tau);
      out.push_back(lam);
      out.push_back(dot);
    }
  }
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
  std::fclose(f);
  std::printf("harness: ok\n");
  return 0;
}
