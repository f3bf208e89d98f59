// Runs the per-hypothesis arithmetic of the batched PnP RANSAC (sim3opt_amd/csrc/pnp_math.hpp: sampler, quartic, P3P)
// on the host, so that tests/test_pnp_ref.py can hold the very statements the kernel runs against tests/pnp_ref.py
// without a GPU.
//   pnp_math_driver FILE     FILE: "f cx cy seed H n", then n lines "X Y Z u v"
//   prints per hypothesis:   "i0 i1 i2 i3 valid n_solutions R(9) t(3)"
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../sim3opt_amd/csrc/pnp_math.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* fp = std::fopen(argv[1], "r");
  if (!fp) return 2;
  double f, cx, cy;
  uint64_t seed;
  int H, n;
  if (std::fscanf(fp, "%lf %lf %lf %" SCNu64 " %d %d", &f, &cx, &cy, &seed, &H, &n) != 6 || n < 4 || H < 1) return 2;
  std::vector<double> p(5 * (size_t)n);
  for (size_t i = 0; i < p.size(); ++i)
    if (std::fscanf(fp, "%lf", &p[i]) != 1) return 2;
  std::fclose(fp);
  for (int h = 0; h < H; ++h) {
    int idx[4], nsol = 0;
    sim3opt_ransac::ransac_sample<4>(seed, (uint32_t)h, n, idx);
    double X[4][3], uv[4][2], R[9], t[3];
    for (int k = 0; k < 4; ++k) {
      for (int c = 0; c < 3; ++c) X[k][c] = p[5 * (size_t)idx[k] + c];
      uv[k][0] = p[5 * (size_t)idx[k] + 3];
      uv[k][1] = p[5 * (size_t)idx[k] + 4];
    }
    const bool valid = sim3opt_pnp::p3p_hypothesis(X, uv, f, cx, cy, R, t, nsol);
    std::printf("%d %d %d %d %d %d", idx[0], idx[1], idx[2], idx[3], valid ? 1 : 0, nsol);
    for (int i = 0; i < 9; ++i) std::printf(" %.17g", R[i]);
    for (int i = 0; i < 3; ++i) std::printf(" %.17g", t[i]);
    std::printf("\n");
  }
  return 0;
}
