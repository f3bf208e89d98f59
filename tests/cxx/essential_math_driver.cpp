// Runs the per-hypothesis arithmetic of the batched essential-matrix RANSAC (sim3opt_amd/csrc/essential_math.hpp:
// sampler, five-point method, Sampson error, pose candidates, depths) on the host, so that tests/test_essential_ref.py
// can hold the very statements the kernel runs against tests/essential_ref.py without a GPU.  Reads stdin.
//   essential_math_driver hyp    "f cx cy seed H n", then n lines "u0 v0 u1 v1"
//       prints per hypothesis    "i0 .. i5 valid n_solutions E(9)"
//   essential_math_driver pose   "f cx cy distance_threshold n m", then n lines "u0 v0 u1 v1", then m lines "E(9)"
//       prints per E             "ok candidates(4 x 7) votes(4)", every point voting
//   essential_math_driver score  "f cx cy threshold n m", then the points and m lines "E(9)"
//       prints per E             "count cost" (points in ascending order) and then the n errors
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sim3opt_amd/csrc/essential_math.hpp"

namespace E5 = sim3opt_essential;

static bool read_doubles(std::vector<double>& v) {
  for (double& x : v)
    if (std::scanf("%lf", &x) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  double f, cx, cy;
  if (std::scanf("%lf %lf %lf", &f, &cx, &cy) != 3 || !(f > 0)) return 2;
  if (!std::strcmp(argv[1], "hyp")) {
    uint64_t seed;
    int H, n;
    if (std::scanf("%" SCNu64 " %d %d", &seed, &H, &n) != 3 || n < 6 || H < 1) return 2;
    std::vector<double> p(4 * (size_t)n);
    if (!read_doubles(p)) return 2;
    std::vector<double> ws(E5::WS_DOUBLES);
    for (int h = 0; h < H; ++h) {
      int idx[6], nsol = 0;
      sim3opt_ransac::ransac_sample<6>(seed, (uint32_t)h, n, idx);
      double q[6][4], E[9];
      for (int k = 0; k < 6; ++k)
        for (int c = 0; c < 4; ++c) q[k][c] = (p[4 * (size_t)idx[k] + c] - ((c & 1) ? cy : cx)) / f;
      const bool valid = E5::ess_hypothesis(E5::HostGroup{}, q, ws.data(), E, nsol);
      for (int k = 0; k < 6; ++k) std::printf("%d ", idx[k]);
      std::printf("%d %d", valid ? 1 : 0, nsol);
      for (int i = 0; i < 9; ++i) std::printf(" %.17g", E[i]);
      std::printf("\n");
    }
    return 0;
  }
  const bool pose = !std::strcmp(argv[1], "pose");
  if (!pose && std::strcmp(argv[1], "score")) return 2;
  double par;
  int n, m;
  if (std::scanf("%lf %d %d", &par, &n, &m) != 3 || n < 1 || m < 1) return 2;
  std::vector<double> p(4 * (size_t)n), Es(9 * (size_t)m);
  if (!read_doubles(p) || !read_doubles(Es)) return 2;
  for (size_t i = 0; i < p.size(); ++i) p[i] = (p[i] - ((i & 1) ? cy : cx)) / f;
  for (int e = 0; e < m; ++e) {
    const double* E = Es.data() + 9 * (size_t)e;
    if (pose) {
      double R[2][9], t[3];
      const bool ok = E5::ess_candidates(E, R, t);
      const double tm[3] = {-t[0], -t[1], -t[2]};
      std::printf("%d", ok ? 1 : 0);
      for (int c = 0; c < 4; ++c) {
        double q[4];
        E5::ess_R_to_quat(R[c & 1], q);
        for (int i = 0; i < 4; ++i) std::printf(" %.17g", q[i]);
        for (int i = 0; i < 3; ++i) std::printf(" %.17g", c < 2 ? t[i] : tm[i]);
      }
      for (int c = 0; c < 4; ++c) {
        int votes = 0;
        for (int i = 0; i < n; ++i)
          votes += ok && E5::ess_votes(R[c & 1], c < 2 ? t : tm, p[4 * (size_t)i], p[4 * (size_t)i + 1],
                                       p[4 * (size_t)i + 2], p[4 * (size_t)i + 3], par);
        std::printf(" %d", votes);
      }
      std::printf("\n");
    } else {
      const double thr = par / f, thr2 = thr * thr;
      int count = 0;
      double cost = 0.0;
      std::vector<double> e2(n);
      for (int i = 0; i < n; ++i) {
        e2[i] = E5::ess_sampson(E, p[4 * (size_t)i], p[4 * (size_t)i + 1], p[4 * (size_t)i + 2], p[4 * (size_t)i + 3]);
        if (e2[i] <= thr2) { ++count; cost += e2[i]; }
      }
      std::printf("%d %.17g", count, cost);
      for (int i = 0; i < n; ++i) std::printf(" %.17g", e2[i]);
      std::printf("\n");
    }
  }
  return 0;
}
