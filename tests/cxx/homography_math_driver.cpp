// Runs the arithmetic of the batched homography stage (sim3opt_amd/csrc/homography_math.hpp: sampler, four-point
// homography, error, refinement round, decomposition, choice) on the host, so that tests/test_homography_ref.py can hold
// the very statements the kernel runs against tests/homography_ref.py without a GPU.  Reads stdin.
//   homography_math_driver hyp        "f cx cy seed H n", then n lines "u0 v0 u1 v1"
//       prints per hypothesis         "i0 .. i3 valid H(9) cost"  (cost: MLESAC at max_pixel_error 5, points ascending)
//   homography_math_driver solve      "f cx cy seed H n max_pixel_error rounds", then the points
//       prints                        "best cost m", the mask, "Hm(9)", per round "sigma2 H(9)", then the choice (below)
//   homography_math_driver decompose  "f cx cy 0 0 n max_pixel_error 0", then the points, then "H(9)", then the mask
//       prints the choice:            "status", 8 lines "R(9) t(3) n(3) d", "c1(8)", "kept(4)", "c2(4)",
//                                     "choice ambiguous sampson(2)", "pose(7)"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sim3opt_amd/csrc/homography_math.hpp"

namespace HM = sim3opt_homography;

static void print_row(const double* v, int n) {
  for (int i = 0; i < n; ++i) std::printf("%s%.17g", i ? " " : "", v[i]);
  std::printf("\n");
}

static void print_ints(const int* v, int n) {
  for (int i = 0; i < n; ++i) std::printf("%s%d", i ? " " : "", v[i]);
  std::printf("\n");
}

// DecomposeHomography and ChooseBestDecomposition as homography_batch.hip's decompose_choose states them
static void choose(const std::vector<double>& p, int n, const std::vector<int>& in, const double H[9], double max2) {
  HM::HomSvd S;
  if (!HM::hom_svd(H, S)) {
    std::printf("4\n");
    return;
  }
  std::printf("0\n");
  int c1[8] = {}, kept[4], k1[4], c2[4] = {}, kept2[2], k2[2];
  const int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  double R[9], t[3], nn[3], d;
  for (int k = 0; k < 8; ++k) {
    HM::hom_decomposition(S, k, R, t, nn, d);
    double row[16];
    std::memcpy(row, R, sizeof R);
    std::memcpy(row + 9, t, sizeof t);
    std::memcpy(row + 12, nn, sizeof nn);
    row[15] = d;
    print_row(row, 16);
    for (int i = 0; i < n; ++i)
      if (in[i]) c1[k] += HM::hom_visible_h(H, p[4 * (size_t)i], p[4 * (size_t)i + 1], HM::hom_decomposition_d(S, k));
  }
  HM::hom_keep<8, 4>(ids, c1, kept, k1);
  for (int q = 0; q < 4; ++q) {
    HM::hom_decomposition(S, kept[q], R, t, nn, d);
    for (int i = 0; i < n; ++i)
      if (in[i]) c2[q] += HM::hom_visible_n(nn, p[4 * (size_t)i], p[4 * (size_t)i + 1], d);
  }
  HM::hom_keep<4, 2>(kept, c2, kept2, k2);
  int choice = kept2[0];
  const bool ambiguous = HM::hom_ambiguous(k2[0], k2[1]);
  double sums[2] = {0.0, 0.0};
  if (ambiguous) {
    for (int c = 0; c < 2; ++c) {
      double E[9];
      HM::hom_decomposition(S, kept2[c], R, t, nn, d);
      HM::hom_essential(R, t, E);
      for (int i = 0; i < n; ++i)
        sums[c] += HM::hom_sampson(E, p[4 * (size_t)i], p[4 * (size_t)i + 1], p[4 * (size_t)i + 2], p[4 * (size_t)i + 3],
                                   max2 * 4);
    }
    choice = sums[0] <= sums[1] ? kept2[0] : kept2[1];
  }
  print_ints(c1, 8);
  print_ints(kept, 4);
  print_ints(c2, 4);
  std::printf("%d %d %.17g %.17g\n", choice, ambiguous ? 1 : 0, sums[0], sums[1]);
  double pose[7];
  HM::hom_decomposition(S, choice, R, t, nn, d);
  HM::hom_R_to_quat(R, pose);
  for (int i = 0; i < 3; ++i) pose[4 + i] = t[i];
  print_row(pose, 7);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  double f, cx, cy, maxpx = 5.0;
  uint64_t seed;
  int H, n, rounds = 0;
  if (std::scanf("%lf %lf %lf %" SCNu64 " %d %d", &f, &cx, &cy, &seed, &H, &n) != 6 || !(f > 0) || n < 4) return 2;
  const bool hyp = !std::strcmp(argv[1], "hyp"), solve = !std::strcmp(argv[1], "solve");
  if (!hyp && !solve && std::strcmp(argv[1], "decompose")) return 2;
  if (!hyp && std::scanf("%lf %d", &maxpx, &rounds) != 2) return 2;
  if (rounds < 0 || rounds > HM::MAX_ROUNDS || (!(!hyp && !solve) && H < 1)) return 2;
  std::vector<double> p(4 * (size_t)n);
  for (double& x : p)
    if (std::scanf("%lf", &x) != 1) return 2;
  for (size_t i = 0; i < p.size(); ++i) p[i] = (p[i] - ((i & 1) ? cy : cx)) / f;
  const double max2 = maxpx * maxpx;
  auto err2 = [&](const double* M, int i) {
    return HM::hom_sqerr(M, p[4 * (size_t)i], p[4 * (size_t)i + 1], p[4 * (size_t)i + 2], p[4 * (size_t)i + 3], f);
  };

  std::vector<int> in(n, 0);
  double Hb[9];
  if (!hyp && !solve) {  // decompose
    for (double& x : Hb)
      if (std::scanf("%lf", &x) != 1) return 2;
    for (int& x : in)
      if (std::scanf("%d", &x) != 1) return 2;
    choose(p, n, in, Hb, max2);
    return 0;
  }

  int best = -1;
  double best_cost = 0.0;
  for (int h = 0; h < H; ++h) {
    int idx[4];
    sim3opt_ransac::ransac_sample<4>(seed, (uint32_t)h, n, idx);
    double q[4][4], Hh[9];
    for (int k = 0; k < 4; ++k)
      for (int c = 0; c < 4; ++c) q[k][c] = p[4 * (size_t)idx[k] + c];
    const bool valid = HM::hom_four_point(q, Hh);
    double cost = 0.0;
    if (valid)
      for (int i = 0; i < n; ++i) cost += HM::hom_mlesac(err2(Hh, i), max2);
    if (valid && (best < 0 || cost < best_cost)) {
      best = h; best_cost = cost;
      std::memcpy(Hb, Hh, sizeof Hb);
    }
    if (hyp) {
      std::printf("%d %d %d %d %d ", idx[0], idx[1], idx[2], idx[3], valid ? 1 : 0);
      for (int i = 0; i < 9; ++i) std::printf("%.17g ", Hh[i]);
      std::printf("%.17g\n", cost);
    }
  }
  if (hyp) return 0;
  if (best < 0) return 3;
  int m = 0;
  for (int i = 0; i < n; ++i) m += (in[i] = err2(Hb, i) < max2 ? 1 : 0);
  std::printf("%d %.17g %d\n", best, best_cost, m);
  print_ints(in.data(), n);
  print_row(Hb, 9);
  if (m < 4) return 3;
  std::vector<double> e(n);
  for (int r = 0; r < rounds; ++r) {
    for (int i = 0; i < n; ++i) e[i] = in[i] ? err2(Hb, i) : -1.0;
    double median = 0.0;
    for (int i = 0; i < n; ++i) {  // the element of rank m / 2, ties in the order of the points
      if (!(e[i] >= 0.0)) continue;
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += e[j] >= 0.0 && (e[j] < e[i] || (e[j] == e[i] && j < i));
      if (rank == m / 2) median = e[i];
    }
    const double sigma2 = HM::hom_sigma2(median, m);
    double acc[HM::HOM_ACC] = {}, upd[9];
    for (int i = 0; i < n; ++i) {
      if (!in[i]) continue;
      double ex, ey, p0, p1, den;
      const double e2 = HM::hom_error(Hb, p[4 * (size_t)i], p[4 * (size_t)i + 1], p[4 * (size_t)i + 2],
                                      p[4 * (size_t)i + 3], f, ex, ey, p0, p1, den);
      HM::hom_accumulate(acc, HM::hom_weight(e2, sigma2), p[4 * (size_t)i], p[4 * (size_t)i + 1], f, ex, ey, p0, p1, den);
    }
    HM::hom_solve_update(acc, 1.0, upd);
    for (int i = 0; i < 9; ++i) Hb[i] += upd[i];
    std::printf("%.17g ", sigma2);
    print_row(Hb, 9);
  }
  choose(p, n, in, Hb, max2);
  return 0;
}
