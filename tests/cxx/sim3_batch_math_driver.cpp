// Runs the arithmetic of the batched Sim(3) stage (sim3opt_amd/csrc/sim3_batch_math.hpp: sampler, Horn's closed form,
// scoring, LM refinement, information) on the host in the kernel's order of summation, so that
// tests/test_sim3_batch_ref.py can hold the very statements the kernel runs against tests/sim3_batch_ref.py without a
// GPU, and tests/test_gpu_sim3_batch.py can compare the device with them bit for bit.  Reads stdin:
//   "f cx cy seed H n max_pixel_error huber_delta pixel_noise min_triangle_sin2 tau min_points min_inliers
//    refine_iters max_trials", then n lines "u0 v0 depth0 u1 v1 depth1"; refine and info: then "C(8)" and the mask.
//   sim3_batch_math_driver hyp     per hypothesis "i0 i1 i2 valid C(8) count cost"
//   sim3_batch_math_driver solve   "status best n_hyp cost_hyp", the hypothesis's mask, "C(8)", "iterations chi0 chi1",
//                                  "trials(refine_iters)", the final mask, "count rms", "Omega(49)"
//                                  (status 1 or 2: the first line only)
//   sim3_batch_math_driver refine  "C(8)", "iterations chi0 chi1", "trials(refine_iters)"
//   sim3_batch_math_driver info    "pd", "Omega(49)", n lines "w1 w0"
#include <cfloat>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sim3opt_amd/csrc/lm_damping.hpp"
#include "../../sim3opt_amd/csrc/sim3_batch_math.hpp"

namespace SB = sim3opt_sim3b;

static const int WG = 256, LANES = 64;

struct Problem {
  double f, cx, cy, max2, huber, pixel_noise, min_sin2, tau;
  uint64_t seed;
  int H, n, min_points, min_inliers, refine_iters, max_trials;
  std::vector<double> p;  // n x 6, as s3b_match leaves them
};

static void print_row(const double* v, int n) {
  for (int i = 0; i < n; ++i) std::printf("%s%.17g", i ? " " : "", v[i]);
  std::printf("\n");
}

static void print_ints(const int* v, int n) {
  for (int i = 0; i < n; ++i) std::printf("%s%d", i ? " " : "", v[i]);
  std::printf("\n");
}

// ba_math.hpp's wg_sum of per-thread values v[t][q]: a butterfly over each wavefront, then the wavefronts in order
template <int N>
static void wg_sum(std::vector<double>& v, double out[N]) {
  for (int q = 0; q < N; ++q) {
    double w[4];
    for (int wave = 0; wave < 4; ++wave) {
      double x[LANES], y[LANES];
      for (int l = 0; l < LANES; ++l) x[l] = v[(size_t)(wave * LANES + l) * N + q];
      for (int off = 32; off > 0; off >>= 1) {
        for (int l = 0; l < LANES; ++l) y[l] = x[l] + x[l ^ off];
        std::memcpy(x, y, sizeof x);
      }
      w[wave] = x[0];
    }
    out[q] = ((w[0] + w[1]) + w[2]) + w[3];
  }
}

// ransac_frame.hpp's score_model: lane l takes the matches l, l + 64, ... ascending, then a butterfly
static void score(const Problem& P, const double C[8], int& count, double& cost) {
  SB::S3bPrep prep;
  SB::s3b_prepare(C, prep);
  double s[LANES], y[LANES];
  int c = 0;
  for (int l = 0; l < LANES; ++l) {
    s[l] = 0.0;
    for (int i = l; i < P.n; i += LANES) {
      double e2;
      if (SB::s3b_inlier(prep, &P.p[6 * (size_t)i], P.f, P.max2, e2)) { ++c; s[l] += e2; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    for (int l = 0; l < LANES; ++l) y[l] = s[l] + s[l ^ off];
    std::memcpy(s, y, sizeof s);
  }
  count = c;
  cost = s[0];
}

static void mark(const Problem& P, const double C[8], std::vector<int>& in, int& count, double& cost) {
  SB::S3bPrep prep;
  SB::s3b_prepare(C, prep);
  std::vector<double> acc((size_t)WG * 2, 0.0);
  for (int t = 0; t < WG; ++t)
    for (int i = t; i < P.n; i += WG) {
      double e2;
      in[i] = SB::s3b_inlier(prep, &P.p[6 * (size_t)i], P.f, P.max2, e2) ? 1 : 0;
      if (in[i]) { acc[2 * (size_t)t] += 1.0; acc[2 * (size_t)t + 1] += e2; }
    }
  double out[2];
  wg_sum<2>(acc, out);
  count = (int)out[0];
  cost = out[1];
}

static void linearize(const Problem& P, const std::vector<int>& in, const double C[8], double out[SB::S3B_ACC],
                      std::vector<double>* weights) {
  SB::S3bPrep prep;
  SB::s3b_prepare(C, prep);
  std::vector<double> acc((size_t)WG * SB::S3B_ACC, 0.0);
  for (int t = 0; t < WG; ++t)
    for (int i = t; i < P.n; i += WG) {
      double w[2] = {0.0, 0.0};
      if (in[i]) SB::s3b_accumulate(prep, &P.p[6 * (size_t)i], P.f, P.huber, &acc[(size_t)t * SB::S3B_ACC], w);
      if (weights) { (*weights)[2 * (size_t)i] = w[0]; (*weights)[2 * (size_t)i + 1] = w[1]; }
    }
  wg_sum<SB::S3B_ACC>(acc, out);
}

static double masked_chi2(const Problem& P, const std::vector<int>& in, const double C[8]) {
  SB::S3bPrep prep;
  SB::s3b_prepare(C, prep);
  std::vector<double> acc((size_t)WG, 0.0);
  for (int t = 0; t < WG; ++t)
    for (int i = t; i < P.n; i += WG)
      if (in[i]) acc[t] += SB::s3b_chi2(prep, &P.p[6 * (size_t)i], P.f, P.huber);
  double out[1];
  wg_sum<1>(acc, out);
  return out[0];
}

// sim3_batch.hip's s3b_refit, statement for statement
static void refit(const Problem& P, const std::vector<int>& in, double C[8], std::vector<int>& trials, int& iters,
                  double& chi_before, double& chi_after) {
  const double GAIN_TOL = 1e-9;
  sim3opt::LmDamping damp;
  bool go = true;
  iters = 0;
  double currentChi = 0.0;
  for (int it = 0; it < P.refine_iters && go; ++it) {
    double acc[SB::S3B_ACC];
    linearize(P, in, C, acc, nullptr);
    currentChi = acc[35];
    if (it == 0) {
      chi_before = currentChi;
      double maxdiag = 0.0;
      for (int r = 0; r < 7; ++r) maxdiag = std::fmax(maxdiag, acc[SB::tri7(r, r)]);
      damp.start(0.0, P.tau, maxdiag);
    }
    double rho = 0.0;
    int qmax = 0;
    bool converged = false;
    do {
      const double lambda = damp.lambda;
      double Su[28], gv[7], dx[7], nC[8];
      for (int k = 0; k < 28; ++k) Su[k] = acc[k];
      for (int r = 0; r < 7; ++r) { Su[SB::tri7(r, r)] += lambda; gv[r] = acc[28 + r]; }
      const bool fail = !SB::s3b_chol7_solve(Su, gv, dx);
      double tempChi = DBL_MAX, scale = 0.0;
      std::memcpy(nC, C, sizeof nC);
      if (!fail) {
        for (int r = 0; r < 7; ++r) scale += dx[r] * (lambda * dx[r] + gv[r]);
        if (scale <= GAIN_TOL * currentChi) { converged = true; break; }
        SB::s3b_oplus(dx, nC);
        tempChi = masked_chi2(P, in, nC);
      }
      if (damp.update(currentChi, tempChi, scale, 1.0 / 3.0, 2.0 / 3.0, rho)) {
        currentChi = tempChi;
        std::memcpy(C, nC, sizeof nC);
      }
      ++qmax;
    } while (rho < 0 && qmax < P.max_trials);
    if (converged && qmax == 0) break;
    trials[it] = qmax;
    ++iters;
    if (converged || damp.terminate(qmax, P.max_trials, rho)) go = false;
  }
  if (iters == 0) chi_before = currentChi = masked_chi2(P, in, C);
  chi_after = currentChi;
}

static bool information(const Problem& P, const std::vector<int>& in, const double C[8], double om[49],
                        std::vector<double>* weights) {
  double acc[SB::S3B_ACC], Su[28], z[7] = {}, x[7];
  linearize(P, in, C, acc, weights);
  SB::s3b_information(acc, P.pixel_noise, om);
  for (int r = 0; r < 7; ++r)
    for (int c = r; c < 7; ++c) Su[SB::tri7(r, c)] = om[7 * c + r];
  return SB::s3b_chol7_solve(Su, z, x);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Problem P;
  double maxpx;
  if (std::scanf("%lf %lf %lf %" SCNu64 " %d %d %lf %lf %lf %lf %lf %d %d %d %d", &P.f, &P.cx, &P.cy, &P.seed, &P.H,
                 &P.n, &maxpx, &P.huber, &P.pixel_noise, &P.min_sin2, &P.tau, &P.min_points, &P.min_inliers,
                 &P.refine_iters, &P.max_trials) != 15)
    return 2;
  if (!(P.f > 0) || P.n < 1 || P.H < 0 || P.H > 4096 || P.refine_iters < 0 || P.refine_iters > 1000 || P.max_trials < 1)
    return 2;
  P.max2 = maxpx * maxpx;
  P.p.resize(6 * (size_t)P.n);
  for (int i = 0; i < P.n; ++i) {
    double m[6];
    for (double& x : m)
      if (std::scanf("%lf", &x) != 1) return 2;
    SB::s3b_match(m[0], m[1], m[2], m[3], m[4], m[5], P.f, P.cx, P.cy, &P.p[6 * (size_t)i]);
  }
  const bool hyp = !std::strcmp(argv[1], "hyp"), solve = !std::strcmp(argv[1], "solve");
  const bool refine = !std::strcmp(argv[1], "refine"), info = !std::strcmp(argv[1], "info");
  if (!hyp && !solve && !refine && !info) return 2;
  std::vector<int> in(P.n, 0), trials(P.refine_iters > 0 ? P.refine_iters : 1, 0);
  double C[8], om[49];

  if (refine || info) {
    for (double& x : C)
      if (std::scanf("%lf", &x) != 1) return 2;
    for (int& x : in)
      if (std::scanf("%d", &x) != 1) return 2;
    if (refine) {
      int iters;
      double chi0 = 0.0, chi1 = 0.0;
      refit(P, in, C, trials, iters, chi0, chi1);
      print_row(C, 8);
      std::printf("%d %.17g %.17g\n", iters, chi0, chi1);
      print_ints(trials.data(), P.refine_iters);
    } else {
      std::vector<double> w(2 * (size_t)P.n);
      std::printf("%d\n", information(P, in, C, om, &w) ? 1 : 0);
      print_row(om, 49);
      for (int i = 0; i < P.n; ++i) print_row(&w[2 * (size_t)i], 2);
    }
    return 0;
  }

  if (P.n < P.min_points || P.n < 3) {
    if (solve) std::printf("1 -1 0 0\n");
    return 0;
  }
  int best = -1, best_count = -1;
  double best_cost = 0.0;
  for (int h = 0; h < P.H; ++h) {
    int idx[3], count = 0;
    sim3opt_ransac::ransac_sample<3>(P.seed, (uint32_t)h, P.n, idx);
    double s[3][6], m[8], cost = 0.0;
    for (int j = 0; j < 3; ++j) std::memcpy(s[j], &P.p[6 * (size_t)idx[j]], sizeof s[j]);
    const bool valid = SB::s3b_horn(s, P.min_sin2, m);
    if (valid) {
      score(P, m, count, cost);
      if (count > best_count || (count == best_count && cost < best_cost)) {  // (ascending: of equals the first stays)
        best = h; best_count = count; best_cost = cost;
        std::memcpy(C, m, sizeof C);
      }
    }
    if (hyp) {
      std::printf("%d %d %d %d ", idx[0], idx[1], idx[2], valid ? 1 : 0);
      for (int i = 0; i < 8; ++i) std::printf("%.17g ", m[i]);
      std::printf("%d %.17g\n", count, cost);
    }
  }
  if (hyp) return 0;
  if (best < 0) {
    std::printf("2 -1 0 0\n");
    return 0;
  }
  int count, iters = 0;
  double cost, chi0 = 0.0, chi1 = 0.0, C0[8];
  std::memcpy(C0, C, sizeof C0);
  mark(P, C, in, count, cost);
  std::vector<int> in_hyp = in;
  if (P.refine_iters > 0) {
    refit(P, in, C, trials, iters, chi0, chi1);
    mark(P, C, in, count, cost);
  }
  const bool pd = information(P, in, C, om, nullptr);
  std::printf("%d %d %d %.17g\n", count < P.min_inliers ? 3 : (pd ? 0 : 4), best, best_count, best_cost);
  print_ints(in_hyp.data(), P.n);
  print_row(C, 8);
  std::printf("%d %.17g %.17g\n", iters, chi0, chi1);
  print_ints(trials.data(), P.refine_iters);
  print_ints(in.data(), P.n);
  std::printf("%d %.17g\n", count, count > 0 ? std::sqrt(cost / (2.0 * (double)count)) : 0.0);
  print_row(om, 49);
  return 0;
}
