// Conformance program of include/sim3opt_two_view.hpp (TwoViewRefiner over sim3opt_ba_batch_*), the batched
// replacement of BAOptimize (kittiDetector.h:845-954).
//   two_view_conformance host         argument checks of the helper and of the C-ABI; needs no GPU
//   two_view_conformance run FILE     refines the candidates of FILE in one optimize() and compares with the
//                                     expected values FILE carries (tests/test_gpu_two_view_batch.py writes it from
//                                     the oracle's runs); exit 3 with the library's message when there is no GPU
// FILE: "n f cx cy", then per candidate "npts iters", Rf2s (9, row-major), tfins (3), npts rows "X Y Z u0 v0 u1 v1",
// then the expectation: trials (iters), chi2_after (iters), quaternion x y z w, translation, npts rows of points,
// the number of outlier edges.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "sim3opt_two_view.hpp"

namespace {
int g_checks = 0, g_failed = 0;
void check(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    ++g_failed;
    std::printf("FAILED: %s\n", what);
  }
}
#define CHECK(x) check((x), #x)

struct P3 { float x, y, z; };    // cv::Point3f's members
struct P2 { float x, y; };       // cv::Point2f's
struct P3d { double x, y, z; };
struct P2d { double x, y; };

const double K[9] = {718.856, 0, 607.1928, 0, 718.856, 185.2157, 0, 0, 1};
const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

int host_part() {
  using sim3opt_shim::TwoViewRefiner;
  // ---- the helper ----
  {
    TwoViewRefiner r;
    CHECK(r.size() == 0);
    CHECK(r.options().max_iters == 10 && r.options().max_trials == 5 && r.options().huber_delta == 3.0 &&
          r.options().user_lambda_init == 50.0 && r.options().outlier_chi2 == 5.995 && r.options().pixel_noise == 1.0);
    std::vector<P3> xyz = {{1.f, 0.5f, 10.f}, {-2.f, 0.25f, 20.f}};
    std::vector<P2> a = {{679.f, 221.f}, {535.f, 194.f}}, b = {{650.f, 221.f}, {520.f, 194.f}}, shorter = {{1.f, 2.f}};
    const double t[3] = {0.1, 0.0, -1.0};
    CHECK(r.add(xyz, a, shorter, K, I3, t) == -1 && r.size() == 0 && !r.last_error().empty());
    CHECK(r.add(std::vector<P3>(), std::vector<P2>(), std::vector<P2>(), K, I3, t) == -1 && r.size() == 0);
    CHECK(r.add(xyz, a, b, nullptr, I3, t) == -1 && r.size() == 0);
    CHECK(r.add(xyz, a, b, K, I3, t) == 0 && r.size() == 1 && r.n_points(0) == 2);
    const double K2[9] = {700, 0, 600, 0, 700, 180, 0, 0, 1};
    CHECK(r.add(xyz, a, b, K2, I3, t) == -1 && r.size() == 1);  // one K per refiner
    CHECK(r.add(xyz, a, b, K, I3, t) == 1 && r.size() == 2);
    CHECK(r.quaternion(0)[3] == 1.0 && r.quaternion(0)[0] == 0.0 && r.translation(1)[2] == -1.0);
    CHECK(r.points(1)[2] == 10.0 && r.points(1)[5] == 20.0);
    double R[9];
    r.rotation(0, R);
    bool same = true;
    for (int i = 0; i < 9; ++i) same = same && R[i] == I3[i];
    CHECK(same);
    // a 90 degree yaw goes through the quaternion and back
    const double Ry[9] = {0, 0, 1, 0, 1, 0, -1, 0, 0};
    double q[4];
    TwoViewRefiner::rotation_to_quaternion(Ry, q);
    CHECK(std::fabs(q[1] - std::sqrt(0.5)) < 1e-15 && std::fabs(q[3] - std::sqrt(0.5)) < 1e-15 && q[0] == 0 && q[2] == 0);
    r.options().max_iters = 0;
    CHECK(r.optimize() == SIM3OPT_ERR_ARG && !r.last_error().empty());
    r.clear();
    CHECK(r.size() == 0);
    r.options().max_iters = 10;
    CHECK(r.optimize() == SIM3OPT_ERR_ARG);  // nothing to refine
  }
  // ---- the C-ABI: every refusal leaves the handle as it was ----
  {
    sim3opt_ba_batch* h = sim3opt_ba_batch_create();
    CHECK(h != nullptr);
    const int32_t ptr[3] = {0, 2, 3};
    const double cam[14] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0};
    double cam1[14] = {0, 0, 0, 2, 0.1, 0, -1, 0, 0.1, 0, 1, 0.2, 0, -1};
    double pts[9] = {1, 0.5, 10, -2, 0.25, 20, 0, 0, 15};
    double uv0[6] = {679, 221, 535, 194, 607, 185}, uv1[6] = {650, 221, 520, 194, 600, 185};
    CHECK(sim3opt_ba_batch_optimize(h) == SIM3OPT_ERR_STATE);  // nothing set
    CHECK(sim3opt_ba_batch_set_problems(h, 2, ptr, cam, cam1, pts, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_OK);
    int32_t n = 0, total = 0;
    CHECK(sim3opt_ba_batch_dims(h, &n, &total) == SIM3OPT_OK && n == 2 && total == 3);
    double c0[14], c1[14], p[9];
    CHECK(sim3opt_ba_batch_get_cameras(h, c0, c1) == SIM3OPT_OK && c1[3] == 1.0 && c0[3] == 1.0);  // normalised
    auto unchanged = [&]() {
      double d0[14], d1[14], q[9];
      int32_t nn = 0, tt = 0;
      if (sim3opt_ba_batch_dims(h, &nn, &tt) != SIM3OPT_OK || nn != 2 || tt != 3) return false;
      if (sim3opt_ba_batch_get_cameras(h, d0, d1) != SIM3OPT_OK || sim3opt_ba_batch_get_points(h, q) != SIM3OPT_OK)
        return false;
      for (int i = 0; i < 14; ++i)
        if (d0[i] != c0[i] || d1[i] != c1[i]) return false;
      for (int i = 0; i < 9; ++i)
        if (q[i] != p[i]) return false;
      return true;
    };
    CHECK(sim3opt_ba_batch_get_points(h, p) == SIM3OPT_OK && p[8] == 15.0);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int32_t empty[3] = {0, 0, 3}, back[3] = {0, 3, 2};
    CHECK(sim3opt_ba_batch_set_problems(h, 0, ptr, cam, cam1, pts, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_ba_batch_set_problems(h, 2, empty, cam, cam1, pts, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_ba_batch_set_problems(h, 2, back, cam, cam1, pts, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    pts[4] = nan;
    CHECK(sim3opt_ba_batch_set_problems(h, 2, ptr, cam, cam1, pts, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    pts[4] = 0.25;
    uv1[5] = inf;
    CHECK(sim3opt_ba_batch_set_problems(h, 2, ptr, cam, cam1, pts, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    uv1[5] = 185;
    cam1[11] = nan;
    CHECK(sim3opt_ba_batch_set_problems(h, 2, ptr, cam, cam1, pts, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    cam1[11] = 0.2;
    CHECK(sim3opt_ba_batch_set_problems(h, 2, ptr, cam, cam1, pts, uv0, uv1, 0.0, K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_ba_batch_set_problems(h, 2, ptr, cam, nullptr, pts, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    sim3opt_ba_batch_options o;
    sim3opt_ba_batch_options_default(&o);
    o.max_iters = 0;
    CHECK(sim3opt_ba_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.max_iters = 10; o.max_trials = 0;
    CHECK(sim3opt_ba_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.max_trials = 5; o.pixel_noise = 0.0;
    CHECK(sim3opt_ba_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.pixel_noise = 1.0;
    CHECK(sim3opt_ba_batch_set_options(h, &o) == SIM3OPT_OK && unchanged());
    CHECK(sim3opt_ba_batch_get_chi2(h, c0, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);  // no run yet
    CHECK(sim3opt_ba_batch_num_iterations(h, 0) == 0);
    sim3opt_ba_batch_destroy(h);
  }
  std::printf("two_view_conformance host: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

bool rd(FILE* f, double& v) { return std::fscanf(f, "%lf", &v) == 1; }

int run_part(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
  int n = 0;
  double Kf[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1};
  if (std::fscanf(f, "%d %lf %lf %lf", &n, &Kf[0], &Kf[2], &Kf[5]) != 4 || n < 1) { std::fclose(f); return 2; }
  Kf[4] = Kf[0];
  struct Expect {
    std::vector<int> trials;
    std::vector<double> chi2, pts;
    double q[4], t[3];
    int outliers;
  };
  std::vector<Expect> want(n);
  sim3opt_shim::TwoViewRefiner r;
  bool ok = true;
  for (int k = 0; k < n && ok; ++k) {
    int np = 0, iters = 0;
    ok = std::fscanf(f, "%d %d", &np, &iters) == 2 && np > 0 && iters > 0;
    double R[9], t[3];
    for (int i = 0; i < 9 && ok; ++i) ok = rd(f, R[i]);
    for (int i = 0; i < 3 && ok; ++i) ok = rd(f, t[i]);
    std::vector<P3d> xyz(ok ? np : 0);
    std::vector<P2d> a(xyz.size()), b(xyz.size());
    for (std::size_t i = 0; i < xyz.size() && ok; ++i)
      ok = rd(f, xyz[i].x) && rd(f, xyz[i].y) && rd(f, xyz[i].z) && rd(f, a[i].x) && rd(f, a[i].y) && rd(f, b[i].x) && rd(f, b[i].y);
    Expect& E = want[k];
    E.trials.resize(ok ? iters : 0); E.chi2.resize(E.trials.size()); E.pts.resize(3 * xyz.size());
    for (std::size_t i = 0; i < E.trials.size() && ok; ++i) ok = std::fscanf(f, "%d", &E.trials[i]) == 1;
    for (std::size_t i = 0; i < E.chi2.size() && ok; ++i) ok = rd(f, E.chi2[i]);
    for (int i = 0; i < 4 && ok; ++i) ok = rd(f, E.q[i]);
    for (int i = 0; i < 3 && ok; ++i) ok = rd(f, E.t[i]);
    for (std::size_t i = 0; i < E.pts.size() && ok; ++i) ok = rd(f, E.pts[i]);
    ok = ok && std::fscanf(f, "%d", &E.outliers) == 1;
    if (ok) ok = r.add(xyz, a, b, Kf, R, t) == k;
  }
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "malformed case file %s (%s)\n", path, r.last_error().c_str()); return 2; }
  const int rc = r.optimize();
  if (rc < 0) {
    std::fprintf(stderr, "optimize failed (%d): %s\n", rc, r.last_error().c_str());
    return 3;
  }
  CHECK(rc == n);
  for (int k = 0; k < n; ++k) {
    const Expect& E = want[k];
    CHECK(r.iterations(k) == (int)E.trials.size());
    for (int it = 0; it < r.iterations(k) && it < (int)E.trials.size(); ++it) {
      sim3opt_iter_stats s;
      CHECK(r.stats(k, it, &s));
      CHECK(s.trials == E.trials[it]);
      CHECK(std::fabs(s.chi2_after - E.chi2[it]) <= 1e-7 * E.chi2[it]);
    }
    const double* q = r.quaternion(k);
    double dm = 0, dp = 0;
    for (int i = 0; i < 4; ++i) { dm = std::fmax(dm, std::fabs(q[i] - E.q[i])); dp = std::fmax(dp, std::fabs(q[i] + E.q[i])); }
    CHECK(std::fmin(dm, dp) < 1e-8);
    for (int i = 0; i < 3; ++i) CHECK(std::fabs(r.translation(k)[i] - E.t[i]) < 1e-7);
    double worst = 0;
    for (std::size_t i = 0; i < E.pts.size(); ++i) worst = std::fmax(worst, std::fabs(r.points(k)[i] - E.pts[i]));
    CHECK(worst < 1e-6);
    CHECK(r.n_incorrect_edges(k) == E.outliers);
    CHECK(r.init_error(k) > 0 && r.final_error(k) > 0);
    double R[9];
    r.rotation(k, R);
    CHECK(std::fabs(R[0] * R[0] + R[3] * R[3] + R[6] * R[6] - 1.0) < 1e-12);
  }
  std::printf("two_view_conformance run: %d candidates, %d checks, %d failed\n", n, g_checks, g_failed);
  return g_failed ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "host") return host_part();
  if (mode == "run" && argc > 2) return run_part(argv[2]);
  std::fprintf(stderr, "usage: %s host | run FILE\n", argv[0]);
  return 2;
}
