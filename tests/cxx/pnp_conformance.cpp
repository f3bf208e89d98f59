// Conformance program of include/sim3opt_pnp.hpp (PnpRansacBatch over sim3opt_pnp_batch_*), the batched replacement
// of cv::solvePnPRansac (kittiDetector.h:1300-1301), composed with include/sim3opt_two_view.hpp as a call site
// composes them: the PnP poses are the start of the two-view refinement (:1325).
//   pnp_conformance host         argument checks of the helper and of the C-ABI; needs no GPU
//   pnp_conformance run FILE     PnpRansacBatch::solve() on the candidates of FILE, its rotations, translations and
//                                inliers to TwoViewRefiner::add, optimize(), and the refined poses against the planted
//                                truth FILE carries; exit 3 with the library's message when there is no GPU
// FILE: "n f cx cy rot_bound t_bound", then per candidate "npts", npts rows "X Y Z u0 v0 u1 v1", the true quaternion
// x y z w and translation of camera 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sim3opt_pnp.hpp"
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

int host_part() {
  using sim3opt_shim::PnpRansacBatch;
  // ---- the helper ----
  {
    PnpRansacBatch p;
    CHECK(p.size() == 0);
    CHECK(p.options().iterations == 100 && p.options().reproj_error == 3.0 && p.options().min_inliers == 10 &&
          p.options().min_points == 9 && p.options().refine_iters == 10 && p.options().max_trials == 5 &&
          p.options().tau == 1e-5 && p.options().seed == 0 && p.options().device == -1);
    std::vector<P3> xyz = {{1.f, 0.5f, 10.f}, {-2.f, 0.25f, 20.f}};
    std::vector<P2> b = {{650.f, 221.f}, {520.f, 194.f}}, shorter = {{1.f, 2.f}};
    CHECK(p.add(xyz, shorter, K) == -1 && p.size() == 0 && !p.last_error().empty());
    CHECK(p.add(std::vector<P3>(), std::vector<P2>(), K) == -1 && p.size() == 0);
    CHECK(p.add(xyz, b, nullptr) == -1 && p.size() == 0);
    CHECK(p.add(xyz, b, K) == 0 && p.size() == 1 && p.n_points(0) == 2);
    const double K2[9] = {700, 0, 600, 0, 700, 180, 0, 0, 1};
    CHECK(p.add(xyz, b, K2) == -1 && p.size() == 1);  // one K per batch
    CHECK(p.add(xyz, b, K) == 1 && p.size() == 2);
    CHECK(p.status(0) == -1 && p.n_inliers(0) == 0 && !p.inlier(0, 1) && p.quaternion(1)[3] == 1.0 &&
          p.translation(1)[2] == 0.0);
    p.options().iterations = 0;
    CHECK(p.solve() == SIM3OPT_ERR_ARG && !p.last_error().empty());
    p.clear();
    CHECK(p.size() == 0);
    p.options().iterations = 100;
    CHECK(p.solve() == SIM3OPT_ERR_ARG);  // nothing to solve
  }
  // ---- the C-ABI: every refusal leaves the handle as it was ----
  {
    sim3opt_pnp_batch* h = sim3opt_pnp_batch_create();
    CHECK(h != nullptr);
    double pts[15] = {1, 0.5, 10, -2, 0.25, 20, 0, 0, 15, 3, 1, 12, -1, -1, 9};
    double uv[10] = {650, 221, 520, 194, 600, 180, 700, 240, 500, 100};
    int32_t ptr[3] = {0, 2, 5}, empty[3] = {0, 0, 5}, back[3] = {0, 3, 2}, off[3] = {1, 2, 5};
    CHECK(sim3opt_pnp_batch_solve(h) == SIM3OPT_ERR_STATE);  // nothing set
    CHECK(sim3opt_pnp_batch_set_problems(h, 2, ptr, pts, uv, K[0], K[2], K[5]) == SIM3OPT_OK);  // 2 and 3 points: accepted
    auto unchanged = [&]() {
      int32_t n = 0, t = 0;
      return sim3opt_pnp_batch_dims(h, &n, &t) == SIM3OPT_OK && n == 2 && t == 5;
    };
    CHECK(unchanged());
    CHECK(sim3opt_pnp_batch_set_problems(h, 0, ptr, pts, uv, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_pnp_batch_set_problems(h, 2, empty, pts, uv, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_pnp_batch_set_problems(h, 2, back, pts, uv, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_pnp_batch_set_problems(h, 2, off, pts, uv, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_pnp_batch_set_problems(h, 2, ptr, nullptr, uv, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_pnp_batch_set_problems(h, 2, ptr, pts, uv, 0.0, K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    pts[4] = NAN;
    CHECK(sim3opt_pnp_batch_set_problems(h, 2, ptr, pts, uv, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    pts[4] = 0.25;
    uv[9] = INFINITY;
    CHECK(sim3opt_pnp_batch_set_problems(h, 2, ptr, pts, uv, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    uv[9] = 100;
    sim3opt_pnp_batch_options o;
    sim3opt_pnp_batch_options_default(&o);
    o.iterations = 4097;
    CHECK(sim3opt_pnp_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.iterations = 100; o.min_points = 3;
    CHECK(sim3opt_pnp_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.min_points = 9; o.reproj_error = NAN;
    CHECK(sim3opt_pnp_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.reproj_error = 2.0; o.seed = 77;
    CHECK(sim3opt_pnp_batch_set_options(h, &o) == SIM3OPT_OK && unchanged());
    double cam[14];
    uint8_t mask[5];
    int32_t cnt[2];
    CHECK(sim3opt_pnp_batch_get_poses(h, cam) == SIM3OPT_ERR_STATE);  // no solve yet
    CHECK(sim3opt_pnp_batch_get_inliers(h, mask, cnt) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_pnp_batch_get_summary(h, cnt, nullptr, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_pnp_batch_debug_hypotheses(h, 0, nullptr, cnt, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    sim3opt_pnp_batch_destroy(h);
  }
  // ---- sloop of :1305-1311: index floor(0.5 n) of each sorted list, second over first ----
  {
    const int32_t ptr[3] = {0, 4, 9};
    const double d0[9] = {4, 1, 3, 2, 10, 50, 20, 40, 30}, d1[9] = {8, 2, 4, 6, 5, 1, 4, 2, 3};
    double r[2] = {0, 0};
    CHECK(sim3opt_median_depth_ratio(2, ptr, d0, d1, r) == SIM3OPT_OK && r[0] == 6.0 / 3.0 && r[1] == 3.0 / 30.0);
    const int32_t bad[3] = {0, 4, 4};
    CHECK(sim3opt_median_depth_ratio(2, bad, d0, d1, r) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_median_depth_ratio(2, ptr, d0, nullptr, r) == SIM3OPT_ERR_ARG);
  }
  std::printf("pnp_conformance host: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

bool rd(FILE* f, double& v) { return std::fscanf(f, "%lf", &v) == 1; }

int run_part(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
  int n = 0;
  double Kf[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1}, rot_bound = 0, t_bound = 0;
  if (std::fscanf(f, "%d %lf %lf %lf %lf %lf", &n, &Kf[0], &Kf[2], &Kf[5], &rot_bound, &t_bound) != 6 || n < 1) {
    std::fclose(f);
    return 2;
  }
  Kf[4] = Kf[0];
  struct Candidate {
    std::vector<P3d> xyz;
    std::vector<P2d> a, b;
    double q[4], t[3];
  };
  std::vector<Candidate> cand(n);
  sim3opt_shim::PnpRansacBatch pnp;
  bool ok = true;
  for (int k = 0; k < n && ok; ++k) {
    int np = 0;
    ok = std::fscanf(f, "%d", &np) == 1 && np > 0;
    Candidate& C = cand[k];
    C.xyz.resize(ok ? np : 0); C.a.resize(C.xyz.size()); C.b.resize(C.xyz.size());
    for (std::size_t i = 0; i < C.xyz.size() && ok; ++i)
      ok = rd(f, C.xyz[i].x) && rd(f, C.xyz[i].y) && rd(f, C.xyz[i].z) && rd(f, C.a[i].x) && rd(f, C.a[i].y) &&
           rd(f, C.b[i].x) && rd(f, C.b[i].y);
    for (int i = 0; i < 4 && ok; ++i) ok = rd(f, C.q[i]);
    for (int i = 0; i < 3 && ok; ++i) ok = rd(f, C.t[i]);
    if (ok) ok = pnp.add(C.xyz, C.b, Kf) == k;  // the call at :1300
  }
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "malformed candidate file %s (%s)\n", path, pnp.last_error().c_str()); return 2; }
  int rc = pnp.solve();  // after the loop: one launch
  if (rc < 0) {
    std::fprintf(stderr, "solve failed (%d): %s\n", rc, pnp.last_error().c_str());
    return 3;
  }
  CHECK(rc == n);
  sim3opt_shim::TwoViewRefiner refiner;
  for (int k = 0; k < n; ++k) {
    CHECK(pnp.status(k) == SIM3OPT_PNP_OK);
    CHECK(pnp.n_inliers(k) >= pnp.n_points(k) / 2);
    int marked = 0;
    for (int i = 0; i < pnp.n_points(k); ++i) marked += pnp.inlier(k, i) ? 1 : 0;
    CHECK(marked == pnp.n_inliers(k));
    double Rf2s[9];
    pnp.rotation(k, Rf2s);
    // the call at :1325, on the matches PnP kept: the gross outliers would pull a Huber refinement with them
    std::vector<P3d> xyz;
    std::vector<P2d> a, b;
    for (int i = 0; i < pnp.n_points(k); ++i)
      if (pnp.inlier(k, i)) { xyz.push_back(cand[k].xyz[i]); a.push_back(cand[k].a[i]); b.push_back(cand[k].b[i]); }
    CHECK(refiner.add(xyz, a, b, Kf, Rf2s, pnp.translation(k)) == k);
  }
  rc = refiner.optimize();
  if (rc < 0) {
    std::fprintf(stderr, "optimize failed (%d): %s\n", rc, refiner.last_error().c_str());
    return 3;
  }
  CHECK(rc == n);
  for (int k = 0; k < n; ++k) {
    const double* q = refiner.quaternion(k);
    double dot = 0, dt = 0;
    for (int i = 0; i < 4; ++i) dot += q[i] * cand[k].q[i];
    const double ang = 2.0 * std::acos(std::fmin(1.0, std::fabs(dot)));
    for (int i = 0; i < 3; ++i) dt = std::fmax(dt, std::fabs(refiner.translation(k)[i] - cand[k].t[i]));
    std::printf("candidate %d: %d points, %d PnP inliers, refined pose %.3e rad, %.3e m from the truth\n", k,
                pnp.n_points(k), pnp.n_inliers(k), ang, dt);
    CHECK(ang <= rot_bound);
    CHECK(dt <= t_bound);
  }
  std::printf("pnp_conformance run: %d candidates, %d checks, %d failed\n", n, g_checks, g_failed);
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
