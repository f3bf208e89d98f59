// Conformance program of include/sim3opt_homography.hpp (HomographyBatch over sim3opt_homography_batch_*), the batched
// replacement of the HomographyInit::Compute call site (kittiDetector.h:1387-1443).
//   homography_conformance host         argument checks of the helper and of the C-ABI; needs no GPU
//   homography_conformance run FILE     HomographyBatch::solve() on the candidates of FILE; rotations and translation
//                                       directions against the planted truth FILE carries; exit 3 with the library's
//                                       message when there is no GPU
// FILE: "n f cx cy iterations rot_bound dir_bound", then per candidate "npts", npts rows "u0 v0 u1 v1", the true
// rotation (9, row-major) and the true unit translation (3).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sim3opt_essential.hpp"  // (the helpers compile side by side)
#include "sim3opt_homography.hpp"

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

struct P2 { float x, y; };  // cv::Point2f's members
struct P2d { double x, y; };

const double K[9] = {718.856, 0, 607.1928, 0, 718.856, 185.2157, 0, 0, 1};

int host_part() {
  using sim3opt_shim::HomographyBatch;
  {
    HomographyBatch e;
    CHECK(e.size() == 0);
    CHECK(e.options().iterations == 300 && e.options().max_pixel_error == 5.0 && e.options().refine_rounds == 5 &&
          e.options().min_points == 10 && e.options().seed == 0 && e.options().device == -1);
    std::vector<P2> a = {{650.f, 221.f}, {520.f, 194.f}}, b = {{640.f, 220.f}, {530.f, 190.f}}, shorter = {{1.f, 2.f}};
    CHECK(e.add(a, shorter, K) == -1 && e.size() == 0 && !e.last_error().empty());
    CHECK(e.add(std::vector<P2>(), std::vector<P2>(), K) == -1 && e.size() == 0);
    CHECK(e.add(a, b, nullptr) == -1 && e.size() == 0);
    CHECK(e.add(a, b, K) == 0 && e.size() == 1 && e.n_points(0) == 2);
    const double K2[9] = {700, 0, 600, 0, 700, 180, 0, 0, 1};
    CHECK(e.add(a, b, K2) == -1 && e.size() == 1);  // one K per batch
    CHECK(e.add(a, b, K) == 1 && e.size() == 2);
    CHECK(e.status(0) == -1 && !e.good(0) && e.n_inliers(0) == 0 && !e.inlier(0, 1) && e.quaternion(1)[3] == 1.0 &&
          e.translation(1)[2] == 0.0 && e.homography(1)[0] == 0.0 && e.homography(1)[8] == 0.0);
    e.options().iterations = 0;
    CHECK(e.solve() == SIM3OPT_ERR_ARG && !e.last_error().empty());
    e.clear();
    CHECK(e.size() == 0);
    e.options().iterations = 100;
    CHECK(e.solve() == SIM3OPT_ERR_ARG);  // nothing to solve
  }
  {  // the C-ABI: every refusal leaves the handle as it was
    sim3opt_homography_batch* h = sim3opt_homography_batch_create();
    CHECK(h != nullptr);
    double uv0[10] = {650, 221, 520, 194, 600, 180, 700, 240, 500, 100};
    double uv1[10] = {640, 220, 530, 190, 610, 182, 690, 238, 505, 104};
    int32_t ptr[3] = {0, 2, 5}, empty[3] = {0, 0, 5}, back[3] = {0, 3, 2}, off[3] = {1, 2, 5};
    CHECK(sim3opt_homography_batch_solve(h) == SIM3OPT_ERR_STATE);  // nothing set
    CHECK(sim3opt_homography_batch_set_problems(h, 2, ptr, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_OK);
    auto unchanged = [&]() {
      int32_t n = 0, t = 0, tiles[2] = {0, 0};
      return sim3opt_homography_batch_dims(h, &n, &t, tiles) == SIM3OPT_OK && n == 2 && t == 5 && tiles[0] >= 1047 &&
             tiles[1] >= 1;
    };
    CHECK(unchanged());
    CHECK(sim3opt_homography_batch_set_problems(h, 0, ptr, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_homography_batch_set_problems(h, 2, empty, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_homography_batch_set_problems(h, 2, back, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_homography_batch_set_problems(h, 2, off, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_homography_batch_set_problems(h, 2, ptr, nullptr, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_homography_batch_set_problems(h, 2, ptr, uv0, uv1, 0.0, K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    uv0[4] = NAN;
    CHECK(sim3opt_homography_batch_set_problems(h, 2, ptr, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    uv0[4] = 600;
    uv1[9] = INFINITY;
    CHECK(sim3opt_homography_batch_set_problems(h, 2, ptr, uv0, uv1, K[0], K[2], K[5]) == SIM3OPT_ERR_ARG && unchanged());
    uv1[9] = 104;
    sim3opt_homography_batch_options o;
    sim3opt_homography_batch_options_default(&o);
    o.iterations = 4097;
    CHECK(sim3opt_homography_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.iterations = 100; o.min_points = 3;
    CHECK(sim3opt_homography_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.min_points = 10; o.max_pixel_error = NAN;
    CHECK(sim3opt_homography_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.max_pixel_error = 2.0; o.refine_rounds = 9;
    CHECK(sim3opt_homography_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.refine_rounds = 3; o.seed = 77;
    CHECK(sim3opt_homography_batch_set_options(h, &o) == SIM3OPT_OK && unchanged());
    double pose[14], H[18];
    uint8_t mask[5];
    int32_t cnt[2];
    CHECK(sim3opt_homography_batch_get_poses(h, pose) == SIM3OPT_ERR_STATE);  // no solve yet
    CHECK(sim3opt_homography_batch_get_homographies(h, H, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_homography_batch_get_inliers(h, mask, cnt) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_homography_batch_get_summary(h, cnt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_homography_batch_debug_hypotheses(h, 0, nullptr, cnt, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_homography_batch_debug_score(h, 0, H, cnt, nullptr) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_homography_batch_debug_refine(h, nullptr, mask, pose, nullptr) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_homography_batch_debug_decompose(h, nullptr, mask, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                   nullptr, nullptr, nullptr) == SIM3OPT_ERR_ARG);
    sim3opt_homography_batch_destroy(h);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

int run_part(const char* path) {
  std::FILE* fp = std::fopen(path, "r");
  if (!fp) return 2;
  int n, iterations;
  double f, cx, cy, rot_bound, dir_bound;
  if (std::fscanf(fp, "%d %lf %lf %lf %d %lf %lf", &n, &f, &cx, &cy, &iterations, &rot_bound, &dir_bound) != 7 || n < 1) return 2;
  const double Kf[9] = {f, 0, cx, 0, f, cy, 0, 0, 1};
  sim3opt_shim::HomographyBatch e;
  e.options().iterations = iterations;
  std::vector<std::vector<double>> truth(n, std::vector<double>(12));
  for (int k = 0; k < n; ++k) {
    int m;
    if (std::fscanf(fp, "%d", &m) != 1 || m < 1) return 2;
    std::vector<P2d> a(m), b(m);
    for (int i = 0; i < m; ++i)
      if (std::fscanf(fp, "%lf %lf %lf %lf", &a[i].x, &a[i].y, &b[i].x, &b[i].y) != 4) return 2;
    for (double& v : truth[k])
      if (std::fscanf(fp, "%lf", &v) != 1) return 2;
    CHECK(e.add(a, b, Kf) == k);
  }
  std::fclose(fp);
  const int ok = e.solve();
  if (ok == SIM3OPT_ERR_NO_DEVICE) {
    std::fprintf(stderr, "%s\n", e.last_error().c_str());
    return 3;
  }
  CHECK(ok == n);
  for (int k = 0; k < n && ok >= 0; ++k) {
    CHECK(e.status(k) == SIM3OPT_HOMOGRAPHY_OK && e.good(k));
    double R[9];
    e.rotation(k, R);
    double tr = 0.0, dot = 0.0, nt = 0.0, cross = 0.0;
    for (int i = 0; i < 9; ++i) tr += R[i] * truth[k][i];  // trace(R_true^T R)
    for (int i = 0; i < 3; ++i) {
      dot += e.translation(k)[i] * truth[k][9 + i];
      nt += e.translation(k)[i] * e.translation(k)[i];
      cross += e.translation(k)[i] * e.translation_as_computed(k)[i];
    }
    const double rot = std::acos(std::fmin(1.0, std::fmax(-1.0, 0.5 * (tr - 1.0))));
    const double dir = std::acos(std::fmin(1.0, std::fmax(-1.0, dot)));
    std::printf("candidate %d: %d points, %d inliers, rotation %.3e rad, direction %.3e rad\n", k, e.n_points(k),
                e.n_inliers(k), rot, dir);
    CHECK(rot <= rot_bound);
    CHECK(dir <= dir_bound);
    CHECK(std::fabs(nt - 1.0) < 1e-12 && cross > 0.0);  // the unit vector of :1431, along t as computed
    int counted = 0;
    for (int i = 0; i < e.n_points(k); ++i) counted += e.inlier(k, i) ? 1 : 0;
    CHECK(counted == e.n_inliers(k) && counted > e.n_points(k) / 2);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "host") return host_part();
  if (argc == 3 && std::string(argv[1]) == "run") return run_part(argv[2]);
  std::fprintf(stderr, "usage: homography_conformance host | run FILE\n");
  return 2;
}
