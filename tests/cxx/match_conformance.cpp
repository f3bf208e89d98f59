// Conformance program of include/sim3opt_match.hpp (LoopMatchBatch over sim3opt_match_batch_*), the batched
// replacement of the descriptor matching, its filters and the map-depth lookup of computeConstraints
// (kittiDetector.h:1085-1160, :1229-1279), composed with include/sim3opt_pnp.hpp and include/sim3opt_two_view.hpp as
// a call site composes them: matches -> PnP -> two-view refinement -> sloop.
//   match_conformance host         argument checks of the helper and of the C-ABI; needs no GPU
//   match_conformance run FILE     planted candidates of FILE through LoopMatchBatch::solve(), feed(PnpRansacBatch),
//                                  TwoViewRefiner; the planted matches, pose and depth ratio come back; exit 3 with
//                                  the library's message when there is no GPU
// FILE: "n f cx cy width height rot_bound t_bound", then per candidate "npts ratio", npts rows
// "u0 v0 z0 u1 v1 z1 kept" (a point's pixel and map depth in either keyframe, and whether the border and skew filters
// keep it), the true quaternion x y z w and translation of camera 1.  Descriptors are made here: point i's is a
// pseudo-random unit vector, keyframe 1 lists the points in reverse order with the descriptors slightly off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sim3opt_match.hpp"
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

struct P2 { float x, y; };  // cv::Point2f's members

const double K[9] = {718.856, 0, 607.1928, 0, 718.856, 185.2157, 0, 0, 1};

uint32_t g_state = 12345u;
float uniform() {  // [-1, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)((g_state >> 8) * (1.0 / 8388608.0) - 1.0);
}

std::vector<float> descriptors(int n) {
  std::vector<float> d(64 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    double s = 0;
    for (int k = 0; k < 64; ++k) { d[64 * (size_t)i + k] = uniform(); s += (double)d[64 * (size_t)i + k] * d[64 * (size_t)i + k]; }
    for (int k = 0; k < 64; ++k) d[64 * (size_t)i + k] = (float)(d[64 * (size_t)i + k] / std::sqrt(s));
  }
  return d;
}

int host_part() {
  using sim3opt_shim::LoopMatchBatch;
  // ---- the helper ----
  {
    LoopMatchBatch m(K, 1241, 376);
    CHECK(m.n_frames() == 0 && m.n_pairs() == 0);
    CHECK(m.options().ratio == 0.0 && m.options().border_ratio == 0.1 && m.options().skew_x == 1.0 / 3.0 &&
          m.options().skew_y == 0.25 && m.options().knn_k == 6 && m.options().device == -1);
    std::vector<P2> keys = {{300.f, 200.f}, {500.f, 150.f}}, obs = {{310.f, 205.f}}, none;
    std::vector<float> z = {12.f}, two = {1.f, 2.f}, nz;
    const std::vector<float> d = descriptors(2);
    CHECK(m.add_frame(keys, nullptr, obs, z) == -1 && m.n_frames() == 0 && !m.last_error().empty());
    CHECK(m.add_frame(keys, d.data(), obs, two) == -1 && m.n_frames() == 0);
    CHECK(m.add_frame(keys, d.data(), obs, z) == 0 && m.n_frames() == 1);
    CHECK(m.add_frame(none, nullptr, none, nz) == 1 && m.n_frames() == 2);  // a keyframe may be empty
    CHECK(m.add_pair(0, 2) == -1 && m.add_pair(-1, 0) == -1 && m.n_pairs() == 0);
    CHECK(m.status(0) == -1 && m.n_matches(0) == 0);
    CHECK(m.solve() == SIM3OPT_ERR_ARG && !m.last_error().empty());  // no pairs
    CHECK(m.add_pair(0, 1) == 0 && m.add_pair(0, 0) == 1 && m.n_pairs() == 2);
    m.options().knn_k = 17;
    CHECK(m.solve() == SIM3OPT_ERR_ARG);
    sim3opt_shim::PnpRansacBatch pnp;
    const std::vector<int> id = m.feed(pnp);  // nothing solved: nothing handed over
    CHECK(id.size() == 2 && id[0] == -1 && id[1] == -1 && pnp.size() == 0);
  }
  {
    sim3opt_shim::LoopMatchBatch m(K, 0, 376);
    std::vector<P2> keys = {{300.f, 200.f}}, obs = {{310.f, 205.f}};
    std::vector<float> z = {12.f};
    const std::vector<float> d = descriptors(1);
    CHECK(m.add_frame(keys, d.data(), obs, z) == 0 && m.add_pair(0, 0) == 0);
    CHECK(m.solve() == SIM3OPT_ERR_ARG);  // a non-positive image size
  }
  // ---- the C-ABI: every refusal leaves the handle as it was ----
  {
    sim3opt_match_batch* h = sim3opt_match_batch_create();
    CHECK(h != nullptr);
    const std::vector<float> d = descriptors(5);
    float kp[10] = {300, 200, 500, 150, 640, 180, 700, 240, 500, 100}, ouv[6] = {310, 205, 400, 100, 650, 185};
    float od[3] = {12, 20, 30};
    int32_t kptr[4] = {0, 2, 2, 5}, optr[4] = {0, 1, 3, 3}, back[4] = {0, 3, 2, 5}, off[4] = {1, 2, 2, 5};
    int32_t pairs[4] = {0, 2, 2, 2}, far[2] = {0, 3}, neg[2] = {-1, 0};
    CHECK(sim3opt_match_batch_solve(h) == SIM3OPT_ERR_STATE);                // nothing set
    CHECK(sim3opt_match_batch_set_pairs(h, 2, pairs) == SIM3OPT_ERR_STATE);  // frames first
    const auto set = [&](int32_t n, const int32_t* a, const int32_t* b, const float* k, const float* de, const float* u,
                         const float* z, double f, int32_t w, int32_t hh) {
      return sim3opt_match_batch_set_frames(h, n, a, b, k, de, u, z, f, K[2], K[5], w, hh);
    };
    CHECK(set(3, kptr, optr, kp, d.data(), ouv, od, K[0], 1241, 376) == SIM3OPT_OK);
    CHECK(sim3opt_match_batch_set_pairs(h, 2, pairs) == SIM3OPT_OK);
    auto unchanged = [&]() {
      int32_t nf = 0, np = 0, nk = 0, no = 0, t[4] = {0, 0, 0, 0};
      return sim3opt_match_batch_dims(h, &nf, &np, &nk, &no, t) == SIM3OPT_OK && nf == 3 && np == 2 && nk == 5 &&
             no == 3 && t[0] == 64 && t[1] > 0 && t[1] % t[0] == 0 && t[2] > 0 && t[3] > 0;
    };
    CHECK(unchanged());
    CHECK(set(0, kptr, optr, kp, d.data(), ouv, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, back, optr, kp, d.data(), ouv, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, off, optr, kp, d.data(), ouv, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, kptr, back, kp, d.data(), ouv, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, nullptr, optr, kp, d.data(), ouv, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, kptr, optr, nullptr, d.data(), ouv, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, kptr, optr, kp, nullptr, ouv, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, kptr, optr, kp, d.data(), nullptr, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, kptr, optr, kp, d.data(), ouv, nullptr, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, kptr, optr, kp, d.data(), ouv, od, 0.0, 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, kptr, optr, kp, d.data(), ouv, od, K[0], 0, 376) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(set(3, kptr, optr, kp, d.data(), ouv, od, K[0], 1241, -1) == SIM3OPT_ERR_ARG && unchanged());
    kp[9] = NAN;
    CHECK(set(3, kptr, optr, kp, d.data(), ouv, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    kp[9] = 100; od[2] = INFINITY;
    CHECK(set(3, kptr, optr, kp, d.data(), ouv, od, K[0], 1241, 376) == SIM3OPT_ERR_ARG && unchanged());
    od[2] = 30;
    CHECK(sim3opt_match_batch_set_pairs(h, 0, pairs) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_match_batch_set_pairs(h, 1, nullptr) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_match_batch_set_pairs(h, 1, far) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_match_batch_set_pairs(h, 1, neg) == SIM3OPT_ERR_ARG && unchanged());
    sim3opt_match_batch_options o;
    sim3opt_match_batch_options_default(&o);
    o.knn_k = 0;
    CHECK(sim3opt_match_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.knn_k = 17;
    CHECK(sim3opt_match_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.knn_k = 6; o.ratio = -1.0;
    CHECK(sim3opt_match_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.ratio = 0.0; o.skew_y = NAN;
    CHECK(sim3opt_match_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.skew_y = 0.25; o.border_ratio = -0.1;
    CHECK(sim3opt_match_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.border_ratio = 0.05; o.ratio = 1.4; o.knn_k = 16;
    CHECK(sim3opt_match_batch_set_options(h, &o) == SIM3OPT_OK && unchanged());
    int32_t ptr[3], idx[8];
    float fl[8];
    double db[8];
    CHECK(sim3opt_match_batch_get_match_ptr(h, ptr) == SIM3OPT_ERR_STATE);  // no solve yet
    CHECK(sim3opt_match_batch_get_matches(h, idx, idx, fl, db, db, db, db, db) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_match_batch_get_summary(h, ptr, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_match_batch_debug_nn(h, 0, idx, fl, idx, fl) == SIM3OPT_ERR_STATE);
    const float px[2] = {100, 100}, bad_px[2] = {NAN, 100};
    CHECK(sim3opt_match_batch_debug_depth(h, 0, 0, px, db, idx) == SIM3OPT_ERR_ARG);       // n < 1
    CHECK(sim3opt_match_batch_debug_depth(h, 1, 3, px, db, idx) == SIM3OPT_ERR_ARG);       // no such frame
    CHECK(sim3opt_match_batch_debug_depth(h, 1, 2, px, db, idx) == SIM3OPT_ERR_ARG);       // a frame without observations
    CHECK(sim3opt_match_batch_debug_depth(h, 1, 0, bad_px, db, idx) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_match_batch_debug_depth(h, 1, 0, nullptr, db, idx) == SIM3OPT_ERR_ARG);
    sim3opt_match_batch_destroy(h);
    sim3opt_match_batch_destroy(nullptr);
  }
  std::printf("match_conformance host: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

bool rd(FILE* f, double& v) { return std::fscanf(f, "%lf", &v) == 1; }

int run_part(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
  int n = 0, width = 0, height = 0;
  double Kf[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1}, rot_bound = 0, t_bound = 0;
  if (std::fscanf(f, "%d %lf %lf %lf %d %d %lf %lf", &n, &Kf[0], &Kf[2], &Kf[5], &width, &height, &rot_bound,
                  &t_bound) != 8 || n < 1) {
    std::fclose(f);
    return 2;
  }
  Kf[4] = Kf[0];
  struct Candidate {
    std::vector<int> kept;  // the points the filters keep, ascending
    double ratio, q[4], t[3];
    int npts;
  };
  std::vector<Candidate> cand(n);
  sim3opt_shim::LoopMatchBatch match(Kf, width, height);
  match.options().knn_k = 1;  // every keypoint is an observation of its keyframe: a match's depth is its point's
  bool ok = true;
  for (int k = 0; k < n && ok; ++k) {
    Candidate& C = cand[k];
    ok = std::fscanf(f, "%d %lf", &C.npts, &C.ratio) == 2 && C.npts > 0;
    const int np = ok ? C.npts : 0;
    std::vector<P2> k0(np), k1(np);
    std::vector<double> z0(np), z1(np);
    for (int i = 0; i < np && ok; ++i) {
      double u0, v0, u1, v1, kept;
      ok = rd(f, u0) && rd(f, v0) && rd(f, z0[i]) && rd(f, u1) && rd(f, v1) && rd(f, z1[np - 1 - i]) && rd(f, kept);
      k0[i] = P2{(float)u0, (float)v0};
      k1[np - 1 - i] = P2{(float)u1, (float)v1};  // keyframe 1 lists the points in reverse
      if (kept != 0) C.kept.push_back(i);
    }
    for (int i = 0; i < 4 && ok; ++i) ok = rd(f, C.q[i]);
    for (int i = 0; i < 3 && ok; ++i) ok = rd(f, C.t[i]);
    if (!ok) break;
    const std::vector<float> d0 = descriptors(np);
    std::vector<float> d1(d0.size());
    for (int i = 0; i < np; ++i)
      for (int c = 0; c < 64; ++c) d1[64 * (size_t)(np - 1 - i) + c] = d0[64 * (size_t)i + c] + 1e-3f * uniform();
    const int f0 = match.add_frame(k0, d0.data(), k0, z0), f1 = match.add_frame(k1, d1.data(), k1, z1);
    ok = f0 == 2 * k && f1 == 2 * k + 1 && match.add_pair(f0, f1) == k;
  }
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "malformed candidate file %s (%s)\n", path, match.last_error().c_str()); return 2; }
  int rc = match.solve();  // after the loop: every candidate
  if (rc < 0) {
    std::fprintf(stderr, "solve failed (%d): %s\n", rc, match.last_error().c_str());
    return 3;
  }
  CHECK(rc == n);
  for (int k = 0; k < n; ++k) {
    const Candidate& C = cand[k];
    CHECK(match.status(k) == SIM3OPT_MATCH_OK);
    CHECK(match.n_matches(k) == (int)C.kept.size());
    bool planted = match.n_matches(k) == (int)C.kept.size();
    for (int i = 0; planted && i < match.n_matches(k); ++i)
      planted = match.query_idx(k, i) == C.kept[i] && match.train_idx(k, i) == C.npts - 1 - C.kept[i];
    CHECK(planted);
    CHECK(match.depth_ratio(k) == C.ratio);  // sloop, :1305-1311
  }
  sim3opt_shim::PnpRansacBatch pnp;
  const std::vector<int> pid = match.feed(pnp);  // the calls at :1300
  CHECK((int)pid.size() == n && pnp.size() == n);
  rc = pnp.solve();
  if (rc < 0) {
    std::fprintf(stderr, "PnP failed (%d): %s\n", rc, pnp.last_error().c_str());
    return 3;
  }
  CHECK(rc == n);
  sim3opt_shim::TwoViewRefiner refiner;
  for (int k = 0; k < n; ++k) {
    CHECK(pid[k] == k && pnp.status(k) == SIM3OPT_PNP_OK && pnp.n_inliers(k) == match.n_matches(k));
    double Rf2s[9];
    pnp.rotation(k, Rf2s);
    std::vector<sim3opt_shim::LoopMatchBatch::P3> xyz;
    std::vector<sim3opt_shim::LoopMatchBatch::P2> a, b;
    for (int i = 0; i < match.n_matches(k); ++i) {
      xyz.push_back(match.surf_point(k, i)); a.push_back(match.point1(k, i)); b.push_back(match.point2(k, i));
    }
    CHECK(refiner.add(xyz, a, b, Kf, Rf2s, pnp.translation(k)) == k);  // the call at :1325
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
    std::printf("candidate %d: %d points, %d matches, refined pose %.3e rad, %.3e m from the truth, depth ratio %.6f\n",
                k, cand[k].npts, match.n_matches(k), ang, dt, match.depth_ratio(k));
    CHECK(ang <= rot_bound);
    CHECK(dt <= t_bound);
  }
  std::printf("match_conformance run: %d candidates, %d checks, %d failed\n", n, g_checks, g_failed);
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
