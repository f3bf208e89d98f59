// match_host_driver.cpp -- the host half of the batched descriptor matching (csrc/match_host.hpp: the checks of what a
// caller hands over and the builder of the tile table) as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer: no GPU and no HIP.  Every refusal the header documents, then plans of ragged pairs whose
// tables are checked entry by entry, the arrays sized exactly so that a read past an end is the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../sim3opt_amd/csrc/match_host.hpp"

using namespace sim3opt_match;

static int failed = 0, checks = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    ++checks;                                                         \
    if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } \
  } while (0)

struct Frames {  // heap arrays of exactly the sizes the pointer arrays name
  std::vector<int32_t> kp_ptr, obs_ptr;
  std::unique_ptr<float[]> kp, desc, obs_uv, obs_depth;
  size_t nk = 0, no = 0;
  Frames(std::vector<int32_t> kn, std::vector<int32_t> on) {
    kp_ptr.push_back(0); obs_ptr.push_back(0);
    for (int32_t n : kn) kp_ptr.push_back(kp_ptr.back() + n);
    for (int32_t n : on) obs_ptr.push_back(obs_ptr.back() + n);
    nk = (size_t)kp_ptr.back(); no = (size_t)obs_ptr.back();
    kp.reset(new float[2 * nk + 1]()); desc.reset(new float[DESC * nk + 1]());
    obs_uv.reset(new float[2 * no + 1]()); obs_depth.reset(new float[no + 1]());
  }
  int32_t n() const { return (int32_t)kp_ptr.size() - 1; }
  std::string check(double f = 700, double cx = 600, double cy = 180, int32_t w = 1241, int32_t h = 376) const {
    return validate_frames(n(), kp_ptr.data(), obs_ptr.data(), kp.get(), desc.get(), obs_uv.get(), obs_depth.get(), f,
                           cx, cy, w, h);
  }
};

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // ---- options
  sim3opt_match_batch_options o{0.0, 0.1, 1.0 / 3, 0.25, 6, -1};
  CHECK(validate_options(o).empty());
  for (int k : {0, -1, MAX_K + 1}) { auto p = o; p.knn_k = k; CHECK(!validate_options(p).empty()); }
  for (int k : {1, MAX_K}) { auto p = o; p.knn_k = k; CHECK(validate_options(p).empty()); }
  { auto p = o; p.ratio = -1e-300; CHECK(!validate_options(p).empty()); }
  { auto p = o; p.border_ratio = nan; CHECK(!validate_options(p).empty()); }
  { auto p = o; p.skew_x = inf; CHECK(!validate_options(p).empty()); }
  { auto p = o; p.skew_y = -0.25; CHECK(!validate_options(p).empty()); }
  // ---- frames
  Frames F({3, 0, 300, 1}, {2, 5, 0, 1030});
  CHECK(F.check().empty());
  CHECK(!F.check(0.0).empty() && !F.check(-1.0).empty() && !F.check(nan).empty());
  CHECK(!F.check(700, inf).empty() && !F.check(700, 600, nan).empty());
  CHECK(!F.check(700, 600, 180, 0).empty() && !F.check(700, 600, 180, 1241, -1).empty());
  CHECK(!validate_frames(0, F.kp_ptr.data(), F.obs_ptr.data(), F.kp.get(), F.desc.get(), F.obs_uv.get(),
                         F.obs_depth.get(), 700, 600, 180, 1241, 376).empty());
  CHECK(!validate_frames(F.n(), nullptr, F.obs_ptr.data(), F.kp.get(), F.desc.get(), F.obs_uv.get(), F.obs_depth.get(),
                         700, 600, 180, 1241, 376).empty());
  CHECK(!validate_frames(F.n(), F.kp_ptr.data(), F.obs_ptr.data(), F.kp.get(), nullptr, F.obs_uv.get(),
                         F.obs_depth.get(), 700, 600, 180, 1241, 376).empty());
  CHECK(!validate_frames(F.n(), F.kp_ptr.data(), F.obs_ptr.data(), F.kp.get(), F.desc.get(), F.obs_uv.get(), nullptr,
                         700, 600, 180, 1241, 376).empty());
  // the last number of every array, the one a loop that stops one short would miss
  F.kp[2 * F.nk - 1] = nan; CHECK(!F.check().empty()); F.kp[2 * F.nk - 1] = 1;
  F.desc[DESC * F.nk - 1] = inf; CHECK(!F.check().empty()); F.desc[DESC * F.nk - 1] = 1;
  F.obs_uv[2 * F.no - 1] = -inf; CHECK(!F.check().empty()); F.obs_uv[2 * F.no - 1] = 1;
  F.obs_depth[F.no - 1] = nan; CHECK(!F.check().empty()); F.obs_depth[F.no - 1] = 1;
  // ... and the one past it, which no check may read as part of the arrays (the arrays hold one spare element)
  F.kp[2 * F.nk] = nan; F.desc[DESC * F.nk] = nan; F.obs_uv[2 * F.no] = nan; F.obs_depth[F.no] = nan;
  CHECK(F.check().empty());
  { Frames G({3, 2}, {1, 1}); G.kp_ptr[0] = 1; CHECK(!G.check().empty()); }
  { Frames G({3, 2}, {1, 1}); G.kp_ptr[2] = 2; CHECK(!G.check().empty()); }
  { Frames G({3, 2}, {1, 1}); G.obs_ptr[1] = 3; CHECK(!G.check().empty()); }
  { Frames G({0}, {0}); CHECK(G.check().empty()); }  // a frame may be empty of both
  // ---- pairs
  const int32_t good[] = {0, 2, 2, 0, 3, 3, 1, 0};
  CHECK(validate_pairs(F.n(), 4, good).empty());
  CHECK(!validate_pairs(F.n(), 0, good).empty() && !validate_pairs(F.n(), 4, nullptr).empty());
  { const int32_t bad[] = {0, 4}; CHECK(!validate_pairs(F.n(), 1, bad).empty()); }
  { const int32_t bad[] = {-1, 0}; CHECK(!validate_pairs(F.n(), 1, bad).empty()); }
  { const int32_t bad[] = {0, 1, 2, INT32_MAX}; CHECK(!validate_pairs(F.n(), 2, bad).empty()); }
  // ---- the plan: F's frames are (3 kp, 2 obs), (0, 5), (300, 0), (1, 1030)
  {
    const int32_t pairs[] = {0, 3, 3, 0, 0, 1, 2, 0, 1, 2, 3, 3, 0, 0};
    Plan P;
    CHECK(build_plan(F.kp_ptr.data(), F.obs_ptr.data(), 7, pairs, P).empty());
    const int32_t st[] = {0, 0, SIM3OPT_MATCH_NO_KEYPOINTS, SIM3OPT_MATCH_NO_MAP, SIM3OPT_MATCH_NO_KEYPOINTS, 0, 0};
    const int32_t q[] = {0, 3, 4, 4, 4, 4, 5, 8}, t[] = {0, 1, 4, 4, 4, 4, 5, 8};
    for (int k = 0; k < 7; ++k) CHECK(P.status[k] == st[k]);
    for (int k = 0; k < 8; ++k) CHECK(P.qptr[k] == q[k] && P.tptr[k] == t[k]);
    CHECK(P.tiles.size() == 4);
    const int32_t tp[] = {0, 1, 5, 6};
    for (size_t k = 0; k < P.tiles.size(); ++k) CHECK(P.tiles[k].pair == tp[k] && P.tiles[k].q0 == 0);
  }
  // ---- tiles of queries round the tile size: every query in exactly one tile, in order
  for (int32_t n : {1, QUERY_TILE - 1, QUERY_TILE, QUERY_TILE + 1, 2 * QUERY_TILE, 2 * QUERY_TILE + 1, 2000}) {
    Frames G({n, 7}, {1, 1});
    const int32_t pairs[] = {0, 1, 1, 0, 0, 0};
    Plan P;
    CHECK(build_plan(G.kp_ptr.data(), G.obs_ptr.data(), 3, pairs, P).empty());
    const size_t per = (size_t)(n + QUERY_TILE - 1) / QUERY_TILE;
    CHECK(P.tiles.size() == 2 * per + 1);
    std::vector<int> seen[3];
    for (int k = 0; k < 3; ++k) seen[k].assign((size_t)(k == 1 ? 7 : n), 0);
    for (const Tile& T : P.tiles) {
      CHECK(T.pair >= 0 && T.pair < 3 && T.q0 % QUERY_TILE == 0);
      const int32_t nq = T.pair == 1 ? 7 : n;
      for (int32_t i = T.q0; i < T.q0 + QUERY_TILE && i < nq; ++i) ++seen[T.pair][(size_t)i];
    }
    for (int k = 0; k < 3; ++k)
      for (int c : seen[k]) CHECK(c == 1);
    CHECK(P.qptr[3] == 2 * n + 7 && P.tptr[3] == 2 * n + 7);
  }
  // ---- more queries than an int32_t indexes: refused, not wrapped
  {
    const std::vector<int32_t> kp_ptr{0, 1 << 20}, obs_ptr{0, 1}, pairs(2 * 2049, 0);
    Plan P;
    CHECK(!build_plan(kp_ptr.data(), obs_ptr.data(), 2049, pairs.data(), P).empty());
    CHECK(build_plan(kp_ptr.data(), obs_ptr.data(), 2047, pairs.data(), P).empty());
    CHECK(P.qptr[2047] == 2047 * (1 << 20) && P.tiles.size() == (size_t)2047 * ((1 << 20) / QUERY_TILE));
  }
  std::printf("%d checks, %d failed\n", checks, failed);
  if (!failed) std::printf("match host ok\n");
  return failed ? 1 : 0;
}
