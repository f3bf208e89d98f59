// Conformance program of include/sim3opt_place.hpp (LoopDetectorBatch over sim3opt_place_batch_*), the batched
// replacement of detector.detectLoop (kittiDetector.h:1663), composed with include/sim3opt_match.hpp as a call site
// composes them: descriptors -> candidates -> pairs of the matching stage.
//   place_conformance host         argument checks of the helper and of the C-ABI; needs no GPU
//   place_conformance run FILE     the keyframes of FILE through LoopDetectorBatch::detect() and feed(LoopMatchBatch);
//                                  the expected status and match of every keyframe come back, and every candidate
//                                  keeps at least 12 matches; exit 3 with the library's message when there is no GPU
// FILE: "n_nodes n_frames", per node "parent word_id weight c0 .. c63", per frame "count" and count rows
// "u v z d0 .. d63" (a keypoint's pixel, its map depth, its descriptor), then per frame "status match".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sim3opt_match.hpp"
#include "sim3opt_place.hpp"

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

struct P2 { float x, y; };

// root, two inner nodes, four leaves: 0 -> 1, 2;  1 -> 3, 4;  2 -> 5, 6
struct SmallTree {
  int32_t parent[7] = {-1, 0, 0, 1, 1, 2, 2}, word_id[7] = {-1, -1, -1, 2, 0, 3, 1};
  double weight[7] = {0, 0, 0, 1, 2, 0.5, 0};
  std::vector<float> centre = std::vector<float>(7 * 64, 0.f);
  SmallTree() {
    const float x[7] = {0, -2, 2, -3, -1, 1, 3};
    for (int i = 0; i < 7; ++i) centre[64 * (size_t)i] = x[i];
  }
};

int host_part() {
  using sim3opt_shim::LoopDetectorBatch;
  SmallTree T;
  // ---- the helper ----
  {
    LoopDetectorBatch p;
    CHECK(p.n_frames() == 0 && p.n_candidates() == 0);
    const sim3opt_place_batch_options& o = p.options();
    CHECK(o.alpha == 0.3 && o.min_nss_factor == 0.005 && o.use_nss == 1 && o.k == 3 && o.dislocal == 20 &&
          o.max_db_results == 50 && o.max_intragroup_gap == 3 && o.min_matches_per_group == 1 &&
          o.max_distance_between_queries == 2 && o.max_distance_between_groups == 3 && o.accumulate == 1 &&
          o.device == -1);
    CHECK(p.result(0).status == -1 && !p.result(0).detection() && p.result(-1).match == -1);
    const std::vector<float> d(2 * 64, 0.25f);
    CHECK(p.add_frame(nullptr, 2) == -1 && p.n_frames() == 0 && !p.last_error().empty());
    CHECK(p.add_frame(d.data(), -1) == -1 && p.n_frames() == 0);
    CHECK(p.add_frame(d.data(), 2) == 0 && p.add_frame(nullptr, 0) == 1 && p.n_frames() == 2);  // a keyframe may be empty
    CHECK(p.detect() == SIM3OPT_ERR_STATE && p.last_error().find("no vocabulary") != std::string::npos);
    CHECK(p.set_vocabulary(7, T.parent, T.centre.data(), T.weight, nullptr) == SIM3OPT_ERR_ARG);
    CHECK(p.last_error() == "place_batch_set_vocabulary: a NULL array");
    T.word_id[6] = 2;
    CHECK(p.set_vocabulary(7, T.parent, T.centre.data(), T.weight, T.word_id) == SIM3OPT_ERR_ARG);
    CHECK(p.last_error() == "place_batch_set_vocabulary: leaf 6: word id 2 is repeated");
    T.word_id[6] = 1;
    CHECK(p.set_vocabulary(7, T.parent, T.centre.data(), T.weight, T.word_id) == SIM3OPT_OK);
    p.options().dislocal = 0;
    CHECK(p.detect() == SIM3OPT_ERR_ARG && p.last_error() == "place_batch_set_options: dislocal < 1");
    const double K[9] = {718.856, 0, 607.1928, 0, 718.856, 185.2157, 0, 0, 1};
    sim3opt_shim::LoopMatchBatch m(K, 1241, 376);
    CHECK(p.feed(m).empty() && m.n_pairs() == 0);  // nothing detected: nothing handed over
  }
  // ---- the C-ABI: every refusal leaves the handle as it was ----
  {
    sim3opt_place_batch* h = sim3opt_place_batch_create();
    CHECK(h != nullptr);
    CHECK(sim3opt_place_batch_solve(h) == SIM3OPT_ERR_STATE);  // nothing set
    const std::vector<float> d(5 * 64, 0.5f);
    int32_t ptr[4] = {0, 2, 2, 5}, back[4] = {0, 3, 2, 5}, off[4] = {1, 2, 2, 5};
    CHECK(sim3opt_place_batch_set_frames(h, 3, ptr, d.data()) == SIM3OPT_OK);
    CHECK(sim3opt_place_batch_solve(h) == SIM3OPT_ERR_STATE);  // no vocabulary
    CHECK(sim3opt_place_batch_set_vocabulary(h, 7, T.parent, T.centre.data(), T.weight, T.word_id) == SIM3OPT_OK);
    auto unchanged = [&]() {
      int32_t nn = 0, nw = 0, de = 0, nf = 0, nd = 0, t[6] = {0, 0, 0, 0, 0, 0};
      return sim3opt_place_batch_dims(h, &nn, &nw, &de, &nf, &nd, t) == SIM3OPT_OK && nn == 7 && nw == 4 && de == 2 &&
             nf == 3 && nd == 5 && t[0] == 64 && t[1] % t[0] == 0 && t[2] % t[1] == 0 && t[3] > 0 && t[4] > 0 && t[5] > 0;
    };
    CHECK(unchanged());
    CHECK(sim3opt_place_batch_set_frames(h, 0, ptr, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_place_batch_set_frames(h, SIM3OPT_PLACE_MAX_FRAMES + 1, ptr, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_place_batch_set_frames(h, 3, back, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_place_batch_set_frames(h, 3, off, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_place_batch_set_frames(h, 3, nullptr, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_place_batch_set_frames(h, 3, ptr, nullptr) == SIM3OPT_ERR_ARG && unchanged());
    {
      std::vector<float> bad = d;
      bad.back() = NAN;
      CHECK(sim3opt_place_batch_set_frames(h, 3, ptr, bad.data()) == SIM3OPT_ERR_ARG && unchanged());
    }
    CHECK(sim3opt_place_batch_set_vocabulary(h, 1, T.parent, T.centre.data(), T.weight, T.word_id) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_place_batch_set_vocabulary(h, 7, nullptr, T.centre.data(), T.weight, T.word_id) == SIM3OPT_ERR_ARG && unchanged());
    {
      SmallTree B;
      B.parent[3] = 3;
      CHECK(sim3opt_place_batch_set_vocabulary(h, 7, B.parent, B.centre.data(), B.weight, B.word_id) == SIM3OPT_ERR_ARG && unchanged());
      B = SmallTree(); B.weight[4] = -1;
      CHECK(sim3opt_place_batch_set_vocabulary(h, 7, B.parent, B.centre.data(), B.weight, B.word_id) == SIM3OPT_ERR_ARG && unchanged());
      B = SmallTree(); B.centre[64 * 6 + 63] = INFINITY;
      CHECK(sim3opt_place_batch_set_vocabulary(h, 7, B.parent, B.centre.data(), B.weight, B.word_id) == SIM3OPT_ERR_ARG && unchanged());
      B = SmallTree(); B.word_id[1] = 0;
      CHECK(sim3opt_place_batch_set_vocabulary(h, 7, B.parent, B.centre.data(), B.weight, B.word_id) == SIM3OPT_ERR_ARG && unchanged());
      B = SmallTree(); B.word_id[5] = -1;
      CHECK(sim3opt_place_batch_set_vocabulary(h, 7, B.parent, B.centre.data(), B.weight, B.word_id) == SIM3OPT_ERR_ARG && unchanged());
    }
    sim3opt_place_batch_options o;
    sim3opt_place_batch_options_default(&o);
    o.max_db_results = 1025;
    CHECK(sim3opt_place_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.max_db_results = 50; o.alpha = NAN;
    CHECK(sim3opt_place_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.alpha = 0.3; o.use_nss = 2;
    CHECK(sim3opt_place_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.use_nss = 0; o.k = 0; o.dislocal = 1;
    CHECK(sim3opt_place_batch_set_options(h, &o) == SIM3OPT_OK && unchanged());
    CHECK(sim3opt_place_batch_set_options(h, nullptr) == SIM3OPT_ERR_ARG);
    int32_t idx[8], np = -1;
    double db[8];
    CHECK(sim3opt_place_batch_get_results(h, idx, idx, db, db, idx, idx) == SIM3OPT_ERR_STATE);  // no solve yet
    CHECK(sim3opt_place_batch_get_pairs(h, 4, &np, idx) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_place_batch_get_pairs(h, 4, nullptr, idx) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_place_batch_get_bow(h, idx, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_place_batch_debug_scores(h, 0, db) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_place_batch_debug_scores(h, 0, nullptr) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_place_batch_debug_islands(h, 0, idx, idx, db, idx, idx, db) == SIM3OPT_ERR_STATE);
    const float bad_d[64] = {NAN};
    CHECK(sim3opt_place_batch_debug_words(h, 0, d.data(), idx, db) == SIM3OPT_ERR_ARG);   // n < 1
    CHECK(sim3opt_place_batch_debug_words(h, 1, nullptr, idx, db) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_place_batch_debug_words(h, 1, bad_d, idx, db) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_place_batch_debug_words(h, 1, d.data(), nullptr, nullptr) == SIM3OPT_ERR_ARG);
    CHECK(unchanged());
    sim3opt_place_batch_destroy(h);
    sim3opt_place_batch_destroy(nullptr);
    CHECK(std::string(sim3opt_place_batch_last_error(nullptr)) == "null batch");
  }
  std::printf("place_conformance host: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

int run_part(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
  int n_nodes = 0, n_frames = 0;
  if (std::fscanf(f, "%d %d", &n_nodes, &n_frames) != 2 || n_nodes < 2 || n_frames < 1) { std::fclose(f); return 2; }
  std::vector<int32_t> parent((size_t)n_nodes), word_id((size_t)n_nodes);
  std::vector<double> weight((size_t)n_nodes);
  std::vector<float> centre(64 * (size_t)n_nodes);
  bool ok = true;
  for (int i = 0; i < n_nodes && ok; ++i) {
    ok = std::fscanf(f, "%d %d %lf", &parent[(size_t)i], &word_id[(size_t)i], &weight[(size_t)i]) == 3;
    for (int k = 0; k < 64 && ok; ++k) ok = std::fscanf(f, "%f", &centre[64 * (size_t)i + k]) == 1;
  }
  const double K[9] = {718.856, 0, 607.1928, 0, 718.856, 185.2157, 0, 0, 1};
  sim3opt_shim::LoopDetectorBatch places;
  sim3opt_shim::LoopMatchBatch match(K, 1241, 376);
  match.options().knn_k = 1;  // every keypoint is an observation of its keyframe
  if (ok && places.set_vocabulary(n_nodes, parent.data(), centre.data(), weight.data(), word_id.data()) != SIM3OPT_OK) {
    std::fprintf(stderr, "set_vocabulary: %s\n", places.last_error().c_str());
    std::fclose(f);
    return 2;
  }
  for (int i = 0; i < n_frames && ok; ++i) {
    int count = 0;
    ok = std::fscanf(f, "%d", &count) == 1 && count >= 0;
    std::vector<P2> keys((size_t)(ok ? count : 0));
    std::vector<float> z(keys.size()), d(64 * keys.size());
    for (size_t r = 0; r < keys.size() && ok; ++r) {
      ok = std::fscanf(f, "%f %f %f", &keys[r].x, &keys[r].y, &z[r]) == 3;
      for (int k = 0; k < 64 && ok; ++k) ok = std::fscanf(f, "%f", &d[64 * r + k]) == 1;
    }
    if (!ok) break;
    ok = places.add_frame(d.data(), count) == i && match.add_frame(keys, d.data(), keys, z) == i;
  }
  std::vector<int> status((size_t)n_frames), expect_match((size_t)n_frames);
  for (int i = 0; i < n_frames && ok; ++i) ok = std::fscanf(f, "%d %d", &status[(size_t)i], &expect_match[(size_t)i]) == 2;
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "malformed file %s (%s)\n", path, places.last_error().c_str()); return 2; }
  const int rc = places.detect();  // after the loop: every keyframe
  if (rc < 0) {
    std::fprintf(stderr, "detect failed (%d): %s\n", rc, places.last_error().c_str());
    return 3;
  }
  int expected = 0;
  for (int i = 0; i < n_frames; ++i) {
    const sim3opt_shim::LoopDetectorBatch::DetectionResult r = places.result(i);
    CHECK(r.query == i && r.status == status[(size_t)i] && r.match == expect_match[(size_t)i]);
    CHECK(r.detection() == (status[(size_t)i] == SIM3OPT_PLACE_CANDIDATE));
    if (r.detection()) {
      CHECK(places.candidate_query(expected) == i && places.candidate_match(expected) == r.match);
      CHECK(r.n_consistent > places.options().k && r.island_first <= r.match && r.match <= r.island_last && r.score > 0);
      ++expected;
    }
  }
  CHECK(rc == expected && places.n_candidates() == expected);
  const std::vector<int> id = places.feed(match);  // the candidates are the matching stage's pairs
  CHECK((int)id.size() == expected && match.n_pairs() == expected);
  const int rm = match.solve();
  if (rm < 0) {
    std::fprintf(stderr, "match failed (%d): %s\n", rm, match.last_error().c_str());
    return 3;
  }
  CHECK(rm == expected);
  for (int c = 0; c < expected; ++c) {
    CHECK(id[(size_t)c] == c && match.status(c) == SIM3OPT_MATCH_OK);
    std::printf("candidate %d: keyframes %d and %d, %d matches\n", c, places.candidate_query(c), places.candidate_match(c),
                match.n_matches(c));
    CHECK(match.n_matches(c) >= 12);
  }
  std::printf("place_conformance run: %d candidates, %d checks, %d failed\n", expected, g_checks, g_failed);
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
