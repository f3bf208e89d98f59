// place_host_driver.cpp -- the host half of the batched place recognition (csrc/place_host.hpp: the checks of the
// options, of the vocabulary tree with every message as an exact string, of the frames, the breadth-first renumbering
// and the temporal-consistency recurrence) as a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer:
// no GPU and no HIP.  The arrays are sized exactly, so that a read past an end is the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../sim3opt_amd/csrc/place_host.hpp"

using namespace sim3opt_place;

static int failed = 0, checks = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    ++checks;                                                         \
    if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } \
  } while (0)

struct Tree {  // heap arrays of exactly n entries
  int32_t n;
  std::unique_ptr<int32_t[]> parent, word_id;
  std::unique_ptr<float[]> centre;
  std::unique_ptr<double[]> weight;
  Tree(std::vector<int32_t> p, std::vector<int32_t> w)
      : n((int32_t)p.size()), parent(new int32_t[p.size()]), word_id(new int32_t[p.size()]),
        centre(new float[DESC * p.size()]()), weight(new double[p.size()]) {
    for (int32_t i = 0; i < n; ++i) {
      parent[i] = p[(size_t)i]; word_id[i] = w[(size_t)i]; weight[i] = 1.0 + i;
      for (int k = 0; k < DESC; ++k) centre[(size_t)DESC * i + k] = (float)(100 * i + k);
    }
  }
  std::string build(Vocabulary& V) const {
    return build_vocabulary(n, parent.get(), centre.get(), weight.get(), word_id.get(), V);
  }
};

// the recurrence over queries of which reach[i] says whether query i reached step 5 with the island [first[i], last[i]]
// (the others carry SIM3OPT_PLACE_NO_DB_RESULTS); returns n_consistent
static std::vector<int32_t> run_window(const sim3opt_place_batch_options& o, const std::vector<int32_t>& reach,
                                       const std::vector<int32_t>& first, const std::vector<int32_t>& last,
                                       std::vector<int32_t>& status) {
  const size_t n = reach.size();
  status.assign(n, 0);
  for (size_t i = 0; i < n; ++i) status[i] = reach[i] ? SIM3OPT_PLACE_CANDIDATE : SIM3OPT_PLACE_NO_DB_RESULTS;
  std::vector<int32_t> cnt(n, -1);
  temporal_consistency((int32_t)n, first.data(), last.data(), o, status.data(), cnt.data());
  return cnt;
}

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // ---- options
  sim3opt_place_batch_options o{0.3, 0.005, 1, 3, 20, 50, 3, 1, 2, 3, 1, -1};
  CHECK(validate_options(o).empty());
  { auto p = o; p.alpha = -1e-300; CHECK(validate_options(p) == "alpha is negative or not finite"); }
  { auto p = o; p.alpha = nan; CHECK(validate_options(p) == "alpha is negative or not finite"); }
  { auto p = o; p.min_nss_factor = inf; CHECK(validate_options(p) == "min_nss_factor is negative or not finite"); }
  { auto p = o; p.use_nss = 2; CHECK(validate_options(p) == "use_nss is neither 0 nor 1"); }
  { auto p = o; p.accumulate = -1; CHECK(validate_options(p) == "accumulate is neither 0 nor 1"); }
  { auto p = o; p.k = -1; CHECK(validate_options(p) == "k < 0"); }
  { auto p = o; p.k = 0; CHECK(validate_options(p).empty()); }
  { auto p = o; p.dislocal = 0; CHECK(validate_options(p) == "dislocal < 1"); }
  { auto p = o; p.max_db_results = 0; CHECK(validate_options(p) == "max_db_results outside 1..1024"); }
  { auto p = o; p.max_db_results = MAX_RESULTS + 1; CHECK(validate_options(p) == "max_db_results outside 1..1024"); }
  { auto p = o; p.max_db_results = MAX_RESULTS; CHECK(validate_options(p).empty()); }
  { auto p = o; p.max_intragroup_gap = 0; CHECK(validate_options(p) == "max_intragroup_gap < 1"); }
  { auto p = o; p.min_matches_per_group = 0; CHECK(validate_options(p) == "min_matches_per_group < 1"); }
  { auto p = o; p.max_distance_between_queries = -1; CHECK(validate_options(p) == "max_distance_between_queries < 0"); }
  { auto p = o; p.max_distance_between_groups = -1; CHECK(validate_options(p) == "max_distance_between_groups < 0"); }
  // ---- the vocabulary: the root, inner nodes 1 and 4 (created depth first: 4 hangs below 1), five leaves
  // 0 -> 1, 2, 3 (2 and 3 are leaves: words 4, 0);  1 -> 4, 5 (5 is a leaf: word 2);  4 -> 6, 7 (leaves: words 1, 3)
  const std::vector<int32_t> par{-1, 0, 0, 0, 1, 1, 4, 4}, wid{-1, -1, 4, 0, -1, 2, 1, 3};
  {
    Tree T(par, wid);
    Vocabulary V;
    CHECK(T.build(V).empty());
    CHECK(V.n_nodes == 8 && V.n_words == 5 && V.depth == 3);
    const int32_t order[8] = {0, 1, 2, 3, 4, 5, 6, 7};  // (this tree's numbering is breadth first already)
    for (int b = 0; b < 8; ++b) CHECK(V.node_id[(size_t)b] == order[b]);
    const int32_t fc[8] = {1, 4, 0, 0, 6, 0, 0, 0}, nc[8] = {3, 2, 0, 0, 2, 0, 0, 0};
    for (int b = 0; b < 8; ++b) {
      CHECK(V.n_child[(size_t)b] == nc[b]);
      if (nc[b]) CHECK(V.first_child[(size_t)b] == fc[b]);
      CHECK(V.node_word[(size_t)b] == wid[(size_t)b]);
      CHECK(V.centre[(size_t)b * DESC + DESC - 1] == (float)(100 * b + DESC - 1));
    }
    const double ww[5] = {4.0, 7.0, 6.0, 8.0, 3.0};  // weight of node i is 1 + i
    for (int w = 0; w < 5; ++w) CHECK(V.word_weight[(size_t)w] == ww[w]);
  }
  {  // the numbering DBoW2 produces (a node's children, then each child's subtree) is not breadth first
    //  0 -> 1, 2;  1 -> 3, 4;  3 -> 5, 6;  2 -> 7, 8
    Tree T({-1, 0, 0, 1, 1, 3, 3, 2, 2}, {-1, -1, -1, -1, 0, 1, 2, 3, 4});
    Vocabulary V;
    CHECK(T.build(V).empty());
    const int32_t order[9] = {0, 1, 2, 3, 4, 7, 8, 5, 6};
    for (int b = 0; b < 9; ++b) CHECK(V.node_id[(size_t)b] == order[b]);
    CHECK(V.first_child[0] == 1 && V.first_child[1] == 3 && V.first_child[2] == 5 && V.first_child[3] == 7);
    CHECK(V.n_child[3] == 2 && V.n_child[4] == 0 && V.depth == 3);
    CHECK(V.node_word[5] == 3 && V.node_word[7] == 1);
    CHECK(V.centre[5 * DESC] == 700.f && V.centre[7 * DESC + 1] == 501.f);
  }
  // every refusal, word for word; V stays as it was
  {
    Vocabulary V;
    { Tree T(par, wid); CHECK(T.build(V).empty()); }
    const auto refused = [&](const Tree& T, const char* why) {
      const std::string e = T.build(V);
      if (e != why) std::printf("got: %s\n", e.c_str());
      return e == why && V.n_nodes == 8 && V.n_words == 5 && V.node_id.size() == 8;
    };
    { Tree T(par, wid); CHECK(build_vocabulary(8, nullptr, T.centre.get(), T.weight.get(), T.word_id.get(), V) == "a NULL array"); }
    { Tree T(par, wid); CHECK(build_vocabulary(8, T.parent.get(), nullptr, T.weight.get(), T.word_id.get(), V) == "a NULL array"); }
    { Tree T(par, wid); CHECK(build_vocabulary(8, T.parent.get(), T.centre.get(), nullptr, T.word_id.get(), V) == "a NULL array"); }
    { Tree T(par, wid); CHECK(build_vocabulary(8, T.parent.get(), T.centre.get(), T.weight.get(), nullptr, V) == "a NULL array"); }
    { Tree T({-1}, {0}); CHECK(refused(T, "n_nodes < 2")); }
    { Tree T(par, wid); T.parent[0] = 0; CHECK(refused(T, "node 0 is not the root (parent[0] must be -1)")); }
    { Tree T(par, wid); T.parent[4] = 4; CHECK(refused(T, "node 4: parent 4 is not a smaller node")); }
    { Tree T(par, wid); T.parent[4] = 6; CHECK(refused(T, "node 4: parent 6 is not a smaller node")); }
    { Tree T(par, wid); T.parent[7] = -1; CHECK(refused(T, "node 7: parent -1 is not a smaller node")); }
    { Tree T(par, wid); T.centre[DESC * 8 - 1] = nan; CHECK(refused(T, "node 7: a non-finite centre")); }
    { Tree T(par, wid); T.centre[0] = inf; CHECK(refused(T, "node 0: a non-finite centre")); }
    { Tree T(par, wid); T.weight[7] = -0.5; CHECK(refused(T, "leaf 7: a negative or non-finite weight")); }
    { Tree T(par, wid); T.weight[2] = (double)nan; CHECK(refused(T, "leaf 2: a negative or non-finite weight")); }
    { Tree T(par, wid); T.weight[1] = -1.0; T.weight[0] = (double)nan; Vocabulary W; CHECK(T.build(W).empty()); }  // read at leaves only
    { Tree T(par, wid); T.weight[7] = 0.0; Vocabulary W; CHECK(T.build(W).empty() && W.word_weight[3] == 0.0); }
    { Tree T(par, wid); T.word_id[5] = -1; CHECK(refused(T, "leaf 5 has no word id")); }
    { Tree T(par, wid); T.word_id[4] = 2; CHECK(refused(T, "inner node 4 has a word id")); }
    { Tree T(par, wid); T.word_id[0] = 0; CHECK(refused(T, "inner node 0 has a word id")); }
    { Tree T(par, wid); T.word_id[7] = 1; CHECK(refused(T, "leaf 7: word id 1 is repeated")); }
    { Tree T(par, wid); T.word_id[7] = 5; CHECK(refused(T, "leaf 7: word id 5 is not below the number of leaves")); }
    // 64 children are a tree, 65 are not
    for (int kids : {MAX_CHILDREN, MAX_CHILDREN + 1}) {
      std::vector<int32_t> p((size_t)kids + 1, 0), w((size_t)kids + 1);
      p[0] = -1; w[0] = -1;
      for (int i = 1; i <= kids; ++i) w[(size_t)i] = kids - i;
      Tree T(p, w);
      if (kids == MAX_CHILDREN) {
        Vocabulary W;
        CHECK(T.build(W).empty() && W.n_child[0] == MAX_CHILDREN && W.depth == 1 && W.node_word[1] == kids - 1);
      } else {
        CHECK(refused(T, "node 0 has more than 64 children"));
      }
    }
  }
  // ---- frames
  {
    const std::vector<int32_t> ptr{0, 3, 3, 5};
    std::unique_ptr<float[]> d(new float[DESC * 5 + 1]());
    CHECK(validate_frames(3, ptr.data(), d.get()).empty());
    CHECK(validate_frames(0, ptr.data(), d.get()) == "n_frames < 1");
    CHECK(validate_frames(SIM3OPT_PLACE_MAX_FRAMES + 1, ptr.data(), d.get()) == "n_frames above SIM3OPT_PLACE_MAX_FRAMES");
    CHECK(validate_frames(3, nullptr, d.get()) == "a NULL array" && validate_frames(3, ptr.data(), nullptr) == "a NULL array");
    d[DESC * 5 - 1] = nan; CHECK(validate_frames(3, ptr.data(), d.get()) == "a non-finite descriptor"); d[DESC * 5 - 1] = 0;
    d[DESC * 5] = nan; CHECK(validate_frames(3, ptr.data(), d.get()).empty());  // one past the last is not the frames'
    const std::vector<int32_t> off{1, 3, 3, 5}, back{0, 3, 2, 5};
    CHECK(validate_frames(3, off.data(), d.get()) == "kp_ptr[0] must be 0");
    CHECK(validate_frames(3, back.data(), d.get()) == "kp_ptr is not monotone at frame 1");
    std::vector<int32_t> full((size_t)SIM3OPT_PLACE_MAX_FRAMES + 1, 0);
    CHECK(validate_frames(SIM3OPT_PLACE_MAX_FRAMES, full.data(), d.get()).empty());  // frames may be empty, all of them
  }
  // ---- the temporal window (k = 3: the fourth consistent query is a candidate)
  {
    std::vector<int32_t> st;
    // consecutive queries on overlapping islands
    std::vector<int32_t> c = run_window(o, {1, 1, 1, 1, 1}, {0, 1, 2, 3, 4}, {2, 3, 4, 5, 6}, st);
    CHECK((c == std::vector<int32_t>{1, 2, 3, 4, 5}));
    CHECK((st == std::vector<int32_t>{6, 6, 6, 0, 0}));
    // queries that did not reach step 5 are left alone and do not touch the window; a break of 2 queries is allowed
    c = run_window(o, {1, 0, 1, 1, 0, 0, 1}, {0, 9, 1, 2, 9, 9, 3}, {0, 9, 1, 2, 9, 9, 3}, st);
    CHECK((c == std::vector<int32_t>{1, 0, 2, 3, 0, 0, 1}));  // 6 - 3 = 3 > max_distance_between_queries
    CHECK(st[1] == SIM3OPT_PLACE_NO_DB_RESULTS && st[6] == SIM3OPT_PLACE_NO_TEMPORAL_CONSISTENCY);
    c = run_window(o, {1, 0, 1, 1, 0, 1}, {0, 9, 1, 2, 9, 3}, {0, 9, 1, 2, 9, 3}, st);
    CHECK((c == std::vector<int32_t>{1, 0, 2, 3, 0, 4}) && st[5] == SIM3OPT_PLACE_CANDIDATE);
    // islands exactly max_distance_between_groups apart fit, on either side; one more does not and restarts at 1
    c = run_window(o, {1, 1, 1, 1}, {10, 14, 9, 15}, {11, 16, 11, 15}, st);
    CHECK((c == std::vector<int32_t>{1, 2, 3, 1}));  // 14 - 11 = 3; 14 - 11 = 3 (before); 15 - 11 = 4
    c = run_window(o, {1, 1, 1}, {10, 3, 12}, {11, 6, 12}, st);
    CHECK((c == std::vector<int32_t>{1, 1, 1}));  // 10 - 6 = 4; 12 - 6 = 6: the window moved to [3, 6]
    c = run_window(o, {1, 1, 1}, {10, 3, 8}, {11, 6, 8}, st);
    CHECK((c == std::vector<int32_t>{1, 1, 2}));  // 8 - 6 = 2
    // an island inside the window's, and one that holds it
    c = run_window(o, {1, 1, 1}, {10, 12, 0}, {20, 13, 40}, st);
    CHECK((c == std::vector<int32_t>{1, 2, 3}));
    // k = 0: every query that reached step 5 is a candidate
    auto p = o; p.k = 0;
    c = run_window(p, {1, 0, 1}, {0, 0, 30}, {0, 0, 30}, st);
    CHECK((st == std::vector<int32_t>{0, SIM3OPT_PLACE_NO_DB_RESULTS, 0}) && (c == std::vector<int32_t>{1, 0, 1}));
    // no frames at all: nothing is read
    temporal_consistency(0, nullptr, nullptr, o, nullptr, nullptr);
  }
  std::printf("%d checks, %d failed\n", checks, failed);
  if (!failed) std::printf("place host ok\n");
  return failed ? 1 : 0;
}
