// place_host.hpp -- the host half of the batched bag-of-words place recognition (place_batch.hip): the tile sizes, the
// checks of the options, the vocabulary tree and the frames a caller hands over, the tree in the order the kernels
// read it, and the temporal-consistency recurrence over the queries.  Plain C++ with no HIP in it, so
// tests/cxx/place_host_driver.cpp runs it under the host sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "handle_host.hpp"

namespace sim3opt_place {

constexpr int WAVE = 64;           // lanes of a wavefront: the vector entries k_place_score looks up at a time
constexpr int WG = 256;            // lanes of every workgroup: descriptors of k_place_words, scan width of k_place_bow
constexpr int BOW_CHUNK = 1024;    // words of a frame staged in LDS at a time by k_place_bow (4 KB)
constexpr int SCORE_LDS = 2048;    // words of a query's vector k_place_score keeps in LDS (8 KB); longer ones stay global
constexpr int SCORE_JB = 64;       // database frames of a workgroup of k_place_score: sixteen per wavefront
constexpr int LDS_NODES = 128;     // nodes from the top of the tree whose centres k_place_words stages in LDS (32 KB)
constexpr int DESC = 64;           // floats of a SURF-64 descriptor
constexpr int MAX_CHILDREN = 64;   // children of one node
constexpr int MAX_RESULTS = 1024;  // options.max_db_results' upper limit: the kept results live in LDS

using sim3opt::all_finite;
using sim3opt::check_frame_ptr;

// The tree as the kernels read it: nodes renumbered breadth first, children in ascending original index, so the
// children of a node are consecutive and the top levels are the first nodes.
struct Vocabulary {
  int32_t n_nodes = 0, n_words = 0, depth = 0;   // depth: edges from the root to the deepest leaf
  std::vector<int32_t> first_child, n_child;     // per node; a leaf has n_child 0
  std::vector<int32_t> node_word;                // per node: the word id, -1 at inner nodes
  std::vector<int32_t> node_id;                  // per node: its index in the caller's arrays
  std::vector<float> centre;                     // per node x DESC
  std::vector<double> word_weight;               // per word id
};

inline std::string validate_options(const sim3opt_place_batch_options& o) {
  if (!std::isfinite(o.alpha) || o.alpha < 0) return "alpha is negative or not finite";
  if (!std::isfinite(o.min_nss_factor) || o.min_nss_factor < 0) return "min_nss_factor is negative or not finite";
  if (o.use_nss != 0 && o.use_nss != 1) return "use_nss is neither 0 nor 1";
  if (o.accumulate != 0 && o.accumulate != 1) return "accumulate is neither 0 nor 1";
  if (o.k < 0) return "k < 0";
  if (o.dislocal < 1) return "dislocal < 1";
  if (o.max_db_results < 1 || o.max_db_results > MAX_RESULTS)
    return "max_db_results outside 1.." + std::to_string(MAX_RESULTS);
  if (o.max_intragroup_gap < 1) return "max_intragroup_gap < 1";
  if (o.min_matches_per_group < 1) return "min_matches_per_group < 1";
  if (o.max_distance_between_queries < 0) return "max_distance_between_queries < 0";
  if (o.max_distance_between_groups < 0) return "max_distance_between_groups < 0";
  return "";
}

// "" and the tree in V, or what is wrong with the arrays (V is then as it was)
inline std::string build_vocabulary(int32_t n_nodes, const int32_t* parent, const float* centre, const double* weight,
                                    const int32_t* word_id, Vocabulary& V) {
  if (!parent || !centre || !weight || !word_id) return "a NULL array";
  if (n_nodes < 2) return "n_nodes < 2";
  if (n_nodes > INT32_MAX / DESC) return "too many nodes";
  const size_t N = (size_t)n_nodes;
  if (parent[0] != -1) return "node 0 is not the root (parent[0] must be -1)";
  std::vector<int32_t> nc(N, 0);
  for (int32_t i = 1; i < n_nodes; ++i) {
    if (parent[i] < 0 || parent[i] >= i)
      return "node " + std::to_string(i) + ": parent " + std::to_string(parent[i]) + " is not a smaller node";
    if (++nc[(size_t)parent[i]] > MAX_CHILDREN)
      return "node " + std::to_string(parent[i]) + " has more than " + std::to_string(MAX_CHILDREN) + " children";
  }
  int32_t n_words = 0;
  for (int32_t i = 0; i < n_nodes; ++i) {
    if (!all_finite(centre + (size_t)DESC * i, DESC)) return "node " + std::to_string(i) + ": a non-finite centre";
    if (nc[(size_t)i] == 0) {
      if (!std::isfinite(weight[i]) || weight[i] < 0)
        return "leaf " + std::to_string(i) + ": a negative or non-finite weight";
      if (word_id[i] < 0) return "leaf " + std::to_string(i) + " has no word id";
      ++n_words;
    } else if (word_id[i] != -1) {
      return "inner node " + std::to_string(i) + " has a word id";
    }
  }
  std::vector<double> ww((size_t)n_words, -1.0);
  for (int32_t i = 0; i < n_nodes; ++i) {
    if (nc[(size_t)i]) continue;
    if (word_id[i] >= n_words)
      return "leaf " + std::to_string(i) + ": word id " + std::to_string(word_id[i]) + " is not below the number of leaves";
    if (ww[(size_t)word_id[i]] >= 0) return "leaf " + std::to_string(i) + ": word id " + std::to_string(word_id[i]) + " is repeated";
    ww[(size_t)word_id[i]] = weight[i];
  }
  // children by parent, in ascending index (a counting sort keeps the order), then the breadth-first numbering
  std::vector<int32_t> cptr(N + 1, 0), child(N - 1), fill(N, 0);
  for (size_t i = 0; i < N; ++i) cptr[i + 1] = cptr[i] + nc[i];
  for (int32_t i = 1; i < n_nodes; ++i) child[(size_t)(cptr[(size_t)parent[i]] + fill[(size_t)parent[i]]++)] = i;
  Vocabulary W;
  W.n_nodes = n_nodes; W.n_words = n_words;
  W.node_id.assign(1, 0);
  W.node_id.reserve(N);
  std::vector<int32_t> level(1, 0);
  level.reserve(N);
  W.first_child.assign(N, 0); W.n_child.assign(N, 0); W.node_word.assign(N, -1);
  for (size_t b = 0; b < W.node_id.size(); ++b) {  // (every node hangs below the root: the queue reaches all N)
    const int32_t i = W.node_id[b];
    W.first_child[b] = (int32_t)W.node_id.size();
    W.n_child[b] = nc[(size_t)i];
    W.node_word[b] = word_id[i];
    if (nc[(size_t)i] == 0 && level[b] > W.depth) W.depth = level[b];
    for (int32_t c = cptr[(size_t)i]; c < cptr[(size_t)i + 1]; ++c) {
      W.node_id.push_back(child[(size_t)c]);
      level.push_back(level[b] + 1);
    }
  }
  W.centre.resize(N * DESC);
  for (size_t b = 0; b < N; ++b)
    for (int k = 0; k < DESC; ++k) W.centre[b * DESC + k] = centre[(size_t)W.node_id[b] * DESC + k];
  W.word_weight.swap(ww);
  V = std::move(W);
  return "";
}

inline std::string validate_frames(int32_t n_frames, const int32_t* kp_ptr, const float* desc) {
  if (n_frames < 1) return "n_frames < 1";
  if (n_frames > SIM3OPT_PLACE_MAX_FRAMES) return "n_frames above SIM3OPT_PLACE_MAX_FRAMES";
  if (!kp_ptr || !desc) return "a NULL array";
  const std::string e = check_frame_ptr("kp_ptr", n_frames, kp_ptr);
  if (!e.empty()) return e;
  const size_t nk = (size_t)kp_ptr[n_frames];
  if (nk > (size_t)INT32_MAX / DESC) return "too many keypoints";
  if (!all_finite(desc, (size_t)DESC * nk)) return "a non-finite descriptor";
  return "";
}

// Step 6 of the definition.  status[i] == SIM3OPT_PLACE_CANDIDATE on entry marks the queries that reached step 5 with
// an island [first[i], last[i]]; on return those are SIM3OPT_PLACE_CANDIDATE or SIM3OPT_PLACE_NO_TEMPORAL_CONSISTENCY
// and n_consistent[i] is the recurrence's n after query i (0 for every other query).
inline void temporal_consistency(int32_t n_frames, const int32_t* first, const int32_t* last,
                                 const sim3opt_place_batch_options& o, int32_t* status, int32_t* n_consistent) {
  int32_t a1 = 0, a2 = 0, last_query = 0, n = 0;
  for (int32_t i = 0; i < n_frames; ++i) {
    n_consistent[i] = 0;
    if (status[i] != SIM3OPT_PLACE_CANDIDATE) continue;
    if (n == 0 || i - last_query > o.max_distance_between_queries) {
      n = 1;
    } else {
      const bool intersect = first[i] <= a2 && a1 <= last[i];
      const int32_t d1 = a1 - last[i], d2 = first[i] - a2;
      const bool fits = intersect || (d1 > d2 ? d1 : d2) <= o.max_distance_between_groups;
      n = fits ? n + 1 : 1;
    }
    a1 = first[i]; a2 = last[i]; last_query = i;
    n_consistent[i] = n;
    if (!(n > o.k)) status[i] = SIM3OPT_PLACE_NO_TEMPORAL_CONSISTENCY;
  }
}

}  // namespace sim3opt_place
