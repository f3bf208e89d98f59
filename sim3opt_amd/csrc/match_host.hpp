// match_host.hpp -- the host half of the batched descriptor matching (match_batch.hip): the tile sizes, the checks of
// what a caller hands over and the table that maps workgroups to (pair, query tile).  Plain C++ with no HIP in it, so
// tests/cxx/match_host_driver.cpp runs it under the host sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "handle_host.hpp"

namespace sim3opt_match {

constexpr int WAVE = 64;          // lanes of a wavefront
constexpr int QUERY_TILE = 256;   // queries of a workgroup of k_match_nn: one per lane, four wavefronts
constexpr int TRAIN_TILE = 128;   // train descriptors staged in LDS at a time (32 KB)
constexpr int OBS_CHUNK = 1024;   // observations staged in LDS at a time by k_match_depth (8 KB)
constexpr int DESC = 64;          // floats of a SURF-64 descriptor
constexpr int MAX_K = 16;         // options.knn_k's upper limit: the sorted list lives in registers

struct Tile {
  int32_t pair, q0;  // the queries q0 .. q0 + QUERY_TILE - 1 of the pair (k_match_depth: its matches)
};

// What a solve needs of the pairs before anything runs: the status of each, where its queries and its train
// keypoints start in the per-query and per-train-keypoint arrays (pairs that are not OK own none), and the tiles.
struct Plan {
  std::vector<int32_t> status, qptr, tptr;
  std::vector<Tile> tiles;
};

using sim3opt::all_finite;
using sim3opt::check_frame_ptr;

inline std::string validate_options(const sim3opt_match_batch_options& o) {
  const double v[4] = {o.ratio, o.border_ratio, o.skew_x, o.skew_y};
  for (double x : v)
    if (!std::isfinite(x) || x < 0) return "a threshold is negative or not finite";
  if (o.knn_k < 1 || o.knn_k > MAX_K) return "knn_k outside 1.." + std::to_string(MAX_K);
  return "";
}

inline std::string validate_frames(int32_t n_frames, const int32_t* kp_ptr, const int32_t* obs_ptr, const float* kp,
                                   const float* desc, const float* obs_uv, const float* obs_depth, double focal,
                                   double cx, double cy, int32_t image_width, int32_t image_height) {
  if (n_frames < 1) return "n_frames < 1";
  if (!kp_ptr || !obs_ptr || !kp || !desc || !obs_uv || !obs_depth) return "a NULL array";
  if (!(focal > 0) || !std::isfinite(focal) || !std::isfinite(cx) || !std::isfinite(cy))
    return "focal <= 0 or a non-finite intrinsic";
  if (image_width < 1 || image_height < 1) return "a non-positive image size";
  std::string e = check_frame_ptr("kp_ptr", n_frames, kp_ptr);
  if (e.empty()) e = check_frame_ptr("obs_ptr", n_frames, obs_ptr);
  if (!e.empty()) return e;
  const size_t nk = (size_t)kp_ptr[n_frames], no = (size_t)obs_ptr[n_frames];
  if (nk > (size_t)INT32_MAX / DESC) return "too many keypoints";
  if (!all_finite(kp, 2 * nk)) return "a non-finite keypoint";
  if (!all_finite(desc, (size_t)DESC * nk)) return "a non-finite descriptor";
  if (!all_finite(obs_uv, 2 * no)) return "a non-finite observation";
  if (!all_finite(obs_depth, no)) return "a non-finite depth";
  return "";
}

// what validate_frames asks of everything but kp_ptr / kp / desc, in its words (set_frames_from: those are the store's)
inline std::string validate_observations(int32_t n_frames, const int32_t* obs_ptr, const float* obs_uv,
                                         const float* obs_depth, double focal, double cx, double cy, int32_t image_width,
                                         int32_t image_height) {
  if (n_frames < 1) return "n_frames < 1";
  if (!obs_ptr || !obs_uv || !obs_depth) return "a NULL array";
  if (!(focal > 0) || !std::isfinite(focal) || !std::isfinite(cx) || !std::isfinite(cy))
    return "focal <= 0 or a non-finite intrinsic";
  if (image_width < 1 || image_height < 1) return "a non-positive image size";
  const std::string e = check_frame_ptr("obs_ptr", n_frames, obs_ptr);
  if (!e.empty()) return e;
  const size_t no = (size_t)obs_ptr[n_frames];
  if (!all_finite(obs_uv, 2 * no)) return "a non-finite observation";
  if (!all_finite(obs_depth, no)) return "a non-finite depth";
  return "";
}

inline std::string validate_pairs(int32_t n_frames, int32_t n_pairs, const int32_t* pairs) {
  if (n_pairs < 1) return "n_pairs < 1";
  if (!pairs) return "a NULL array";
  for (int32_t p = 0; p < 2 * n_pairs; ++p)
    if (pairs[p] < 0 || pairs[p] >= n_frames)
      return "pair " + std::to_string(p / 2) + ": frame index out of range";
  return "";
}

// "" and the plan, or why there is none (the per-query arrays are indexed with int32_t)
inline std::string build_plan(const int32_t* kp_ptr, const int32_t* obs_ptr, int32_t n_pairs, const int32_t* pairs,
                              Plan& P) {
  P.status.assign((size_t)n_pairs, SIM3OPT_MATCH_OK);
  P.qptr.assign((size_t)n_pairs + 1, 0);
  P.tptr.assign((size_t)n_pairs + 1, 0);
  P.tiles.clear();
  int64_t q = 0, t = 0;
  for (int32_t p = 0; p < n_pairs; ++p) {
    const int32_t f0 = pairs[2 * p], f1 = pairs[2 * p + 1];
    const int32_t nq = kp_ptr[f0 + 1] - kp_ptr[f0], nt = kp_ptr[f1 + 1] - kp_ptr[f1];
    if (nq == 0 || nt == 0)
      P.status[p] = SIM3OPT_MATCH_NO_KEYPOINTS;
    else if (obs_ptr[f0 + 1] == obs_ptr[f0] || obs_ptr[f1 + 1] == obs_ptr[f1])
      P.status[p] = SIM3OPT_MATCH_NO_MAP;
    if (P.status[p] == SIM3OPT_MATCH_OK) {
      for (int32_t q0 = 0; q0 < nq; q0 += QUERY_TILE) P.tiles.push_back(Tile{p, q0});
      q += nq;
      t += nt;
    }
    if (q > INT32_MAX || t > INT32_MAX || P.tiles.size() > (size_t)INT32_MAX)
      return "the pairs hold more than 2^31 - 1 queries or train keypoints";
    P.qptr[p + 1] = (int32_t)q;
    P.tptr[p + 1] = (int32_t)t;
  }
  return "";
}

}  // namespace sim3opt_match
