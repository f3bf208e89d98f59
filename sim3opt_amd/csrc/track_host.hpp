// track_host.hpp -- the host side of the loop-track stage (track_batch.hip; include/sim3opt.h, "batched loop tracks"):
// the checks of the arrays a caller hands over, the global observation indices of the matches, and a serial
// restatement of the whole definition -- union-find over the kept matches, then track_math.hpp -- which
// sim3opt_track_reference returns and the device is held to byte for byte.  Plain C++ with no HIP in it, so
// tests/cxx/track_host_driver.cpp runs it under the host sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "handle_host.hpp"
#include "track_math.hpp"

namespace sim3opt_track {

// kp_ptr / kp as every stage takes them; a frame may own nothing
inline std::string validate_frames(int32_t n_frames, const int32_t* kp_ptr, const float* kp) {
  if (n_frames < 1) return "n_frames < 1";
  if (!kp_ptr || !kp) return "a NULL array";
  const std::string e = sim3opt::check_frame_ptr("kp_ptr", n_frames, kp_ptr);
  if (!e.empty()) return e;
  if (!sim3opt::all_finite(kp, 2 * (size_t)kp_ptr[n_frames])) return "a non-finite keypoint";
  return "";
}

// The matches of all pairs against the frames' kp_ptr.  On success ga / gb hold the global observation indices of the
// two sides of every match, ga = -1 where the mask drops the match.
inline std::string validate_matches(int32_t n_frames, const int32_t* kp_ptr, int32_t n_pairs, const int32_t* pairs,
                                    const int32_t* match_ptr, const int32_t* query_idx, const int32_t* train_idx,
                                    const uint8_t* mask, std::vector<int32_t>& ga, std::vector<int32_t>& gb) {
  if (n_pairs < 1) return "n_pairs < 1";
  if (!pairs || !match_ptr || !query_idx || !train_idx) return "a NULL array";
  std::string e = sim3opt::check_frame_ptr("match_ptr", n_pairs, match_ptr);
  if (!e.empty()) return e.find("frame") == std::string::npos ? e : e.replace(e.find("frame"), 5, "pair");
  const size_t total = (size_t)match_ptr[n_pairs];
  if (total >= ((size_t)1 << 30)) return "too many matches";
  for (int32_t p = 0; p < n_pairs; ++p)
    for (int k = 0; k < 2; ++k)
      if (pairs[2 * p + k] < 0 || pairs[2 * p + k] >= n_frames) return "pair " + std::to_string(p) + ": no such frame";
  ga.assign(total, -1);
  gb.assign(total, -1);
  for (int32_t p = 0; p < n_pairs; ++p) {
    const int32_t f0 = pairs[2 * p], f1 = pairs[2 * p + 1];
    const int32_t n0 = kp_ptr[f0 + 1] - kp_ptr[f0], n1 = kp_ptr[f1 + 1] - kp_ptr[f1];
    for (int32_t m = match_ptr[p]; m < match_ptr[p + 1]; ++m) {
      if (query_idx[m] < 0 || query_idx[m] >= n0 || train_idx[m] < 0 || train_idx[m] >= n1)
        return "match " + std::to_string(m) + " of pair " + std::to_string(p) + ": an index outside its frame";
      gb[m] = kp_ptr[f1] + train_idx[m];
      if (!mask || mask[m]) ga[m] = kp_ptr[f0] + query_idx[m];
    }
  }
  return "";
}

inline std::string validate_cameras(int32_t n_frames, int32_t have_frames, const double* states, double focal, double cx,
                                    double cy) {
  if (!states) return "a NULL array";
  if (n_frames != have_frames)
    return "states are of " + std::to_string(n_frames) + " frames, the handle holds " + std::to_string(have_frames);
  if (!sim3opt::all_finite(states, 8 * (size_t)n_frames)) return "a non-finite state";
  for (int32_t f = 0; f < n_frames; ++f)
    if (!(states[8 * (size_t)f + 7] > 0.0)) return "frame " + std::to_string(f) + ": s <= 0";
  const double k[3] = {focal, cx, cy};
  if (!sim3opt::all_finite(k, 3)) return "non-finite intrinsics";
  if (!(focal > 0.0)) return "focal <= 0";
  return "";
}

// per g: 2 * match + side of the lowest kept match that has g on a side with a depth present (side 0 before side 1)
inline void depth_keys(size_t N, const std::vector<int32_t>& ga, const std::vector<int32_t>& gb, const double* depth0,
                       const double* depth1, std::vector<int32_t>& dkey) {
  dkey.assign(std::max<size_t>(N, 1), NONE);
  for (size_t m = 0; m < ga.size(); ++m) {
    if (ga[m] < 0) continue;
    if (depth0 && depth_present(depth0[m]) && dkey[ga[m]] == NONE) dkey[ga[m]] = (int32_t)(2 * m);
    if (depth1 && depth_present(depth1[m]) && dkey[gb[m]] == NONE) dkey[gb[m]] = (int32_t)(2 * m + 1);
  }
}

struct Tracks {  // what a solve returns
  std::vector<int32_t> track_ptr, obs_g, status, first_match, match_track, n_depths;
  std::vector<double> points;
  int32_t n_tracks() const { return (int32_t)status.size(); }
};

// The definition, serially: the connected components of the kept matches by union-find, numbered by their smallest
// kept match, their observations ascending in g; then the point and the status of each through track_math.hpp.
inline void reference_tracks(int32_t n_frames, const int32_t* kp_ptr, const float* kp, const std::vector<int32_t>& ga,
                             const std::vector<int32_t>& gb, const double* depth0, const double* depth1,
                             const double* states, double focal, double cx, double cy, double max_reproj_px, Tracks& out) {
  const size_t N = (size_t)kp_ptr[n_frames], M = ga.size();
  std::vector<int32_t> parent(std::max<size_t>(N, 1));
  for (size_t g = 0; g < parent.size(); ++g) parent[g] = (int32_t)g;
  auto find = [&](int32_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
  };
  for (size_t m = 0; m < M; ++m) {
    if (ga[m] < 0) continue;
    const int32_t a = find(ga[m]), b = find(gb[m]);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
  }
  std::vector<int32_t> track_of(parent.size(), -1);  // by root
  out = Tracks{};
  out.match_track.assign(M, -1);
  for (size_t m = 0; m < M; ++m) {
    if (ga[m] < 0) continue;
    const int32_t r = find(ga[m]);
    if (track_of[r] < 0) {
      track_of[r] = out.n_tracks();
      out.status.push_back(0);
      out.first_match.push_back((int32_t)m);
    }
    out.match_track[m] = track_of[r];
  }
  const int32_t T = out.n_tracks();
  out.track_ptr.assign((size_t)T + 1, 0);
  for (size_t g = 0; g < N; ++g) {
    const int32_t t = track_of[find((int32_t)g)];
    if (t >= 0) ++out.track_ptr[(size_t)t + 1];
  }
  for (int32_t t = 0; t < T; ++t) out.track_ptr[(size_t)t + 1] += out.track_ptr[t];
  out.obs_g.assign((size_t)out.track_ptr[T], 0);
  std::vector<int32_t> cursor(out.track_ptr.begin(), out.track_ptr.end() - 1);
  for (size_t g = 0; g < N; ++g) {  // ascending g: every segment comes out ordered
    const int32_t t = track_of[find((int32_t)g)];
    if (t >= 0) out.obs_g[(size_t)cursor[t]++] = (int32_t)g;
  }
  std::vector<int32_t> dkey;
  depth_keys(N, ga, gb, depth0, depth1, dkey);
  const PointArgs A{kp_ptr, n_frames, kp, dkey.data(), depth0, depth1, states, focal, cx, cy, max_reproj_px};
  out.points.assign(3 * (size_t)T, 0.0);
  out.n_depths.assign((size_t)T, 0);
  for (int32_t t = 0; t < T; ++t)
    out.status[t] = track_point(A, out.obs_g.data() + out.track_ptr[t], out.track_ptr[(size_t)t + 1] - out.track_ptr[t],
                                out.points.data() + 3 * (size_t)t, out.n_depths[t]);
}

// (frame, keypoint) of the observations g[0 .. n)
inline void split_observations(int32_t n_frames, const int32_t* kp_ptr, const int32_t* g, size_t n, int32_t* frame,
                               int32_t* keypoint) {
  for (size_t i = 0; i < n; ++i) {
    const int32_t f = frame_of(kp_ptr, n_frames, g[i]);
    if (frame) frame[i] = f;
    if (keypoint) keypoint[i] = g[i] - kp_ptr[f];
  }
}

}  // namespace sim3opt_track
