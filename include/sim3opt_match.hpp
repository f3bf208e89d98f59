// sim3opt_match.hpp -- header-only C++ helper for the front of the loop detector's computeConstraints, forwarding to
// the sim3opt_match_batch_* entry points of libsim3opt (include/sim3opt.h, "batched descriptor matching").
//
// The reference matches the descriptors of every loop candidate on its own, filters the matches
// (kittiDetector.h:1085-1160) and looks the depth of every kept match up in the map (:1229-1279), inside the loop of
// computeConstraints:
//
//     matcher.match(descriptors[0], descriptors[1], matches);                     // :1088
//     ... border, skew, uniqueness -> good_matches                                // :1092-1160
//     knn[cap]->train(trainData[cap], cv::ml::ROW_SAMPLE, responses[cap]);        // :1255
//     resp = knn[cap]->findNearest(sample, K, res, nearests);                     // :1268 -> surfPoints[cap]
//
// With this helper the call site hands every keyframe over once, names the candidates, and runs after the loop:
//
//     sim3opt_shim::LoopMatchBatch match(K_rowmajor, cols, rows);                 // before the loop
//     int f0 = match.add_frame(keys[0], descriptors[0].ptr<float>(), obsinc[0], depths_of_ptsinc0);
//     int f1 = match.add_frame(keys[1], descriptors[1].ptr<float>(), obsinc[1], depths_of_ptsinc1);
//     int id = match.add_pair(f0, f1);                                            // at :1088
//     ...
//     match.solve();                                                              // after the loop: every candidate
//     sim3opt_shim::PnpRansacBatch pnp;
//     std::vector<int> pnp_id = match.feed(pnp);                                  // point_count > 8 of :1282
//     pnp.solve();
//
// PARITY UNPINNED: the reference stores neither descriptors nor matches and its FlannBasedMatcher is approximate; here
// the search is exact and deterministic (include/sim3opt.h says what is the reference's).  add_frame() takes any point
// types with public x, y members (cv::KeyPoint::pt is one: pass a vector of those points, or of cv::Point2f) and the
// descriptors as one pointer to n rows of 64 floats (cv::Mat::ptr<float>() of a continuous CV_32F matrix).  No Eigen,
// no OpenCV.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"
#include "sim3opt_frames.hpp"
#include "sim3opt_pnp.hpp"

namespace sim3opt_shim {

class LoopMatchBatch {
 public:
  struct P3 { double x, y, z; };
  struct P2 { double x, y; };

  // K as 9 doubles row-major, the image size in pixels (cols, rows of :1101)
  LoopMatchBatch(const double* K, int image_width, int image_height)
      : b_(sim3opt_match_batch_create()), f_(K ? K[0] : 0), cx_(K ? K[2] : 0), cy_(K ? K[5] : 0), w_(image_width),
        h_(image_height) {
    sim3opt_match_batch_options_default(&opt_);
    for (int i = 0; i < 9; ++i) K_[i] = K ? K[i] : 0.0;
  }
  ~LoopMatchBatch() { sim3opt_match_batch_destroy(b_); }
  LoopMatchBatch(const LoopMatchBatch&) = delete;
  LoopMatchBatch& operator=(const LoopMatchBatch&) = delete;

  // thresh, boundaryRatio, skewThreshX / Y and K of the reference; read at solve()
  sim3opt_match_batch_options& options() { return opt_; }
  const std::string& last_error() const { return err_; }
  int n_frames() const { return (int)kp_ptr_.size() - 1; }
  int n_pairs() const { return (int)(pairs_.size() / 2); }

  // One keyframe: its keypoints, their descriptors (keys.size() rows of 64 floats), the map-point observations in its
  // image and the depth (z in the camera's frame) of each.  Returns its index, or -1 with nothing added.
  template <class PK, class PO, class D>
  int add_frame(const std::vector<PK>& keys, const float* descriptor_rows, const std::vector<PO>& obs,
                const std::vector<D>& depths) {
    if (!keys.empty() && !descriptor_rows) return fail("add_frame: NULL descriptors");
    if (obs.size() != depths.size()) return fail("add_frame: one depth per observation");
    for (std::size_t i = 0; i < keys.size(); ++i) {
      kp_.push_back((float)keys[i].x); kp_.push_back((float)keys[i].y);
    }
    if (!keys.empty()) desc_.insert(desc_.end(), descriptor_rows, descriptor_rows + 64 * keys.size());
    for (std::size_t i = 0; i < obs.size(); ++i) {
      obs_uv_.push_back((float)obs[i].x); obs_uv_.push_back((float)obs[i].y);
      obs_depth_.push_back((float)depths[i]);
    }
    kp_ptr_.push_back((int32_t)(kp_.size() / 2));
    obs_ptr_.push_back((int32_t)obs_depth_.size());
    solved_ = false;
    return n_frames() - 1;
  }

  // One candidate: frame0 is the query side (keys[0] of :1088).  Returns its index, or -1 with nothing added.
  int add_pair(int frame0, int frame1) {
    if (frame0 < 0 || frame1 < 0 || frame0 >= n_frames() || frame1 >= n_frames()) return fail("add_pair: no such frame");
    pairs_.push_back(frame0); pairs_.push_back(frame1);
    solved_ = false;
    return n_pairs() - 1;
  }

  // Every candidate added so far.  Candidates with status 0, or a negative SIM3OPT_ERR_*.
  int solve() {
    if (!b_) return fail("solve: out of memory", SIM3OPT_ERR_ARG);
    // (the C-ABI refuses NULL arrays; a batch without keypoints or observations still has arrays)
    const float none = 0.f;
    int rc = sim3opt_match_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK)
      rc = sim3opt_match_batch_set_frames(b_, n_frames(), kp_ptr_.data(), obs_ptr_.data(), kp_.empty() ? &none : kp_.data(),
                                          desc_.empty() ? &none : desc_.data(), obs_uv_.empty() ? &none : obs_uv_.data(),
                                          obs_depth_.empty() ? &none : obs_depth_.data(), f_, cx_, cy_, w_, h_);
    return finish(rc);
  }

  // The keypoints and descriptors of a FrameStore, read where they are on the device
  // (sim3opt_match_batch_set_frames_from); add_frame() gave every keyframe of the store, in order, its map observations
  // (and whatever keys: they are not looked at).  Returns as solve().
  int solve(FrameStore& store) {
    if (!b_) return fail("solve: out of memory", SIM3OPT_ERR_ARG);
    const float none = 0.f;
    int rc = sim3opt_match_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK)
      rc = sim3opt_match_batch_set_frames_from(b_, store.handle(), n_frames(), obs_ptr_.data(),
                                               obs_uv_.empty() ? &none : obs_uv_.data(),
                                               obs_depth_.empty() ? &none : obs_depth_.data(), f_, cx_, cy_, w_, h_);
    return finish(rc);
  }

 private:
  // the pairs, the solve and its results, once the frames are set (rc: what setting them returned)
  int finish(int rc) {
    if (rc == SIM3OPT_OK) rc = sim3opt_match_batch_set_pairs(b_, n_pairs(), pairs_.data());
    if (rc == SIM3OPT_OK) rc = sim3opt_match_batch_solve(b_);
    if (rc < 0) return fail(sim3opt_match_batch_last_error(b_), rc);
    const std::size_t n = (std::size_t)n_pairs();
    ptr_.assign(n + 1, 0); status_.assign(n, 0);
    (void)sim3opt_match_batch_get_match_ptr(b_, ptr_.data());
    (void)sim3opt_match_batch_get_summary(b_, status_.data(), nullptr, nullptr, nullptr, nullptr);
    const std::size_t m = (std::size_t)ptr_[n];
    query_.assign(m, 0); train_.assign(m, 0); dist_.assign(m, 0.f);
    uv0_.assign(2 * m, 0.0); uv1_.assign(2 * m, 0.0); z0_.assign(m, 0.0); z1_.assign(m, 0.0); pts_.assign(3 * m, 0.0);
    (void)sim3opt_match_batch_get_matches(b_, query_.data(), train_.data(), dist_.data(), uv0_.data(), uv1_.data(),
                                          z0_.data(), z1_.data(), pts_.data());
    solved_ = true;
    return rc;
  }

 public:
  // ---- results of candidate id, after solve() (before: status -1, no matches) ----
  int status(int id) const { return solved_ ? status_[id] : -1; }                         // SIM3OPT_MATCH_*
  int n_matches(int id) const { return solved_ ? ptr_[id + 1] - ptr_[id] : 0; }           // good_matches.size()
  int query_idx(int id, int i) const { return query_[at(id, i)]; }                        // good_matches[i].queryIdx
  int train_idx(int id, int i) const { return train_[at(id, i)]; }                        // .trainIdx
  float distance(int id, int i) const { return dist_[at(id, i)]; }                        // .distance
  P2 point1(int id, int i) const { return P2{uv0_[2 * at(id, i)], uv0_[2 * at(id, i) + 1]}; }   // points1[i], :1286
  P2 point2(int id, int i) const { return P2{uv1_[2 * at(id, i)], uv1_[2 * at(id, i) + 1]}; }   // points2[i]
  double depth(int id, int side, int i) const { return (side ? z1_ : z0_)[at(id, i)]; }   // depths[side][i], :1305
  P3 surf_point(int id, int i) const {                                                    // surfPoints[0][i], :1275
    const double* p = &pts_[3 * at(id, i)];
    return P3{p[0], p[1], p[2]};
  }
  // sloop of :1305-1311 for one candidate with at least one match (0 otherwise)
  double depth_ratio(int id) const {
    if (n_matches(id) < 1) return 0.0;
    const int32_t ptr[2] = {0, n_matches(id)};
    double r = 0.0;
    (void)sim3opt_median_depth_ratio(1, ptr, &z0_[at(id, 0)], &z1_[at(id, 0)], &r);
    return r;
  }

  // Hands every candidate with status 0 and more than min_matches matches (point_count > 8, :1282) to the PnP helper,
  // as the call at :1300 does.  Returns, per candidate of this batch, its index in `pnp` or -1.
  std::vector<int> feed(PnpRansacBatch& pnp, int min_matches = 8) const {
    std::vector<int> id((std::size_t)n_pairs(), -1);
    std::vector<P3> xyz;
    std::vector<P2> uv;
    for (int k = 0; k < n_pairs(); ++k) {
      if (status(k) != SIM3OPT_MATCH_OK || n_matches(k) <= min_matches) continue;
      xyz.clear(); uv.clear();
      for (int i = 0; i < n_matches(k); ++i) { xyz.push_back(surf_point(k, i)); uv.push_back(point2(k, i)); }
      id[(std::size_t)k] = pnp.add(xyz, uv, K_);
    }
    return id;
  }

 private:
  int fail(const std::string& why, int rc = -1) { err_ = why; return rc; }
  std::size_t at(int id, int i) const { return (std::size_t)ptr_[id] + (std::size_t)i; }

  sim3opt_match_batch* b_;
  sim3opt_match_batch_options opt_;
  std::string err_;
  double f_, cx_, cy_, K_[9];
  int w_, h_;
  std::vector<int32_t> kp_ptr_ = std::vector<int32_t>(1, 0), obs_ptr_ = std::vector<int32_t>(1, 0), pairs_;
  std::vector<float> kp_, desc_, obs_uv_, obs_depth_, dist_;
  std::vector<int32_t> ptr_, status_, query_, train_;
  std::vector<double> uv0_, uv1_, z0_, z1_, pts_;
  bool solved_ = false;
};

}  // namespace sim3opt_shim
