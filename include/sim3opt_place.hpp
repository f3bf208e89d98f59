// sim3opt_place.hpp -- header-only C++ helper for the loop detector's place recognition, forwarding to the
// sim3opt_place_batch_* entry points of libsim3opt (include/sim3opt.h, "batched bag-of-words place recognition").
//
// The reference asks DLoopDetector once per keyframe, in sequence, on the host:
//
//     DetectionResult result;
//     detector.detectLoop(keys, descriptors, result);                             // kittiDetector.h:1663
//     if (result.detection()) vDetectionResults.push_back(...result.query, result.match...);
//
// With this helper the call site hands every keyframe's descriptors over and asks once, after the loop:
//
//     sim3opt_shim::LoopDetectorBatch places;                                      // before the loop
//     places.set_vocabulary(n_nodes, parent, centre, weight, word_id);             // DBoW2's saved nodes and words
//     places.options().alpha = 0.3;                                                // :1549-1564
//     int id = places.add_frame(descriptors.ptr<float>(), descriptors.rows);       // at :1663
//     ...
//     places.detect();                                                             // after the loop: every keyframe
//     if (places.result(id).detection()) ... places.result(id).match ...
//     sim3opt_shim::LoopMatchBatch match(K, cols, rows);                           // the same keyframes, same order
//     ... match.add_frame(...) per keyframe ...
//     std::vector<int> pair_id = places.feed(match);                               // the candidates become its pairs
//     match.solve();                                                               // then EssentialBatch: the
//                                                                                  // inlier test at 12 is the caller's
//
// PARITY UNPINNED: the reference tree holds neither DLoopDetector nor DBoW2, no vocabulary and no detection results;
// include/sim3opt.h says what is the reference's and what is recalled from upstream.  DLoopDetector's geometric check
// is not here: it is what the stages the pairs go to compute.  Descriptors are rows of 64 floats (cv::Mat::ptr<float>()
// of a continuous CV_32F matrix).  No Eigen, no OpenCV, no DBoW2.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"
#include "sim3opt_frames.hpp"
#include "sim3opt_match.hpp"

namespace sim3opt_shim {

class LoopDetectorBatch {
 public:
  // what detectLoop() fills, for one keyframe
  struct DetectionResult {
    int status = -1;       // SIM3OPT_PLACE_*; -1 before detect()
    int query = -1;        // the keyframe's index
    int match = -1;        // the earlier keyframe it matches; -1 where the status reports none
    double score = 0.0;    // s(query, match)
    double ns_factor = 0.0;
    int n_consistent = 0;  // the temporal window's count
    int island_first = -1, island_last = -1;
    bool detection() const { return status == SIM3OPT_PLACE_CANDIDATE; }
  };

  LoopDetectorBatch() : b_(sim3opt_place_batch_create()) { sim3opt_place_batch_options_default(&opt_); }
  ~LoopDetectorBatch() { sim3opt_place_batch_destroy(b_); }
  LoopDetectorBatch(const LoopDetectorBatch&) = delete;
  LoopDetectorBatch& operator=(const LoopDetectorBatch&) = delete;

  // DLoopDetector's parameters; read at detect()
  sim3opt_place_batch_options& options() { return opt_; }
  const std::string& last_error() const { return err_; }
  int n_frames() const { return (int)kp_ptr_.size() - 1; }
  int n_candidates() const { return (int)(pairs_.size() / 2); }

  // The tree as DBoW2 saves it (include/sim3opt.h).  SIM3OPT_OK, or SIM3OPT_ERR_ARG with the library's reason in
  // last_error() and the vocabulary as it was.
  int set_vocabulary(int n_nodes, const int32_t* parent, const float* centre, const double* weight,
                     const int32_t* word_id) {
    if (!b_) return fail("set_vocabulary: out of memory", SIM3OPT_ERR_ARG);
    const int rc = sim3opt_place_batch_set_vocabulary(b_, n_nodes, parent, centre, weight, word_id);
    if (rc != SIM3OPT_OK) return fail(sim3opt_place_batch_last_error(b_), rc);
    detected_ = false;
    return rc;
  }

  // One keyframe: `count` descriptors, rows of 64 floats.  Returns its index, or -1 with nothing added.
  int add_frame(const float* descriptor_rows, int count) {
    if (count < 0 || (count > 0 && !descriptor_rows)) return fail("add_frame: NULL descriptors");
    if (count > 0) desc_.insert(desc_.end(), descriptor_rows, descriptor_rows + 64 * (std::size_t)count);
    kp_ptr_.push_back((int32_t)(desc_.size() / 64));
    detected_ = false;
    return n_frames() - 1;
  }

  // Every keyframe added so far.  The number of candidates, or a negative SIM3OPT_ERR_*.
  int detect() {
    if (!b_) return fail("detect: out of memory", SIM3OPT_ERR_ARG);
    const float none = 0.f;  // (the C-ABI refuses a NULL array; keyframes without descriptors still have one)
    int rc = sim3opt_place_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK)
      rc = sim3opt_place_batch_set_frames(b_, n_frames(), kp_ptr_.data(), desc_.empty() ? &none : desc_.data());
    return finish(rc);
  }

  // The keyframes of a FrameStore, read where they are on the device (sim3opt_place_batch_set_frames_from), in place of
  // those added with add_frame(): they are forgotten.  Returns as detect().
  int detect(FrameStore& store) {
    if (!b_) return fail("detect: out of memory", SIM3OPT_ERR_ARG);
    int rc = sim3opt_place_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK) rc = sim3opt_place_batch_set_frames_from(b_, store.handle());
    if (rc == SIM3OPT_OK) {
      kp_ptr_ = store.kp_ptr();
      desc_.clear();
      detected_ = false;
    }
    return finish(rc);
  }

  // the keyframe's result; before detect(), and for an index that is no keyframe, status -1
  DetectionResult result(int i) const {
    return detected_ && i >= 0 && i < (int)results_.size() ? results_[(std::size_t)i] : DetectionResult();
  }
  // candidate c (ascending query), after detect()
  int candidate_query(int c) const { return pairs_[2 * (std::size_t)c]; }
  int candidate_match(int c) const { return pairs_[2 * (std::size_t)c + 1]; }

  // Names every candidate as a pair (query, match) of `match`, which holds the same keyframes in the same order.
  // Returns, per candidate, its pair index in `match`, or -1.
  std::vector<int> feed(LoopMatchBatch& match) const {
    std::vector<int> id((std::size_t)(detected_ ? n_candidates() : 0), -1);
    for (std::size_t c = 0; c < id.size(); ++c) id[c] = match.add_pair(candidate_query((int)c), candidate_match((int)c));
    return id;
  }

 private:
  int fail(const std::string& why, int rc = -1) { err_ = why; return rc; }

  // the solve and its results, once the frames are set (rc: what setting them returned)
  int finish(int rc) {
    if (rc == SIM3OPT_OK) rc = sim3opt_place_batch_solve(b_);
    if (rc < 0) return fail(sim3opt_place_batch_last_error(b_), rc);
    const std::size_t n = (std::size_t)n_frames();
    std::vector<int32_t> status(n), match(n), consistent(n), island(2 * n);
    std::vector<double> score(n), ns(n);
    (void)sim3opt_place_batch_get_results(b_, status.data(), match.data(), score.data(), ns.data(), consistent.data(),
                                          island.data());
    results_.assign(n, DetectionResult());
    for (std::size_t i = 0; i < n; ++i) {
      DetectionResult& r = results_[i];
      r.status = status[i]; r.query = (int)i; r.match = match[i]; r.score = score[i]; r.ns_factor = ns[i];
      r.n_consistent = consistent[i]; r.island_first = island[2 * i]; r.island_last = island[2 * i + 1];
    }
    int32_t np = 0;
    pairs_.assign(2 * (std::size_t)rc, 0);
    (void)sim3opt_place_batch_get_pairs(b_, rc, &np, pairs_.data());
    detected_ = true;
    return rc;
  }

  sim3opt_place_batch* b_;
  sim3opt_place_batch_options opt_;
  std::string err_;
  std::vector<int32_t> kp_ptr_ = std::vector<int32_t>(1, 0), pairs_;
  std::vector<float> desc_;
  std::vector<DetectionResult> results_;
  bool detected_ = false;
};

}  // namespace sim3opt_shim
