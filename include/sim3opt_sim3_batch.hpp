// sim3opt_sim3_batch.hpp -- header-only C++ helper for the Sim(3) measurement of a loop candidate with its information
// matrix, forwarding to the sim3opt_sim3_batch_* entry points of libsim3opt (include/sim3opt.h, "batched Sim(3) RANSAC
// and refinement").
//
// The reference gives every loop edge the identity as information (kitti_surf.cpp:167, 202: inf7 = Identity(7)), takes
// the scale from a ratio of median depths (kittiDetector.h:1305-1311) and never fills Constraint::fisher_information
// (kittiDetector.h:404-422).  With this helper the call site collects the matches of every accepted candidate and, after
// the loop, has a measurement and an information matrix for each, in the layouts the g2o shim takes:
//
//     sim3opt_shim::Sim3Batch sb;                                            // before the loop
//     int id = sb.add(points1, points2, depth1, depth2, K_rowmajor);         // per candidate, or
//     sb.feed(n, match_ptr, uv0, uv1, depth0, depth1, K_rowmajor);           // what LoopMatchBatch / sim3opt_match_batch_get_* return
//     ...
//     sb.solve();                                                            // every candidate, one launch
//     if (sb.good(id)) {
//       vio::EdgeSim3* e = new vio::EdgeSim3();  e->setVertex(0, vi);  e->setVertex(1, vj);
//       e->setMeasurement(g2o::Sim3(sb.measurement(id)));                    // Sji: X_j = s R X_i + t
//       e->information() = sb.information(id);                               // 7 x 7, [omega upsilon sigma]
//       double d2;  if (optimizer.gateEdge(*e, d2) && d2 < 18.475) optimizer.addEdge(e);    // chi^2_7 at 0.99
//     }
//
// PARITY UNPINNED: the reference has no such step (include/sim3opt.h says what the method is and where it departs from
// ORB-SLAM's Sim3Solver / OptimizeSim3); a seed gives the same result on every run.  add() takes any point type with
// public x, y members (cv::Point2f) and K as 9 doubles row-major.  No Eigen, no OpenCV.  All candidates of a batch
// share one K.  Omega holds for points without error: pixel_noise (options()) scales it.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"

namespace sim3opt_shim {

class Sim3Batch {
 public:
  // what information(id) returns: a 7 x 7 matrix-like (operator()(r, c)) over the stage's column-major block, which
  // edge->information() = ... of sim3opt_g2o.hpp and Eigen's Matrix<double, 7, 7> constructor-by-elements both take
  class Information {
   public:
    explicit Information(const double* a) : a_(a) {}
    double operator()(int r, int c) const { return a_[7 * c + r]; }
    const double* data() const { return a_; }  // column-major: the `info` of sim3opt_add_edge / sim3opt_gate_edges
   private:
    const double* a_;
  };

  Sim3Batch() : b_(sim3opt_sim3_batch_create()) { sim3opt_sim3_batch_options_default(&opt_); }
  ~Sim3Batch() { sim3opt_sim3_batch_destroy(b_); }
  Sim3Batch(const Sim3Batch&) = delete;
  Sim3Batch& operator=(const Sim3Batch&) = delete;

  sim3opt_sim3_batch_options& options() { return opt_; }  // read at solve()
  const std::string& last_error() const { return err_; }
  int size() const { return (int)ptr_.size() - 1; }
  void clear() {
    ptr_.assign(1, 0);
    uv0_.clear(); uv1_.clear(); d0_.clear(); d1_.clear();
    solved_ = false;
  }

  // One candidate; returns its index, or -1 (last_error() says why) with nothing added.
  template <class P2, class D>
  int add(const std::vector<P2>& points1, const std::vector<P2>& points2, const std::vector<D>& depth1,
          const std::vector<D>& depth2, const double* K) {
    if (!K) return fail("add: NULL argument");
    if (points1.empty() || points1.size() != points2.size() || depth1.size() != points1.size() ||
        depth2.size() != points1.size())
      return fail("add: the point and depth lists must have one common, non-zero length");
    if (!same_camera(K)) return fail("add: every candidate of a batch shares one K");
    for (std::size_t i = 0; i < points1.size(); ++i)
      if (!((double)depth1[i] > 0) || !((double)depth2[i] > 0)) return fail("add: a depth is not positive");
    set_camera(K);
    for (std::size_t i = 0; i < points1.size(); ++i) {
      uv0_.push_back((double)points1[i].x); uv0_.push_back((double)points1[i].y);
      uv1_.push_back((double)points2[i].x); uv1_.push_back((double)points2[i].y);
      d0_.push_back((double)depth1[i]); d1_.push_back((double)depth2[i]);
    }
    ptr_.push_back((int32_t)d0_.size());
    solved_ = false;
    return size() - 1;
  }

  // n candidates at once from the arrays sim3opt_match_batch_get_match_ptr / _get_matches return; the index of the
  // first, or -1 with nothing added.  A candidate without a match is refused: leave it out of match_ptr.
  int feed(int32_t n, const int32_t* match_ptr, const double* uv0, const double* uv1, const double* depth0,
           const double* depth1, const double* K) {
    if (n < 1 || !match_ptr || !uv0 || !uv1 || !depth0 || !depth1 || !K) return fail("feed: bad argument");
    if (!same_camera(K)) return fail("feed: every candidate of a batch shares one K");
    if (match_ptr[0] != 0) return fail("feed: match_ptr[0] must be 0");
    for (int32_t k = 0; k < n; ++k)
      if (match_ptr[k + 1] <= match_ptr[k]) return fail("feed: a candidate has no match");
    set_camera(K);
    const int first = size();
    const int32_t base = ptr_.back();
    const std::size_t m = (std::size_t)match_ptr[n];
    uv0_.insert(uv0_.end(), uv0, uv0 + 2 * m); uv1_.insert(uv1_.end(), uv1, uv1 + 2 * m);
    d0_.insert(d0_.end(), depth0, depth0 + m); d1_.insert(d1_.end(), depth1, depth1 + m);
    for (int32_t k = 1; k <= n; ++k) ptr_.push_back(base + match_ptr[k]);
    solved_ = false;
    return first;
  }

  // Every candidate added so far: one launch.  Candidates with status 0, or a negative SIM3OPT_ERR_*.
  int solve() {
    if (!b_) return fail("solve: out of memory", SIM3OPT_ERR_ARG);
    int rc = sim3opt_sim3_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK)
      rc = sim3opt_sim3_batch_set_problems(b_, size(), ptr_.data(), uv0_.data(), uv1_.data(), d0_.data(), d1_.data(),
                                           f_, cx_, cy_);
    if (rc == SIM3OPT_OK) rc = sim3opt_sim3_batch_solve(b_);
    if (rc < 0) return fail(sim3opt_sim3_batch_last_error(b_), rc);
    const std::size_t n = (std::size_t)size();
    sim_.assign(8 * n, 0.0); info_.assign(49 * n, 0.0); rms_.assign(n, 0.0);
    mask_.assign(d0_.size(), 0); inliers_.assign(n, 0); status_.assign(n, 0);
    (void)sim3opt_sim3_batch_get_sim3(b_, sim_.data(), info_.data());
    (void)sim3opt_sim3_batch_get_inliers(b_, mask_.data(), inliers_.data());
    (void)sim3opt_sim3_batch_get_summary(b_, status_.data(), nullptr, nullptr, nullptr, rms_.data(), nullptr, nullptr);
    solved_ = true;
    return rc;
  }

  // ---- results of candidate id, after solve() (before: the identity, zero information, no inliers, status -1) ----
  int n_points(int id) const { return ptr_[id + 1] - ptr_[id]; }
  int status(int id) const { return solved_ ? status_[id] : -1; }  // SIM3OPT_SIM3_*
  bool good(int id) const { return solved_ && status_[id] == SIM3OPT_SIM3_OK; }
  // [qx qy qz qw tx ty tz s] with X1 = s R X0 + t: the `meas` of sim3opt_add_edge(v0 = first frame, v1 = second),
  // what g2o::Sim3(const double[8]) of sim3opt_g2o.hpp and SparseOptimizer::gateEdge's edge take
  const double* measurement(int id) const { return solved_ ? &sim_[8 * (std::size_t)id] : kIdentity(); }
  Information information(int id) const { return Information(solved_ ? &info_[49 * (std::size_t)id] : kZero()); }
  double scale(int id) const { return measurement(id)[7]; }
  double rms_px(int id) const { return solved_ ? rms_[id] : 0.0; }
  int n_inliers(int id) const { return solved_ ? inliers_[id] : 0; }
  bool inlier(int id, int i) const { return solved_ && mask_[(std::size_t)ptr_[id] + i] != 0; }

 private:
  int fail(const std::string& why, int rc = -1) { err_ = why; return rc; }
  bool same_camera(const double* K) const { return size() == 0 || (K[0] == f_ && K[2] == cx_ && K[5] == cy_); }
  void set_camera(const double* K) { f_ = K[0]; cx_ = K[2]; cy_ = K[5]; }
  static const double* kIdentity() {
    static const double id[8] = {0, 0, 0, 1, 0, 0, 0, 1};
    return id;
  }
  static const double* kZero() {
    static const double z[49] = {};
    return z;
  }

  sim3opt_sim3_batch* b_;
  sim3opt_sim3_batch_options opt_;
  std::string err_;
  std::vector<int32_t> ptr_ = std::vector<int32_t>(1, 0);
  std::vector<double> uv0_, uv1_, d0_, d1_, sim_, info_, rms_;
  std::vector<uint8_t> mask_;
  std::vector<int32_t> inliers_, status_;
  double f_ = 0, cx_ = 0, cy_ = 0;
  bool solved_ = false;
};

}  // namespace sim3opt_shim
