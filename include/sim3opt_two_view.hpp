// sim3opt_two_view.hpp -- header-only C++ helper for the loop detector's two-view refinement, forwarding to
// the sim3opt_ba_batch_* entry points of libsim3opt (include/sim3opt.h, "batched two-view bundle adjustment").
//
// The reference refines every accepted loop candidate on its own (kittiDetector.h:1325, inside the loop of
// computeConstraints):
//
//     BAOptimize(pointsXYZ, points1, points2, K, OptParams(10, true, 3), Rf2s, tfins);     // :845-954
//
// With this helper the call site collects instead, and refines all candidates with one kernel launch after the loop:
//
//     sim3opt_shim::TwoViewRefiner refiner;                         // before the loop
//     int id = refiner.add(pointsXYZ, points1, points2, K_rowmajor, Rf2s_rowmajor, tfins);   // at :1325
//     ...
//     refiner.optimize();                                           // after the loop
//     refiner.rotation(id) / refiner.translation(id)                // Rf2s, tfins of :915-921
//     refiner.init_error(id) / final_error(id) / n_incorrect_edges(id)      // what :907 and :953 print
//
// add() takes the arguments BAOptimize takes: any point types with public x, y(, z) members (cv::Point3f,
// cv::Point2f), K, Rf2s as 9 doubles row-major, tfins as 3 doubles.  No Eigen, no OpenCV.  All candidates of a
// refiner share one K (the detector has one camera); camera 0 is the identity, as in the reference (:861-869).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"

namespace sim3opt_shim {

class TwoViewRefiner {
 public:
  TwoViewRefiner() : b_(sim3opt_ba_batch_create()) { sim3opt_ba_batch_options_default(&opt_); }
  ~TwoViewRefiner() { sim3opt_ba_batch_destroy(b_); }
  TwoViewRefiner(const TwoViewRefiner&) = delete;
  TwoViewRefiner& operator=(const TwoViewRefiner&) = delete;

  // OptParams(num_iters, ?, huber_kernel_width) and the rest of sim3opt_ba_batch_options; read at optimize()
  sim3opt_ba_batch_options& options() { return opt_; }
  const std::string& last_error() const { return err_; }
  int size() const { return (int)ptr_.size() - 1; }
  void clear() {
    ptr_.assign(1, 0);
    cam1_.clear(); pts_.clear(); uv0_.clear(); uv1_.clear(); iters_.clear();
    refined_ = false;
  }

  // One candidate; returns its index, or -1 (last_error() says why) with nothing added.
  template <class P3, class P2>
  int add(const std::vector<P3>& pointsXYZ, const std::vector<P2>& points1, const std::vector<P2>& points2,
          const double* K, const double* Rf2s, const double* tfins) {
    if (!K || !Rf2s || !tfins) return fail("add: NULL argument");
    if (pointsXYZ.empty() || pointsXYZ.size() != points1.size() || pointsXYZ.size() != points2.size())
      return fail("add: the three point lists must have one common, non-zero length");  // the assert of :903
    if (size() == 0) {
      f_ = K[0]; cx_ = K[2]; cy_ = K[5];
    } else if (K[0] != f_ || K[2] != cx_ || K[5] != cy_) {
      return fail("add: every candidate of a refiner shares one K");
    }
    double q[4];
    rotation_to_quaternion(Rf2s, q);
    for (int i = 0; i < 4; ++i) cam1_.push_back(q[i]);
    for (int i = 0; i < 3; ++i) cam1_.push_back(tfins[i]);
    for (std::size_t i = 0; i < pointsXYZ.size(); ++i) {
      pts_.push_back((double)pointsXYZ[i].x); pts_.push_back((double)pointsXYZ[i].y); pts_.push_back((double)pointsXYZ[i].z);
      uv0_.push_back((double)points1[i].x); uv0_.push_back((double)points1[i].y);
      uv1_.push_back((double)points2[i].x); uv1_.push_back((double)points2[i].y);
    }
    ptr_.push_back((int32_t)(pts_.size() / 3));
    refined_ = false;
    return size() - 1;
  }

  // Refines every candidate added so far: one launch.  Candidates refined, or a negative SIM3OPT_ERR_*.
  int optimize() {
    if (!b_) return fail("optimize: out of memory", SIM3OPT_ERR_ARG);
    int rc = sim3opt_ba_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK) {
      const int n = size();
      std::vector<double> cam0(7 * (std::size_t)(n > 0 ? n : 0), 0.0);
      for (int k = 0; k < n; ++k) cam0[7 * (std::size_t)k + 3] = 1.0;  // identity, :861-869
      rc = sim3opt_ba_batch_set_problems(b_, n, ptr_.data(), cam0.data(), cam1_.data(), pts_.data(), uv0_.data(),
                                         uv1_.data(), f_, cx_, cy_);
    }
    if (rc == SIM3OPT_OK) rc = sim3opt_ba_batch_optimize(b_);
    if (rc < 0) return fail(sim3opt_ba_batch_last_error(b_), rc);
    const std::size_t n = (std::size_t)size();
    before_.assign(n, 0.0); after_.assign(n, 0.0); outliers_.assign(n, 0); iters_.assign(n, 0);
    edge_chi2_.assign(uv0_.size() + uv1_.size(), 0.0);
    (void)sim3opt_ba_batch_get_cameras(b_, nullptr, cam1_.data());
    (void)sim3opt_ba_batch_get_points(b_, pts_.data());
    (void)sim3opt_ba_batch_get_chi2(b_, before_.data(), after_.data(), edge_chi2_.data(), outliers_.data());
    for (std::size_t k = 0; k < n; ++k) iters_[k] = sim3opt_ba_batch_num_iterations(b_, (int32_t)k);
    refined_ = true;
    return rc;
  }

  // ---- results of candidate k (the start values before optimize()) ----
  int n_points(int k) const { return ptr_[k + 1] - ptr_[k]; }
  const double* quaternion(int k) const { return &cam1_[7 * (std::size_t)k]; }       // x y z w of Rf2s
  const double* translation(int k) const { return &cam1_[7 * (std::size_t)k + 4]; }  // tfins, :917-921
  void rotation(int k, double* Rf2s) const {                                         // row-major, :915-916
    const double* q = quaternion(k);
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    Rf2s[0] = 1 - 2 * (y * y + z * z); Rf2s[1] = 2 * (x * y - z * w); Rf2s[2] = 2 * (x * z + y * w);
    Rf2s[3] = 2 * (x * y + z * w); Rf2s[4] = 1 - 2 * (x * x + z * z); Rf2s[5] = 2 * (y * z - x * w);
    Rf2s[6] = 2 * (x * z - y * w); Rf2s[7] = 2 * (y * z + x * w); Rf2s[8] = 1 - 2 * (x * x + y * y);
  }
  const double* points(int k) const { return &pts_[3 * (std::size_t)ptr_[k]]; }  // n_points(k) x 3
  // after optimize():
  double init_error(int k) const { return refined_ ? before_[k] : 0.0; }         // activeChi2 before, :785, :907
  double final_error(int k) const { return refined_ ? after_[k] : 0.0; }         // activeChi2 after, :787, :907
  int n_incorrect_edges(int k) const { return refined_ ? outliers_[k] : 0; }     // :947-953
  const double* edge_chi2(int k) const { return &edge_chi2_[2 * (std::size_t)ptr_[k]]; }  // n_points(k) x 2
  int iterations(int k) const { return refined_ ? iters_[k] : 0; }
  bool stats(int k, int iter, sim3opt_iter_stats* out) const {
    return refined_ && sim3opt_ba_batch_get_stats(b_, k, iter, out) == SIM3OPT_OK;
  }

  // Eigen's Quaternion(Matrix3) (the `qd = eigenRf2s` of :883): x y z w of a row-major rotation
  static void rotation_to_quaternion(const double* R, double q[4]) {
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
      double k = std::sqrt(tr + 1.0);
      q[3] = 0.5 * k; k = 0.5 / k;
      q[0] = (R[7] - R[5]) * k; q[1] = (R[2] - R[6]) * k; q[2] = (R[3] - R[1]) * k;
    } else {
      int i = 0;
      if (R[4] > R[0]) i = 1;
      if (R[8] > R[4 * i]) i = 2;
      const int j = (i + 1) % 3, l = (j + 1) % 3;
      double k = std::sqrt(R[4 * i] - R[4 * j] - R[4 * l] + 1.0);
      q[i] = 0.5 * k; k = 0.5 / k;
      q[3] = (R[3 * l + j] - R[3 * j + l]) * k;
      q[j] = (R[3 * j + i] + R[3 * i + j]) * k;
      q[l] = (R[3 * l + i] + R[3 * i + l]) * k;
    }
  }

 private:
  int fail(const std::string& why, int rc = -1) { err_ = why; return rc; }

  sim3opt_ba_batch* b_;
  sim3opt_ba_batch_options opt_;
  std::string err_;
  std::vector<int32_t> ptr_ = std::vector<int32_t>(1, 0);
  std::vector<double> cam1_, pts_, uv0_, uv1_, before_, after_, edge_chi2_;
  std::vector<int32_t> outliers_, iters_;
  double f_ = 0, cx_ = 0, cy_ = 0;
  bool refined_ = false;
};

}  // namespace sim3opt_shim
