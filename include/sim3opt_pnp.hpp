// sim3opt_pnp.hpp -- header-only C++ helper for the loop detector's start pose, forwarding to the
// sim3opt_pnp_batch_* entry points of libsim3opt (include/sim3opt.h, "batched PnP RANSAC").
//
// The reference estimates camera 1 for every accepted loop candidate on its own (kittiDetector.h:1300-1301, inside
// the loop of computeConstraints), and refines it at once (:1325):
//
//     cv::solvePnPRansac(surfPoints[0], points2, K, dist, rvec, tvec, false, 100, 3, 10, noArray(), CV_ITERATIVE);
//     Rodrigues(rvec, Rf2s);
//     BAOptimize(surfPoints[0], points1, points2, K, OptParams(10, true, 3), Rf2s, tvec);
//
// With this helper and sim3opt_two_view.hpp the call site collects instead, and runs two launches after the loop:
//
//     sim3opt_shim::PnpRansacBatch pnp;                              // before the loop
//     int id = pnp.add(surfPoints[0], points2, K_rowmajor);          // at :1300
//     ...
//     pnp.solve();                                                   // after the loop: every candidate, one launch
//     double Rf2s[9]; pnp.rotation(id, Rf2s);                        // Rodrigues(rvec) of :1302, row-major
//     refiner.add(surfPoints[0], points1, points2, K_rowmajor, Rf2s, pnp.translation(id));   // TwoViewRefiner, :1325
//     ...
//     refiner.optimize();
//
// PARITY UNPINNED: this is not OpenCV's solvePnPRansac restated (include/sim3opt.h says what differs); a seed gives
// the same poses on every run.  add() takes any point types with public x, y(, z) members (cv::Point3f,
// cv::Point2f) and K as 9 doubles row-major.  No Eigen, no OpenCV.  All candidates of a batch share one K.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"

namespace sim3opt_shim {

class PnpRansacBatch {
 public:
  PnpRansacBatch() : b_(sim3opt_pnp_batch_create()) { sim3opt_pnp_batch_options_default(&opt_); }
  ~PnpRansacBatch() { sim3opt_pnp_batch_destroy(b_); }
  PnpRansacBatch(const PnpRansacBatch&) = delete;
  PnpRansacBatch& operator=(const PnpRansacBatch&) = delete;

  // iterationsCount, reprojectionError, minInliersCount of :1301 and the rest of sim3opt_pnp_batch_options; read at solve()
  sim3opt_pnp_batch_options& options() { return opt_; }
  const std::string& last_error() const { return err_; }
  int size() const { return (int)ptr_.size() - 1; }
  void clear() {
    ptr_.assign(1, 0);
    pts_.clear(); uv_.clear();
    solved_ = false;
  }

  // One candidate; returns its index, or -1 (last_error() says why) with nothing added.
  template <class P3, class P2>
  int add(const std::vector<P3>& pointsXYZ, const std::vector<P2>& points2, const double* K) {
    if (!K) return fail("add: NULL argument");
    if (pointsXYZ.empty() || pointsXYZ.size() != points2.size())
      return fail("add: the two point lists must have one common, non-zero length");
    if (size() == 0) {
      f_ = K[0]; cx_ = K[2]; cy_ = K[5];
    } else if (K[0] != f_ || K[2] != cx_ || K[5] != cy_) {
      return fail("add: every candidate of a batch shares one K");
    }
    for (std::size_t i = 0; i < pointsXYZ.size(); ++i) {
      pts_.push_back((double)pointsXYZ[i].x); pts_.push_back((double)pointsXYZ[i].y); pts_.push_back((double)pointsXYZ[i].z);
      uv_.push_back((double)points2[i].x); uv_.push_back((double)points2[i].y);
    }
    ptr_.push_back((int32_t)(pts_.size() / 3));
    solved_ = false;
    return size() - 1;
  }

  // Every candidate added so far: one launch.  Candidates with status 0, or a negative SIM3OPT_ERR_*.
  int solve() {
    if (!b_) return fail("solve: out of memory", SIM3OPT_ERR_ARG);
    int rc = sim3opt_pnp_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK)
      rc = sim3opt_pnp_batch_set_problems(b_, size(), ptr_.data(), pts_.data(), uv_.data(), f_, cx_, cy_);
    if (rc == SIM3OPT_OK) rc = sim3opt_pnp_batch_solve(b_);
    if (rc < 0) return fail(sim3opt_pnp_batch_last_error(b_), rc);
    const std::size_t n = (std::size_t)size();
    cam1_.assign(7 * n, 0.0); mask_.assign(uv_.size() / 2, 0); inliers_.assign(n, 0); status_.assign(n, 0);
    rms_.assign(n, 0.0);
    (void)sim3opt_pnp_batch_get_poses(b_, cam1_.data());
    (void)sim3opt_pnp_batch_get_inliers(b_, mask_.data(), inliers_.data());
    (void)sim3opt_pnp_batch_get_summary(b_, status_.data(), nullptr, nullptr, nullptr, rms_.data(), nullptr);
    solved_ = true;
    return rc;
  }

  // ---- results of candidate id, after solve() (before: the identity, no inliers, status -1) ----
  int n_points(int id) const { return ptr_[id + 1] - ptr_[id]; }
  int status(int id) const { return solved_ ? status_[id] : -1; }                      // SIM3OPT_PNP_*
  const double* quaternion(int id) const { return solved_ ? &cam1_[7 * (std::size_t)id] : kIdentity(); }  // x y z w
  const double* translation(int id) const { return quaternion(id) + 4; }               // tvec of :1300
  void rotation(int id, double* R) const {                                             // Rf2s of :1302, row-major
    const double* q = quaternion(id);
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
  }
  int n_inliers(int id) const { return solved_ ? inliers_[id] : 0; }
  bool inlier(int id, int i) const { return solved_ && mask_[(std::size_t)ptr_[id] + i] != 0; }
  double rms_px(int id) const { return solved_ ? rms_[id] : 0.0; }

 private:
  int fail(const std::string& why, int rc = -1) { err_ = why; return rc; }
  static const double* kIdentity() {
    static const double id[7] = {0, 0, 0, 1, 0, 0, 0};
    return id;
  }

  sim3opt_pnp_batch* b_;
  sim3opt_pnp_batch_options opt_;
  std::string err_;
  std::vector<int32_t> ptr_ = std::vector<int32_t>(1, 0);
  std::vector<double> pts_, uv_, cam1_, rms_;
  std::vector<uint8_t> mask_;
  std::vector<int32_t> inliers_, status_;
  double f_ = 0, cx_ = 0, cy_ = 0;
  bool solved_ = false;
};

}  // namespace sim3opt_shim
