// sim3opt_homography.hpp -- header-only C++ helper for the loop detector's planar relative pose, forwarding to the
// sim3opt_homography_batch_* entry points of libsim3opt (include/sim3opt.h, "batched homography MLESAC").
//
// The reference estimates it for every accepted loop candidate on its own (kittiDetector.h:1387-1443, inside the loop
// of computeConstraints, the USE_KLEIN record line):
//
//     std::vector<HomographyMatch> vMatches;  ...  m.v2CamPlaneFirst = Camera.UnProject(vfirst);  ...
//     bGood = HomographyInit.Compute(vMatches, 5.0, se3);
//     double dTransMagn = sqrt(se3.get_translation() * se3.get_translation());
//     if (dTransMagn == 0) ...            // "estimated zero baseline"
//     se3.get_translation() *= 1 / dTransMagn;
//
// With this helper the call site collects instead, and runs one launch after the loop:
//
//     sim3opt_shim::HomographyBatch hb;                              // before the loop
//     int id = hb.add(points1, points2, K_rowmajor);                 // at :1393-1409, if point_count > 8
//     ...
//     hb.solve();                                                    // after the loop: every candidate, one launch
//     if (hb.good(id)) { double R[9]; hb.rotation(id, R); const double* t = hb.translation(id); }   // :1415-1436
//
// good(id) is bGood of :1414 and a non-zero baseline (:1423-1429); translation(id) is the unit vector of :1431.
// PARITY UNPINNED: the reference's sampling is not reproducible (include/sim3opt.h says what else differs: the pinhole
// in ATANCamera's place, the tie rule, ten points at least); a seed gives the same poses on every run.  add() takes any
// point type with public x, y members (cv::Point2f) and K as 9 doubles row-major.  No Eigen, no OpenCV, no TooN.  All
// candidates of a batch share one K.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"

namespace sim3opt_shim {

class HomographyBatch {
 public:
  HomographyBatch() : b_(sim3opt_homography_batch_create()) { sim3opt_homography_batch_options_default(&opt_); }
  ~HomographyBatch() { sim3opt_homography_batch_destroy(b_); }
  HomographyBatch(const HomographyBatch&) = delete;
  HomographyBatch& operator=(const HomographyBatch&) = delete;

  // dMaxPixelError of :1414 and the rest of sim3opt_homography_batch_options; read at solve()
  sim3opt_homography_batch_options& options() { return opt_; }
  const std::string& last_error() const { return err_; }
  int size() const { return (int)ptr_.size() - 1; }
  void clear() {
    ptr_.assign(1, 0);
    uv0_.clear(); uv1_.clear();
    solved_ = false;
  }

  // One candidate; returns its index, or -1 (last_error() says why) with nothing added.
  template <class P2>
  int add(const std::vector<P2>& points1, const std::vector<P2>& points2, const double* K) {
    if (!K) return fail("add: NULL argument");
    if (points1.empty() || points1.size() != points2.size())
      return fail("add: the two point lists must have one common, non-zero length");
    if (size() == 0) {
      f_ = K[0]; cx_ = K[2]; cy_ = K[5];
    } else if (K[0] != f_ || K[2] != cx_ || K[5] != cy_) {
      return fail("add: every candidate of a batch shares one K");
    }
    for (std::size_t i = 0; i < points1.size(); ++i) {
      uv0_.push_back((double)points1[i].x); uv0_.push_back((double)points1[i].y);
      uv1_.push_back((double)points2[i].x); uv1_.push_back((double)points2[i].y);
    }
    ptr_.push_back((int32_t)(uv0_.size() / 2));
    solved_ = false;
    return size() - 1;
  }

  // Every candidate added so far: one launch.  Candidates with status 0, or a negative SIM3OPT_ERR_*.
  int solve() {
    if (!b_) return fail("solve: out of memory", SIM3OPT_ERR_ARG);
    int rc = sim3opt_homography_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK)
      rc = sim3opt_homography_batch_set_problems(b_, size(), ptr_.data(), uv0_.data(), uv1_.data(), f_, cx_, cy_);
    if (rc == SIM3OPT_OK) rc = sim3opt_homography_batch_solve(b_);
    if (rc < 0) return fail(sim3opt_homography_batch_last_error(b_), rc);
    const std::size_t n = (std::size_t)size();
    pose_.assign(7 * n, 0.0); H_.assign(9 * n, 0.0); unit_.assign(3 * n, 0.0);
    mask_.assign(uv0_.size() / 2, 0); inliers_.assign(n, 0); status_.assign(n, 0);
    (void)sim3opt_homography_batch_get_poses(b_, pose_.data());
    (void)sim3opt_homography_batch_get_homographies(b_, nullptr, H_.data());
    (void)sim3opt_homography_batch_get_inliers(b_, mask_.data(), inliers_.data());
    (void)sim3opt_homography_batch_get_summary(b_, status_.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr);
    for (std::size_t k = 0; k < n; ++k) {  // :1423-1431
      const double* t = &pose_[7 * k + 4];
      const double magn = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
      if (magn == 0 || !std::isfinite(magn)) continue;
      for (int i = 0; i < 3; ++i) unit_[3 * k + i] = t[i] * (1 / magn);
    }
    solved_ = true;
    return rc;
  }

  // ---- results of candidate id, after solve() (before: the identity, zero t, no inliers, status -1) ----
  int n_points(int id) const { return ptr_[id + 1] - ptr_[id]; }
  int status(int id) const { return solved_ ? status_[id] : -1; }                      // SIM3OPT_HOMOGRAPHY_*
  // bGood of :1414 and "estimated a non-zero baseline" of :1423-1429
  bool good(int id) const {
    if (!solved_ || status_[id] != SIM3OPT_HOMOGRAPHY_OK) return false;
    const double* u = &unit_[3 * (std::size_t)id];
    return u[0] != 0 || u[1] != 0 || u[2] != 0;
  }
  const double* quaternion(int id) const { return solved_ ? &pose_[7 * (std::size_t)id] : kIdentity(); }  // x y z w
  const double* translation(int id) const { return solved_ ? &unit_[3 * (std::size_t)id] : kIdentity() + 4; }  // :1431
  const double* translation_as_computed(int id) const { return quaternion(id) + 4; }   // se3's own, :61
  const double* homography(int id) const { return solved_ ? &H_[9 * (std::size_t)id] : kIdentity() + 7; }  // refined
  void rotation(int id, double* R) const {                                             // row-major
    const double* q = quaternion(id);
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
  }
  int n_inliers(int id) const { return solved_ ? inliers_[id] : 0; }                   // mvHomographyInliers.size()
  bool inlier(int id, int i) const { return solved_ && mask_[(std::size_t)ptr_[id] + i] != 0; }

 private:
  int fail(const std::string& why, int rc = -1) { err_ = why; return rc; }
  static const double* kIdentity() {
    static const double id[16] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return id;
  }

  sim3opt_homography_batch* b_;
  sim3opt_homography_batch_options opt_;
  std::string err_;
  std::vector<int32_t> ptr_ = std::vector<int32_t>(1, 0);
  std::vector<double> uv0_, uv1_, pose_, H_, unit_;
  std::vector<uint8_t> mask_;
  std::vector<int32_t> inliers_, status_;
  double f_ = 0, cx_ = 0, cy_ = 0;
  bool solved_ = false;
};

}  // namespace sim3opt_shim
