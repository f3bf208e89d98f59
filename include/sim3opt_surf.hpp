// sim3opt_surf.hpp -- header-only C++ helper for the head of the detector chain, forwarding to the
// sim3opt_surf_batch_* entry points of libsim3opt (include/sim3opt.h, "batched SURF-64 extraction").
//
// The reference extracts once per keyframe, on the CPU, through OpenCV's contrib module:
//
//     SurfExtractor extractor;                                                     // kitti_surf.cpp:501-523
//     extractor(im, keys, descriptors);     // cv::xfeatures2d::SURF::create(400): detect + compute, 64 floats each
//
// With this helper the images of a sequence are collected and extracted in one batch on the device:
//
//     sim3opt_shim::SurfExtractorBatch surf;
//     for (const cv::Mat& im : images) surf.add(im.data, im.cols, im.rows, (int)im.step);   // grey, 8 bit
//     surf.extract();
//     surf.keys(f); surf.descriptors(f);    // frame f in the shapes operator() fills
//     voc.create(surf.n_frames(), surf.kp_ptr().data(), surf.desc().data());                // the next stages take the
//     for (int f = 0; f < surf.n_frames(); ++f) places.add_frame(surf.frame_desc(f), surf.count(f));   // flat arrays
//
// PARITY UNPINNED: OpenCV is not part of the reference tree; include/sim3opt.h holds the definition and says what is
// the call site's (minHessian = 400, defaults, 64 floats) and what is recalled from upstream.  One image size per
// batch.  No Eigen, no OpenCV.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"
#include "sim3opt_frames.hpp"

namespace sim3opt_shim {

// the fields of cv::KeyPoint that SURF fills (class_id carries the sign of the Laplacian there)
struct SurfKey {
  float x, y, size, angle, response;
  int octave, laplacian;
};

class SurfExtractorBatch {
 public:
  SurfExtractorBatch() : b_(sim3opt_surf_batch_create()) { sim3opt_surf_batch_options_default(&opt_); }
  ~SurfExtractorBatch() { sim3opt_surf_batch_destroy(b_); }
  SurfExtractorBatch(const SurfExtractorBatch&) = delete;
  SurfExtractorBatch& operator=(const SurfExtractorBatch&) = delete;

  // read at extract()
  sim3opt_surf_batch_options& options() { return opt_; }
  const std::string& last_error() const { return err_; }
  int n_frames() const { return n_; }

  // One grey 8-bit image per call, rows `stride` bytes apart; copied.  SIM3OPT_OK, or SIM3OPT_ERR_ARG with the images
  // collected so far as they were: NULL, a size under 1, stride < width, a size other than the first image's.
  int add(const unsigned char* data, int width, int height, int stride) {
    if (!data) return fail("add: data is NULL", SIM3OPT_ERR_ARG);
    if (width < 1 || height < 1) return fail("add: width or height < 1", SIM3OPT_ERR_ARG);
    if (stride < width) return fail("add: stride < width", SIM3OPT_ERR_ARG);
    if (n_ > 0 && (width != w_ || height != h_)) return fail("add: an image of another size (one size per batch)", SIM3OPT_ERR_ARG);
    w_ = width; h_ = height;
    for (int y = 0; y < height; ++y) pixels_.insert(pixels_.end(), data + (std::size_t)y * (std::size_t)stride, data + (std::size_t)y * (std::size_t)stride + width);
    ++n_;
    return SIM3OPT_OK;
  }

  // forgets the images and the results
  void clear() {
    pixels_.clear(); n_ = w_ = h_ = 0;
    kp_ptr_.assign(1, 0); kp_.clear(); desc_.clear(); size_.clear(); angle_.clear(); response_.clear(); octave_.clear(); laplacian_.clear();
  }

  // The batch: the number of frames with keypoints, or a negative SIM3OPT_ERR_* with the reason in last_error() and
  // the results as they were.
  int extract() {
    if (!b_) return fail("extract: out of memory", SIM3OPT_ERR_ARG);
    if (n_ < 1) return fail("extract: no image added", SIM3OPT_ERR_STATE);
    int rc = sim3opt_surf_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK) rc = sim3opt_surf_batch_set_images(b_, n_, w_, h_, w_, pixels_.data());
    if (rc == SIM3OPT_OK) rc = sim3opt_surf_batch_solve(b_);
    if (rc < 0) return fail(sim3opt_surf_batch_last_error(b_), rc);
    std::vector<int32_t> ptr((std::size_t)n_ + 1);
    (void)sim3opt_surf_batch_get_kp_ptr(b_, ptr.data());
    const std::size_t n = (std::size_t)ptr.back();
    kp_ptr_.swap(ptr);
    kp_.assign(2 * n, 0.f); desc_.assign(64 * n, 0.f); size_.assign(n, 0.f); angle_.assign(n, 0.f); response_.assign(n, 0.f);
    octave_.assign(n, 0); laplacian_.assign(n, 0);
    (void)sim3opt_surf_batch_get_keypoints(b_, kp_.data(), desc_.data(), size_.data(), angle_.data(), response_.data(),
                                           octave_.data(), laplacian_.data());
    return rc;
  }

  // The batch with kp and desc left on the device in `store` (sim3opt_surf_batch_solve_into), for the stages that take a
  // FrameStore.  Returns as extract(); keys(f), kp_ptr() and count(f) answer as after extract(), desc() is empty and
  // descriptors(f) / frame_desc(f) have nothing to give: the descriptors are store.get()'s.
  int extract(FrameStore& store) {
    if (!b_) return fail("extract: out of memory", SIM3OPT_ERR_ARG);
    if (n_ < 1) return fail("extract: no image added", SIM3OPT_ERR_STATE);
    if (int rs = store.prepare()) return fail(store.last_error(), rs);
    int rc = sim3opt_surf_batch_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK) rc = sim3opt_surf_batch_set_images(b_, n_, w_, h_, w_, pixels_.data());
    if (rc == SIM3OPT_OK) rc = sim3opt_surf_batch_solve_into(b_, store.handle());
    if (rc < 0) return fail(sim3opt_surf_batch_last_error(b_), rc);
    std::vector<int32_t> ptr((std::size_t)n_ + 1);
    (void)sim3opt_surf_batch_get_kp_ptr(b_, ptr.data());
    const std::size_t n = (std::size_t)ptr.back();
    kp_ptr_.swap(ptr);
    kp_.assign(2 * n, 0.f); desc_.clear(); size_.assign(n, 0.f); angle_.assign(n, 0.f); response_.assign(n, 0.f);
    octave_.assign(n, 0); laplacian_.assign(n, 0);
    (void)sim3opt_surf_batch_get_keypoints(b_, kp_.data(), nullptr, size_.data(), angle_.data(), response_.data(),
                                           octave_.data(), laplacian_.data());
    return rc;
  }

  // the flat arrays sim3opt_match_batch_set_frames, sim3opt_place_batch_set_frames and sim3opt_vocabulary_set_frames take
  const std::vector<int32_t>& kp_ptr() const { return kp_ptr_; }
  const std::vector<float>& kp() const { return kp_; }      // x, y per keypoint
  const std::vector<float>& desc() const { return desc_; }  // 64 per keypoint
  int count(int f) const { return f >= 0 && f + 1 < (int)kp_ptr_.size() ? kp_ptr_[(std::size_t)f + 1] - kp_ptr_[(std::size_t)f] : 0; }
  const float* frame_desc(int f) const { return desc_.data() + 64 * (std::size_t)(count(f) ? kp_ptr_[(std::size_t)f] : 0); }

  // frame f in the shapes SurfExtractor::operator() fills (empty for a frame out of range)
  std::vector<SurfKey> keys(int f) const {
    std::vector<SurfKey> out;
    for (int k = 0; k < count(f); ++k) {
      const std::size_t i = (std::size_t)(kp_ptr_[(std::size_t)f] + k);
      out.push_back(SurfKey{kp_[2 * i], kp_[2 * i + 1], size_[i], angle_[i], response_[i], octave_[i], laplacian_[i]});
    }
    return out;
  }
  std::vector<std::vector<float>> descriptors(int f) const {
    std::vector<std::vector<float>> out;
    for (int k = 0; k < count(f) && !desc_.empty(); ++k) {
      const float* d = desc_.data() + 64 * (std::size_t)(kp_ptr_[(std::size_t)f] + k);
      out.emplace_back(d, d + 64);
    }
    return out;
  }

 private:
  int fail(const std::string& why, int rc) { err_ = why; return rc; }

  sim3opt_surf_batch* b_;
  sim3opt_surf_batch_options opt_;
  std::string err_;
  std::vector<unsigned char> pixels_;
  int n_ = 0, w_ = 0, h_ = 0;
  std::vector<int32_t> kp_ptr_ = std::vector<int32_t>(1, 0), octave_, laplacian_;
  std::vector<float> kp_, desc_, size_, angle_, response_;
};

}  // namespace sim3opt_shim
