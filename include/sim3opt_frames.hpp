// sim3opt_frames.hpp -- header-only C++ helper for the device-resident frame store, forwarding to the sim3opt_frames_*
// entry points of libsim3opt (include/sim3opt.h, "device-resident frame store").
//
// Stage by stage, the helpers of the detector chain hand kp_ptr / kp / desc to each other through host vectors, and
// each stage uploads a copy of its own.  With one store the extractor fills the frames on the device and the three
// consumers read them where they are:
//
//     sim3opt_shim::FrameStore frames;
//     surf.extract(frames);                 // SurfExtractorBatch: kp and desc stay on the device
//     voc.create(frames);                   // VocabularyTrainer
//     voc.feed(places); places.detect(frames);      // LoopDetectorBatch
//     for (f ...) matches.add_frame(no_keys, nullptr, obs[f], depths[f]);   // LoopMatchBatch: the map observations only
//     places.feed(matches); matches.solve(frames);
//
// What the store holds is an immutable snapshot: a stage that took it keeps it through a refill and through the
// store's destruction.  No Eigen, no OpenCV.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"

namespace sim3opt_shim {

class FrameStore {
 public:
  FrameStore() : s_(sim3opt_frames_create()) { sim3opt_frames_options_default(&opt_); }
  ~FrameStore() { sim3opt_frames_destroy(s_); }
  FrameStore(const FrameStore&) = delete;
  FrameStore& operator=(const FrameStore&) = delete;

  // read at prepare(), which every filler calls first
  sim3opt_frames_options& options() { return opt_; }
  const std::string& last_error() const { return err_; }
  sim3opt_frames* handle() { return s_; }

  // the options handed to the library: SIM3OPT_OK, or SIM3OPT_ERR_ARG with the store as it was
  int prepare() {
    if (!s_) return fail("prepare: out of memory", SIM3OPT_ERR_ARG);
    const int rc = sim3opt_frames_set_options(s_, &opt_);
    return rc == SIM3OPT_OK ? rc : fail(sim3opt_frames_last_error(s_), rc);
  }

  // One upload of the flat arrays sim3opt_match_batch_set_frames takes.  SIM3OPT_OK, or a negative SIM3OPT_ERR_* with the
  // reason in last_error() and the store as it was.
  int set(int n_frames, const int32_t* kp_ptr, const float* kp, const float* desc) {
    int rc = prepare();
    const float none = 0.f;  // (the C-ABI refuses a NULL array; frames without keypoints still have one)
    if (rc == SIM3OPT_OK) rc = sim3opt_frames_set(s_, n_frames, kp_ptr, kp ? kp : &none, desc ? desc : &none);
    return rc == SIM3OPT_OK ? rc : fail(sim3opt_frames_last_error(s_), rc);
  }

  // 0 before a fill
  int n_frames() const { return dim(0); }
  int total_keypoints() const { return dim(1); }
  bool filled() const { return dim(2) >= 0; }

  // the host mirror of kp_ptr ({0} before a fill): nothing is read from the device
  std::vector<int32_t> kp_ptr() const {
    std::vector<int32_t> p((std::size_t)n_frames() + 1, 0);
    if (filled()) (void)sim3opt_frames_get(s_, p.data(), nullptr, nullptr);
    return p;
  }

  // the read-back: SIM3OPT_OK, or SIM3OPT_ERR_STATE before a fill
  int get(std::vector<float>& kp, std::vector<float>& desc) {
    if (!s_ || !filled()) return fail("get: the store is not filled", SIM3OPT_ERR_STATE);
    const std::size_t n = (std::size_t)total_keypoints();
    kp.assign(2 * n, 0.f); desc.assign(64 * n, 0.f);
    const int rc = sim3opt_frames_get(s_, nullptr, kp.data(), desc.data());
    return rc == SIM3OPT_OK ? rc : fail(sim3opt_frames_last_error(s_), rc);
  }

 private:
  int fail(const std::string& why, int rc) { err_ = why; return rc; }
  int dim(int which) const {
    int32_t v[3] = {0, 0, -1};
    if (s_) (void)sim3opt_frames_get_dims(s_, &v[0], &v[1], &v[2], nullptr, nullptr);
    return v[which];
  }

  sim3opt_frames* s_;
  sim3opt_frames_options opt_;
  std::string err_;
};

}  // namespace sim3opt_shim
