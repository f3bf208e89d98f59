// sim3opt_tracks.hpp -- header-only C++ helper for the batched loop tracks, forwarding to the sim3opt_track_batch_*
// entry points of libsim3opt (include/sim3opt.h, "batched loop tracks").
//
// computeConstraints records every kept match of every loop pair as a two-observation track (kittiDetector.h:1493-1501)
// and SaveAsSfMInit connects them afterwards (kitti_surf.cpp:349-391).  With this helper the call site hands the pair's
// matches over and the connection, one 3-D point per track and the rows of the bundle adjustment come back at once:
//
//     sim3opt_shim::LoopTrackBatch tracks;
//     tracks.set_frames(n_frames, kp_ptr, kp);           // or set_frames(store): a sim3opt_shim::FrameStore, read in place
//     for (every loop pair)                               // kittiDetector.h:1493: good_matches, the RANSAC's inliers
//       tracks.add_pair(firstFrame, secondFrame, matches, mask);
//     tracks.set_cameras(states, focal, cx, cy);          // S_iw as sim3opt_get_vertices returns them
//     tracks.solve();
//     tracks.append_to(cams, points, obs_cam, obs_point, obs_uv);   // behind the map's rows: sim3opt_ba_set_problem takes them
//
// DEVIATIONS from SaveAsSfMInit are those of the C-ABI: a match between two tracks joins them, a track's observations
// are ordered by frame and keypoint, a track with a frame twice is reported (status 1) and left out of the rows.
// No Eigen, no OpenCV.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"
#include "sim3opt_frames.hpp"

namespace sim3opt_shim {

struct LoopMatch {  // cv::DMatch's queryIdx / trainIdx, and the map depths at the two keypoints (<= 0 or NaN: none)
  int query, train;
  double depth0, depth1;
  LoopMatch(int q = 0, int t = 0, double d0 = 0.0, double d1 = 0.0) : query(q), train(t), depth0(d0), depth1(d1) {}
};

class LoopTrackBatch {
 public:
  LoopTrackBatch() : b_(sim3opt_track_batch_create()) { sim3opt_track_batch_options_default(&opt_); clear_pairs(); }
  ~LoopTrackBatch() { sim3opt_track_batch_destroy(b_); }
  LoopTrackBatch(const LoopTrackBatch&) = delete;
  LoopTrackBatch& operator=(const LoopTrackBatch&) = delete;

  sim3opt_track_batch_options& options() { return opt_; }  // read at solve()
  const std::string& last_error() const { return err_; }
  sim3opt_track_batch* handle() { return b_; }

  // The frames every pair names.  SIM3OPT_OK, or a negative SIM3OPT_ERR_* with the reason in last_error() and the helper
  // as it was.  The pairs added so far stay.
  int set_frames(int n_frames, const int32_t* kp_ptr, const float* kp) {
    if (!b_) return fail("set_frames: out of memory", SIM3OPT_ERR_ARG);
    const float none = 0.f;  // (the C-ABI refuses a NULL array; frames without keypoints still have one)
    const int rc = sim3opt_track_batch_set_frames(b_, n_frames, kp_ptr, kp ? kp : &none);
    if (rc != SIM3OPT_OK) return fail(sim3opt_track_batch_last_error(b_), rc);
    n_frames_ = n_frames;
    return rc;
  }
  int set_frames(FrameStore& store) {
    if (!b_) return fail("set_frames: out of memory", SIM3OPT_ERR_ARG);
    int rc = sim3opt_track_batch_set_options(b_, &opt_);  // (the device the snapshot is checked against)
    if (rc == SIM3OPT_OK) rc = sim3opt_track_batch_set_frames_from(b_, store.handle());
    if (rc != SIM3OPT_OK) return fail(sim3opt_track_batch_last_error(b_), rc);
    n_frames_ = store.n_frames();
    return rc;
  }

  // The call site of kittiDetector.h:1493: the kept matches of one loop pair, with the inlier mask of the stage that
  // kept them (NULL: all).  Returns the pair's index.
  int add_pair(int frame0, int frame1, const std::vector<LoopMatch>& matches, const std::vector<uint8_t>* mask = nullptr) {
    pairs_.push_back(frame0); pairs_.push_back(frame1);
    for (std::size_t k = 0; k < matches.size(); ++k) {
      query_.push_back(matches[k].query); train_.push_back(matches[k].train);
      depth0_.push_back(matches[k].depth0); depth1_.push_back(matches[k].depth1);
      mask_.push_back(mask && k < mask->size() ? (*mask)[k] : 1);
    }
    match_ptr_.push_back((int32_t)query_.size());
    return (int)pairs_.size() / 2 - 1;
  }
  void clear_pairs() {
    pairs_.clear(); query_.clear(); train_.clear(); depth0_.clear(); depth1_.clear(); mask_.clear();
    match_ptr_.assign(1, 0);
  }
  int n_pairs() const { return (int)pairs_.size() / 2; }

  // states: 8 per frame, [qx qy qz qw tx ty tz s]
  int set_cameras(const std::vector<double>& states, double focal, double cx, double cy) {
    states_ = states; focal_ = focal; cx_ = cx; cy_ = cy;
    have_cams_ = true;
    return SIM3OPT_OK;
  }

  // The number of status-0 tracks, or a negative SIM3OPT_ERR_* with the reason in last_error().
  int solve() {
    if (!b_) return fail("solve: out of memory", SIM3OPT_ERR_ARG);
    if (n_frames_ < 1) return fail("solve: no frames set", SIM3OPT_ERR_STATE);
    if (pairs_.empty()) return fail("solve: no pair added", SIM3OPT_ERR_STATE);
    if (!have_cams_) return fail("solve: no cameras set", SIM3OPT_ERR_STATE);
    int rc = sim3opt_track_batch_set_options(b_, &opt_);
    const int32_t none = 0;  // (a batch without any match still hands arrays over)
    if (rc == SIM3OPT_OK)
      rc = sim3opt_track_batch_set_matches(b_, n_pairs(), pairs_.data(), match_ptr_.data(), query_.empty() ? &none : query_.data(),
                                           train_.empty() ? &none : train_.data(), mask_.data(), depth0_.data(),
                                           depth1_.data());
    if (rc == SIM3OPT_OK)
      rc = sim3opt_track_batch_set_cameras(b_, (int32_t)(states_.size() / 8), states_.data(), focal_, cx_, cy_);
    if (rc == SIM3OPT_OK) rc = sim3opt_track_batch_solve(b_);
    return rc >= 0 ? rc : fail(sim3opt_track_batch_last_error(b_), rc);
  }

  int n_tracks() const { return dim(3); }
  int n_kept_tracks() const { return dim(5); }
  int rounds() const { return dim(7); }

  // Every track: SIM3OPT_OK, or SIM3OPT_ERR_STATE before a solve.
  int tracks(std::vector<int32_t>& track_ptr, std::vector<int32_t>& obs_frame, std::vector<int32_t>& obs_keypoint,
             std::vector<int32_t>& status) {
    if (!b_) return fail("tracks: out of memory", SIM3OPT_ERR_ARG);
    std::vector<int32_t> p((std::size_t)n_tracks() + 1), f((std::size_t)dim(4) + 1), k(f.size()), s(p.size());
    const int rc = sim3opt_track_batch_get_tracks(b_, p.data(), f.data(), k.data(), s.data(), nullptr);
    if (rc != SIM3OPT_OK) return fail(sim3opt_track_batch_last_error(b_), rc);
    f.pop_back(); k.pop_back(); s.pop_back();
    track_ptr.swap(p); obs_frame.swap(f); obs_keypoint.swap(k); status.swap(s);
    return rc;
  }

  // Appends the status-0 tracks behind a map: their points behind `points` (3 each), their rows behind obs_cam /
  // obs_point / obs_uv (2 each), obs_point counting on from the map's points.  cams (7 each) is what the rows index:
  // one camera per frame.  SIM3OPT_OK, or a negative SIM3OPT_ERR_* with the arrays as they were.
  int append_to(const std::vector<double>& cams, std::vector<double>& points, std::vector<int32_t>& obs_cam,
                std::vector<int32_t>& obs_point, std::vector<double>& obs_uv) {
    if (!b_) return fail("append_to: out of memory", SIM3OPT_ERR_ARG);
    if (cams.size() != 7 * (std::size_t)n_frames_) return fail("append_to: one camera per frame", SIM3OPT_ERR_ARG);
    if (points.size() % 3 || obs_cam.size() != obs_point.size() || obs_uv.size() != 2 * obs_cam.size())
      return fail("append_to: the map's arrays differ in length", SIM3OPT_ERR_ARG);
    const std::size_t nk = (std::size_t)n_kept_tracks(), no = (std::size_t)dim(6);
    std::vector<double> p(3 * nk + 1), uv(2 * no + 1);
    std::vector<int32_t> oc(no + 1), op(no + 1);
    const int rc = sim3opt_track_batch_get_ba(b_, (int32_t)(points.size() / 3), p.data(), oc.data(), op.data(), uv.data());
    if (rc != SIM3OPT_OK) return fail(sim3opt_track_batch_last_error(b_), rc);
    points.insert(points.end(), p.begin(), p.end() - 1);
    obs_cam.insert(obs_cam.end(), oc.begin(), oc.end() - 1);
    obs_point.insert(obs_point.end(), op.begin(), op.end() - 1);
    obs_uv.insert(obs_uv.end(), uv.begin(), uv.end() - 1);
    return rc;
  }

 private:
  int fail(const std::string& why, int rc) { err_ = why; return rc; }
  int dim(int which) const {
    int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (b_) (void)sim3opt_track_batch_dims(b_, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], nullptr);
    return v[which];
  }

  sim3opt_track_batch* b_;
  sim3opt_track_batch_options opt_;
  std::string err_;
  int n_frames_ = 0;
  bool have_cams_ = false;
  std::vector<int32_t> pairs_, match_ptr_, query_, train_;
  std::vector<uint8_t> mask_;
  std::vector<double> depth0_, depth1_, states_;
  double focal_ = 0, cx_ = 0, cy_ = 0;
};

}  // namespace sim3opt_shim
