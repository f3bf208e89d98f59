// frames_host.hpp -- the host side of the frame store (frames.hip; include/sim3opt.h, "device-resident frame store"):
// the checks of the arrays a caller hands over, the snapshot the store and its consumers share, and the serial
// restatement of the ordered compaction's offsets.  Plain C++ with no HIP in it, so tests/cxx/frames_host_driver.cpp
// runs it under the host sanitizers against a stub allocator.  DESIGN.md, section 5c.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "handle_host.hpp"

struct sim3opt_frames;

namespace sim3opt_fstore {

constexpr int DESC = 64;            // floats of a descriptor: a row of 256 bytes
constexpr int COMPACT_TILE = 256;   // slots a workgroup of the compaction scans at a time
constexpr int ROW_LANES = 16;       // lanes that move one row, 16 bytes each
constexpr int32_t KEPT = 2;         // the slot state the compaction keeps (surf_batch.hip: described)

// What sim3opt_match_batch_set_frames, sim3opt_place_batch_set_frames and sim3opt_vocabulary_set_frames ask alike of
// kp_ptr / kp / desc, in their words.  "" or what is wrong.
inline std::string validate_frames(int32_t n_frames, const int32_t* kp_ptr, const float* kp, const float* desc) {
  if (n_frames < 1) return "n_frames < 1";
  if (!kp_ptr || !kp || !desc) return "a NULL array";
  const std::string e = sim3opt::check_frame_ptr("kp_ptr", n_frames, kp_ptr);
  if (!e.empty()) return e;
  const size_t nk = (size_t)kp_ptr[n_frames];
  if (nk > (size_t)INT32_MAX / DESC) return "too many keypoints";
  if (!sim3opt::all_finite(kp, 2 * nk)) return "a non-finite keypoint";
  if (!sim3opt::all_finite(desc, (size_t)DESC * nk)) return "a non-finite descriptor";
  return "";
}

// the slot arrays sim3opt_frames_debug_compact takes: cand_ptr as a frame ptr, states of 0 .. 3, finite rows
inline std::string validate_slots(int32_t n_images, const int32_t* cand_ptr, const int32_t* state, const float* slot_kp,
                                  const float* slot_desc) {
  if (n_images < 1) return "n_images < 1";
  if (!cand_ptr || !state || !slot_kp || !slot_desc) return "a NULL array";
  const std::string e = sim3opt::check_frame_ptr("cand_ptr", n_images, cand_ptr);
  if (!e.empty()) return e;
  const size_t ns = (size_t)cand_ptr[n_images];
  if (ns > (size_t)INT32_MAX / DESC) return "too many slots";
  for (size_t s = 0; s < ns; ++s)
    if (state[s] < 0 || state[s] > 3) return "slot " + std::to_string(s) + ": no such state";
  if (!sim3opt::all_finite(slot_kp, 2 * ns)) return "a non-finite keypoint";
  if (!sim3opt::all_finite(slot_desc, (size_t)DESC * ns)) return "a non-finite descriptor";
  return "";
}

// "" when `more` rows fit behind `have` rows under the int32 offsets of kp_ptr and of the descriptor floats
inline std::string check_total(size_t have, size_t more) {
  if (have + more > (size_t)INT32_MAX / DESC) return "more keypoints than an int32 offset counts";
  return "";
}

// The compaction restated serially: kp_ptr (n_images + 1, starting at `base`) and, per kept row in output order, the
// slot it comes from.  The kernels write row base + r from slot src[r].
inline void compact_offsets(int32_t n_images, const int32_t* cand_ptr, const int32_t* state, int32_t base,
                            std::vector<int32_t>& kp_ptr, std::vector<int32_t>& src) {
  kp_ptr.assign(1, base);
  src.clear();
  for (int32_t i = 0; i < n_images; ++i) {
    for (int32_t s = cand_ptr[i]; s < cand_ptr[i + 1]; ++s)
      if (state[s] == KEPT) src.push_back(s);
    kp_ptr.push_back(base + (int32_t)src.size());
  }
}

// the tiles of the longest segment: the x extent of the compaction's grids
inline int32_t max_tiles(int32_t n_images, const int32_t* cand_ptr) {
  int32_t m = 0;
  for (int32_t i = 0; i < n_images; ++i) m = cand_ptr[i + 1] - cand_ptr[i] > m ? cand_ptr[i + 1] - cand_ptr[i] : m;
  return (m + COMPACT_TILE - 1) / COMPACT_TILE;
}

// The frames of a sequence on one device, immutable once filled.  The store and every consumer that took it hold a
// SnapshotRef; the blocks go back through `free_block` (dev_free in the library) when the last holder lets go.
struct Snapshot {
  int device = -1;
  std::vector<int32_t> kp_ptr;  // the host mirror the consumers plan on
  int32_t* d_kp_ptr = nullptr;
  float* d_kp = nullptr;
  float* d_desc = nullptr;
  bool distinct = false;        // two descriptors differ as numbers (what the vocabulary trainer asks for)
  void (*free_block)(void*) = nullptr;

  Snapshot() = default;
  Snapshot(const Snapshot&) = delete;
  Snapshot& operator=(const Snapshot&) = delete;
  ~Snapshot() {
    if (!free_block) return;
    free_block(d_desc); free_block(d_kp); free_block(d_kp_ptr);
  }
  int32_t n_frames() const { return (int32_t)kp_ptr.size() - 1; }
  size_t N() const { return (size_t)kp_ptr.back(); }
};
using SnapshotRef = std::shared_ptr<const Snapshot>;

// ---- what frames.hip gives the other translation units of the library (not the C-ABI)
// The store's current snapshot for a consumer `who` whose options.device is `want_device` (-1: the current one).
// SIM3OPT_OK and `out`, or the refusal's code with its message in `err`; `out` is left as it was.
int take_snapshot(const sim3opt_frames* store, const char* who, int32_t want_device, SnapshotRef& out, std::string& err);
// SIM3OPT_OK when a handle `who` whose options.device is `want_device` works on the snapshot's device, else the refusal
int check_snapshot_device(const Snapshot& snap, const char* who, int32_t want_device, std::string& err);
// May a filler `who` that runs on `device` (current) fill the store?  The store's options.device is -1 or that device.
int check_fill_device(const sim3opt_frames* store, const char* who, int device, std::string& err);
// A snapshot for kp_ptr with its blocks allocated on the current device (kp_ptr uploaded, kp and desc not written), for
// a filler that completes it on its own stream and hands it over with adopt_snapshot once that stream is synchronised.
int new_snapshot(const std::vector<int32_t>& kp_ptr, std::shared_ptr<Snapshot>& out, std::string& err);
void adopt_snapshot(sim3opt_frames* store, std::shared_ptr<Snapshot> snap);
// the current device where a consumer's options say -1 (SIM3OPT_ERR_NO_DEVICE without one)
int resolve_device(int32_t want_device, int& device, std::string& err);

}  // namespace sim3opt_fstore
