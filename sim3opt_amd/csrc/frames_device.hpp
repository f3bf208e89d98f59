// frames_device.hpp -- what frames.hip gives a filler inside the library that works on a stream of its own
// (surf_batch.hip): the ordered compaction and the last step of a fill.  frames_host.hpp holds the rest.
#pragma once

#include "devmem.hpp"
#include "frames_host.hpp"

namespace sim3opt_fstore {

struct CompactArgs {  // every pointer is the device's
  int32_t n_images, tiles;          // tiles: max_tiles() of the segments
  const int32_t *cand_ptr, *state;  // n_images + 1; per slot
  const float *slot_kp, *slot_desc;
  int32_t base;                     // kp_ptr_out[0]
  int32_t* kp_ptr_out;              // n_images + 1
  float *out_kp, *out_desc;         // row 0 of the output: row kp_ptr_out[i] + r receives the r-th kept slot of image i
};

// Enqueues the compaction on `stream`; its work blocks come from `work`, which the caller releases after it has
// synchronised.  The output has room for every row the predicate keeps (the caller's bound: the number of slots).
int compact_enqueue(const CompactArgs& A, sim3opt::DevArena& work, hipStream_t stream, std::string& err);
// The last step of a fill: whether two descriptors differ, read from the device; synchronises `stream`, so the
// snapshot's blocks are complete when it returns.
int seal_snapshot(Snapshot& snap, hipStream_t stream, std::string& err);

}  // namespace sim3opt_fstore
