// frames.hip -- the frame store: one owner for kp_ptr / kp / desc of a sequence on one device, filled once (from host
// arrays, by the extractor on the device, or by the compaction run as an operator) and read in place by the vocabulary
// trainer, place recognition and the matcher.  include/sim3opt.h ("device-resident frame store") says what a snapshot
// is and why a fill synchronises; DESIGN.md, section 5c.  frames_host.hpp holds the checks, the snapshot and the serial
// restatement of the compaction's offsets.
//
//   k_frames_count         a workgroup per image walks the image's slots in tiles of COMPACT_TILE: the kept slots
//                          before every tile (the carry of the scan) and the image's kept count
//   k_frames_scan_images   exclusive offsets of the images: kp_ptr of the fill
//   k_frames_move          a workgroup per tile: a scan of the predicate over its lanes places the kept slots, then 16
//                          lanes move a 256-byte row with one 16-byte load and store each, four rows a wavefront, in
//                          output order: consecutive rows of a wavefront's store are consecutive in memory
//   k_frames_distinct      does any descriptor differ from the first?  (what the trainer's set_frames asks on the host)
// No atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "frames_device.hpp"
#include "handle_device.hpp"

namespace sim3opt_fstore {

static_assert(COMPACT_TILE == 256 && ROW_LANES * sizeof(float4) == DESC * sizeof(float), "a row is 16 lanes of 16 bytes");
constexpr int ROWS_PER_STEP = COMPACT_TILE / ROW_LANES;

// exclusive prefix sum of v over the workgroup's lanes; total: the sum.  s: COMPACT_TILE ints.
__device__ inline int32_t tile_excl_scan(int32_t v, int32_t* s, int32_t& total) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < COMPACT_TILE; off <<= 1) {
    const int32_t x = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += x;
    __syncthreads();
  }
  const int32_t incl = s[tid];
  total = s[COMPACT_TILE - 1];
  __syncthreads();  // s may be written again
  return incl - v;
}

__global__ __launch_bounds__(COMPACT_TILE) void k_frames_count(const int32_t* cand_ptr, const int32_t* state, int32_t tiles,
                                                               int32_t* tile_base, int32_t* img_count) {
  const int32_t image = blockIdx.x, lo = cand_ptr[image], hi = cand_ptr[image + 1];
  int32_t run = 0, t = 0;
  for (int32_t first = lo; first < hi; first += COMPACT_TILE, ++t) {  // (uniform)
    const int32_t s = first + (int32_t)threadIdx.x;
    const int kept = s < hi && state[s] == KEPT;
    const int n = __syncthreads_count(kept);
    if (threadIdx.x == 0) tile_base[(size_t)image * (size_t)tiles + (size_t)t] = run;
    run += n;
  }
  if (threadIdx.x == 0) img_count[image] = run;
}

__global__ __launch_bounds__(COMPACT_TILE) void k_frames_scan_images(const int32_t* img_count, int32_t n, int32_t base,
                                                                     int32_t* kp_ptr) {
  __shared__ int32_t sc[COMPACT_TILE];
  int32_t run = base;
  for (int32_t i0 = 0; i0 < n; i0 += COMPACT_TILE) {
    const int32_t i = i0 + (int32_t)threadIdx.x;
    const int32_t v = i < n ? img_count[i] : 0;
    int32_t total;
    const int32_t excl = tile_excl_scan(v, sc, total);
    if (i < n) kp_ptr[i] = run + excl;
    run += total;
  }
  if (threadIdx.x == 0) kp_ptr[n] = run;
}

__global__ __launch_bounds__(COMPACT_TILE) void k_frames_move(const int32_t* cand_ptr, const int32_t* state, int32_t tiles,
                                                              const int32_t* tile_base, const int32_t* kp_ptr,
                                                              const float* slot_kp, const float* slot_desc, float* out_kp,
                                                              float* out_desc) {
  __shared__ int32_t sc[COMPACT_TILE];
  __shared__ int32_t src[COMPACT_TILE];
  const int32_t image = blockIdx.y, lo = cand_ptr[image], hi = cand_ptr[image + 1], tid = threadIdx.x;
  const int32_t first = lo + (int32_t)blockIdx.x * COMPACT_TILE;
  if (first >= hi) return;  // (the whole workgroup)
  const int32_t s = first + tid;
  const int32_t kept = s < hi && state[s] == KEPT;
  int32_t total;
  const int32_t excl = tile_excl_scan(kept, sc, total);
  if (kept) src[excl] = s;
  __syncthreads();
  const size_t row0 = (size_t)kp_ptr[image] + (size_t)tile_base[(size_t)image * (size_t)tiles + (size_t)blockIdx.x];
  if (tid < total)
    reinterpret_cast<float2*>(out_kp)[row0 + (size_t)tid] = reinterpret_cast<const float2*>(slot_kp)[(size_t)src[tid]];
  const int32_t q = tid % ROW_LANES;
  for (int32_t r = tid / ROW_LANES; r < total; r += ROWS_PER_STEP) {
    const float4 v = reinterpret_cast<const float4*>(slot_desc)[(size_t)src[r] * ROW_LANES + (size_t)q];
    reinterpret_cast<float4*>(out_desc)[(row0 + (size_t)r) * ROW_LANES + (size_t)q] = v;
  }
}

// flag[0] = 1 when a descriptor differs, as numbers, from the first (every writer writes the same value)
__global__ __launch_bounds__(COMPACT_TILE) void k_frames_distinct(const float* desc, size_t n_rows, int32_t* flag) {
  const size_t e = (size_t)blockIdx.x * COMPACT_TILE + threadIdx.x;
  if (e >= n_rows * ROW_LANES) return;
  const float4 a = reinterpret_cast<const float4*>(desc)[e % ROW_LANES], b = reinterpret_cast<const float4*>(desc)[e];
  if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) flag[0] = 1;
}

int compact_enqueue(const CompactArgs& A, sim3opt::DevArena& work, hipStream_t stream, std::string& err) {
  int32_t *tile_base = nullptr, *img_count = nullptr;
  HIPCHK(work.raw(tile_base, (size_t)A.n_images * (size_t)A.tiles));
  HIPCHK(work.raw(img_count, (size_t)A.n_images));
  hipLaunchKernelGGL(k_frames_count, dim3((unsigned)A.n_images), dim3(COMPACT_TILE), 0, stream, A.cand_ptr, A.state, A.tiles,
                     tile_base, img_count);
  hipLaunchKernelGGL(k_frames_scan_images, dim3(1), dim3(COMPACT_TILE), 0, stream, img_count, A.n_images, A.base, A.kp_ptr_out);
  if (A.tiles)
    hipLaunchKernelGGL(k_frames_move, dim3((unsigned)A.tiles, (unsigned)A.n_images), dim3(COMPACT_TILE), 0, stream, A.cand_ptr,
                       A.state, A.tiles, tile_base, A.kp_ptr_out, A.slot_kp, A.slot_desc, A.out_kp, A.out_desc);
  HIPCHK(hipGetLastError());
  return SIM3OPT_OK;
}

int seal_snapshot(Snapshot& snap, hipStream_t stream, std::string& err) {
  const size_t n = snap.N();
  sim3opt::DevBuf<int32_t> flag;
  int32_t h = 0;
  if (n > 1) {
    HIPCHK(flag.alloc(1));
    HIPCHK(hipMemsetAsync(flag.get(), 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_frames_distinct, dim3((unsigned)((n * ROW_LANES + COMPACT_TILE - 1) / COMPACT_TILE)), dim3(COMPACT_TILE),
                       0, stream, snap.d_desc, n, flag.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&h, flag.get(), sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  }
  HIPCHK(hipStreamSynchronize(stream));
  snap.distinct = h != 0;
  return SIM3OPT_OK;
}

int resolve_device(int32_t want_device, int& device, std::string& err) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    err = "no usable HIP device (libsim3opt has no CPU fallback)";
    return SIM3OPT_ERR_NO_DEVICE;
  }
  if (want_device >= 0) { device = want_device; return SIM3OPT_OK; }
  HIPCHK(hipGetDevice(&device));
  return SIM3OPT_OK;
}

int new_snapshot(const std::vector<int32_t>& kp_ptr, std::shared_ptr<Snapshot>& out, std::string& err) {
  auto s = std::make_shared<Snapshot>();
  s->free_block = sim3opt::dev_free;
  HIPCHK(hipGetDevice(&s->device));
  s->kp_ptr = kp_ptr;
  const size_t n = s->N();
  HIPCHK(sim3opt::dev_malloc_of((void**)&s->d_kp_ptr, sizeof(int32_t) * kp_ptr.size(), false));
  HIPCHK(sim3opt::dev_malloc_of((void**)&s->d_kp, sizeof(float) * 2 * std::max<size_t>(n, 1), true));
  HIPCHK(sim3opt::dev_malloc_of((void**)&s->d_desc, sizeof(float) * DESC * std::max<size_t>(n, 1), true));
  HIPCHK(hipMemcpy(s->d_kp_ptr, s->kp_ptr.data(), sizeof(int32_t) * kp_ptr.size(), hipMemcpyHostToDevice));
  out = std::move(s);
  return SIM3OPT_OK;
}

struct Store : sim3opt::BatchHandle {
  sim3opt_frames_options opt;
  SnapshotRef snap;
  std::shared_ptr<Snapshot> filling;  // the snapshot of a fill under way: let go only once the stream has run dry
  sim3opt::DevArena work;

  ~Store() { release(); }
  void release() { close_stream(work); }

  // the store's device made current, its stream open
  int ensure_device() {
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    if (!stream)
      if (int rc = open_stream()) return rc;
    return SIM3OPT_OK;
  }

  int set(int32_t n_frames, const int32_t* kp_ptr, const float* kp, const float* desc) {
    const int rc = set_body(n_frames, kp_ptr, kp, desc);
    wait();
    filling.reset();
    return rc;
  }

  int set_body(int32_t n_frames, const int32_t* kp_ptr, const float* kp, const float* desc) {
    err.clear();
    const std::string e = validate_frames(n_frames, kp_ptr, kp, desc);
    if (!e.empty()) { err = "frames_set: " + e; return SIM3OPT_ERR_ARG; }
    if (int rc = ensure_device()) return rc;
    std::shared_ptr<Snapshot>& s = filling;
    if (int rc = new_snapshot(std::vector<int32_t>(kp_ptr, kp_ptr + n_frames + 1), s, err)) return rc;
    const size_t n = s->N();
    if (n) {
      HIPCHK(hipMemcpyAsync(s->d_kp, kp, sizeof(float) * 2 * n, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(s->d_desc, desc, sizeof(float) * DESC * n, hipMemcpyHostToDevice, stream));
    }
    if (int rc = seal_snapshot(*s, stream, err)) return rc;
    snap = std::move(s);
    return SIM3OPT_OK;
  }

  int get(int32_t* kp_ptr, float* kp, float* desc) {
    err.clear();
    if (!snap) { err = "frames_get: the store is not filled"; return SIM3OPT_ERR_STATE; }
    const size_t n = snap->N();
    if (kp_ptr) std::memcpy(kp_ptr, snap->kp_ptr.data(), sizeof(int32_t) * snap->kp_ptr.size());
    if (!n || (!kp && !desc)) return SIM3OPT_OK;
    HIPCHK(hipSetDevice(snap->device));
    if (kp) HIPCHK(hipMemcpy(kp, snap->d_kp, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
    if (desc) HIPCHK(hipMemcpy(desc, snap->d_desc, sizeof(float) * DESC * n, hipMemcpyDeviceToHost));
    return SIM3OPT_OK;
  }

  int debug_compact(int32_t n_images, const int32_t* cand_ptr, const int32_t* state, const float* slot_kp,
                    const float* slot_desc) {
    const int rc = compact_body(n_images, cand_ptr, state, slot_kp, slot_desc);
    wait();
    work.release();
    filling.reset();
    return rc;
  }

  int compact_body(int32_t n_images, const int32_t* cand_ptr, const int32_t* state, const float* slot_kp,
                   const float* slot_desc) {
    err.clear();
    const std::string e = validate_slots(n_images, cand_ptr, state, slot_kp, slot_desc);
    if (!e.empty()) { err = "frames_debug_compact: " + e; return SIM3OPT_ERR_ARG; }
    if (int rc = ensure_device()) return rc;
    // the host's restatement sizes the blocks; kp_ptr itself is what the kernels emit
    std::vector<int32_t> want, src;
    compact_offsets(n_images, cand_ptr, state, 0, want, src);
    const size_t ns = (size_t)cand_ptr[n_images];
    std::shared_ptr<Snapshot>& s = filling;
    if (int rc = new_snapshot(want, s, err)) return rc;
    CompactArgs A{};
    A.n_images = n_images; A.tiles = max_tiles(n_images, cand_ptr); A.base = 0;
    int32_t *d_cand_ptr = nullptr, *d_state = nullptr, *d_out_ptr = nullptr;
    float *d_kp = nullptr, *d_desc = nullptr;
    HIPCHK(work.raw(d_cand_ptr, (size_t)n_images + 1));
    HIPCHK(work.raw(d_state, ns));
    HIPCHK(work.raw(d_kp, 2 * ns));
    HIPCHK(work.raw(d_desc, ns * DESC));
    HIPCHK(work.raw(d_out_ptr, (size_t)n_images + 1));
    HIPCHK(hipMemcpyAsync(d_cand_ptr, cand_ptr, sizeof(int32_t) * ((size_t)n_images + 1), hipMemcpyHostToDevice, stream));
    if (ns) {
      HIPCHK(hipMemcpyAsync(d_state, state, sizeof(int32_t) * ns, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_kp, slot_kp, sizeof(float) * 2 * ns, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_desc, slot_desc, sizeof(float) * DESC * ns, hipMemcpyHostToDevice, stream));
    }
    A.cand_ptr = d_cand_ptr; A.state = d_state; A.slot_kp = d_kp; A.slot_desc = d_desc;
    A.kp_ptr_out = d_out_ptr; A.out_kp = s->d_kp; A.out_desc = s->d_desc;
    if (int rc = compact_enqueue(A, work, stream, err)) return rc;
    std::vector<int32_t> got;
    HIPCHK(sim3opt::read_back(got, d_out_ptr, (size_t)n_images + 1, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (got.back() != want.back()) { err = "frames_debug_compact: internal error (the kept counts)"; return SIM3OPT_ERR_HIP; }
    s->kp_ptr = got;
    HIPCHK(hipMemcpyAsync(s->d_kp_ptr, s->kp_ptr.data(), sizeof(int32_t) * got.size(), hipMemcpyHostToDevice, stream));
    if (int rc = seal_snapshot(*s, stream, err)) return rc;
    snap = std::move(s);
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_fstore

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "device-resident frame store")
// ------------------------------------------------------------------------------------------
struct sim3opt_frames : sim3opt_fstore::Store {};

namespace sim3opt_fstore {

int take_snapshot(const sim3opt_frames* store, const char* who, int32_t want_device, SnapshotRef& out, std::string& err) {
  if (!store) { err = std::string(who) + ": NULL store"; return SIM3OPT_ERR_ARG; }
  if (!store->snap) { err = std::string(who) + ": the store is not filled"; return SIM3OPT_ERR_STATE; }
  if (int rc = check_snapshot_device(*store->snap, who, want_device, err)) return rc;
  out = store->snap;
  return SIM3OPT_OK;
}

int check_snapshot_device(const Snapshot& snap, const char* who, int32_t want_device, std::string& err) {
  int device = -1;
  std::string e;
  if (int rc = resolve_device(want_device, device, e)) { err = std::string(who) + ": " + e; return rc; }
  if (device != snap.device) {
    err = std::string(who) + ": the store's frames are on device " + std::to_string(snap.device) +
          ", the handle's options resolve to device " + std::to_string(device);
    return SIM3OPT_ERR_ARG;
  }
  return SIM3OPT_OK;
}

int check_fill_device(const sim3opt_frames* store, const char* who, int device, std::string& err) {
  if (!store) { err = std::string(who) + ": NULL store"; return SIM3OPT_ERR_ARG; }
  if (store->opt.device >= 0 && store->opt.device != device) {
    err = std::string(who) + ": the store's options name device " + std::to_string(store->opt.device) +
          ", the handle runs on device " + std::to_string(device);
    return SIM3OPT_ERR_ARG;
  }
  return SIM3OPT_OK;
}

void adopt_snapshot(sim3opt_frames* store, std::shared_ptr<Snapshot> snap) { store->snap = std::move(snap); }

}  // namespace sim3opt_fstore

extern "C" {

void sim3opt_frames_options_default(sim3opt_frames_options* o) {
  if (o) o->device = -1;
}

sim3opt_frames* sim3opt_frames_create(void) {
  return sim3opt::handle_create<sim3opt_frames>(sim3opt_frames_options_default);
}

void sim3opt_frames_destroy(sim3opt_frames* s) { sim3opt::handle_destroy(s); }

const char* sim3opt_frames_last_error(const sim3opt_frames* s) { return s ? s->err.c_str() : "null store"; }

int sim3opt_frames_set_options(sim3opt_frames* s, const sim3opt_frames_options* o) {
  if (!s || !o) return SIM3OPT_ERR_ARG;
  if (o->device < -1) { s->err = "frames_set_options: device below -1"; return SIM3OPT_ERR_ARG; }
  if (o->device != s->opt.device) {  // the device is chosen at the next fill
    s->release();
    s->snap.reset();
  }
  s->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_frames_set(sim3opt_frames* s, int32_t n_frames, const int32_t* kp_ptr, const float* kp, const float* desc) {
  if (!s) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(s, "frames_set", sim3opt::NO_MEMORY, [&] { return s->set(n_frames, kp_ptr, kp, desc); });
}

int sim3opt_frames_get_dims(const sim3opt_frames* s, int32_t* n_frames, int32_t* total_keypoints, int32_t* device,
                            int64_t* desc_bytes, int32_t tiles[2]) {
  if (!s) return SIM3OPT_ERR_ARG;
  const sim3opt_fstore::Snapshot* p = s->snap.get();
  if (n_frames) *n_frames = p ? p->n_frames() : 0;
  if (total_keypoints) *total_keypoints = p ? (int32_t)p->N() : 0;
  if (device) *device = p ? p->device : -1;
  if (desc_bytes) *desc_bytes = p ? (int64_t)(sizeof(float) * sim3opt_fstore::DESC * p->N()) : 0;
  if (tiles) { tiles[0] = sim3opt_fstore::COMPACT_TILE; tiles[1] = sim3opt_fstore::ROW_LANES; }
  return SIM3OPT_OK;
}

int sim3opt_frames_get(sim3opt_frames* s, int32_t* kp_ptr, float* kp, float* desc) {
  if (!s) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(s, "frames_get", sim3opt::NO_MEMORY, [&] { return s->get(kp_ptr, kp, desc); });
}

int sim3opt_frames_debug_compact(sim3opt_frames* s, int32_t n_images, const int32_t* cand_ptr, const int32_t* state,
                                 const float* slot_kp, const float* slot_desc) {
  if (!s) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(s, "frames_debug_compact", sim3opt::NO_MEMORY,
                          [&] { return s->debug_compact(n_images, cand_ptr, state, slot_kp, slot_desc); });
}

}  // extern "C"
