// devmem.hpp -- device allocations of the engine go through a small cache: g2o allows
// initializeOptimization() again and again (the incremental configuration re-plans after every loop
// closure), and 60 hipFree + 60 hipMalloc calls were most of the 6 ms such a re-initialisation cost.
// Freed blocks of up to 64 MB are kept (1 GB in all, per process) and handed out again for requests
// of the same rounded size; everything larger goes straight to hipMalloc / hipFree.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

// Returns SIM3OPT_ERR_HIP with "<call>: <hip's message>" in the `err` of the enclosing scope: the one form of "check a
// HIP call" of the engine's units, comm.cpp and the bundle adjusters (the user includes sim3opt.h for the code).
#define HIPCHK(call)                                                        \
  do {                                                                      \
    hipError_t e_ = (call);                                                 \
    if (e_ != hipSuccess) {                                                 \
      err = std::string(#call) + ": " + hipGetErrorString(e_);              \
      return SIM3OPT_ERR_HIP;                                               \
    }                                                                       \
  } while (0)

namespace sim3opt {

hipError_t dev_malloc(void** p, size_t bytes);
void dev_free(void* p);
// The element kind of the calling thread's next dev_malloc: what the test mode below fills the block with (it reads and
// clears it; nothing else looks).  Every caller allocates through dev_malloc_of, which sets it.
inline bool& dev_next_floating() {
  static thread_local bool kind = false;
  return kind;
}
inline hipError_t dev_malloc_of(void** p, size_t bytes, bool floating) {
  dev_next_floating() = floating;
  return dev_malloc(p, bytes);
}
void dev_cache_release();  // gives every cached block back to the driver
// {blocks, bytes (as rounded)} dev_malloc has handed out and not got back, process-wide (sim3opt_device_memory_in_use)
void dev_in_use(int64_t out[2]);
// live handles of the process, of every type handle_device.hpp's handle_create makes (delta = +1 / -1; returns the new
// count): the cache is released when the last one goes (sim3opt_release_device_cache does it on request)
int handle_count(int delta);

// ---- the test mode (sim3opt_debug_device_memory; tests/test_gpu_stale_memory.py) --------------------------------------
// Off: dev_malloc and dev_free test one flag and do what they always did.  On: dev_malloc asks for
// rounded(bytes + DEBUG_TAIL), so every block ends in a tail of at least DEBUG_TAIL bytes that no owner asked for, fills
// [0, bytes) with 0xFF bytes (a quiet NaN in float and in double) where the element type is floating point and with
// 0x00 where it is not (a stale integer may be an index: a poison that could send a load outside its array is not used),
// and the tail with DEBUG_CANARY; dev_free compares the tail with the canary and counts the blocks that differ.  So a
// floating-point read before the owner's write turns the result into NaN, and a write past the requested length is
// counted.  Not covered: integer arrays, LDS, pinned host blocks, accesses outside the block.  The fill is a synchronous
// hipMemset and a synchronisation of the block's device (the engine's streams are non-blocking), so nothing may allocate
// inside a stream capture while the mode is on -- nothing does: the PCG's capture region launches kernels only.
// Blocks handed out while the mode was off are not checked, so the mode may change while handles live.
constexpr size_t DEBUG_TAIL = 256;  // rounded()'s smallest block
constexpr unsigned char DEBUG_CANARY = 0xA5, DEBUG_NAN_BYTE = 0xFF;
void dev_debug(bool on);               // switching it on resets the counters
// {blocks filled, blocks checked at free, blocks whose tail was overwritten, first overwritten offset past the requested
// size of the first such block or -1}
void dev_debug_report(int64_t out[4]);
// allocates `bytes` through dev_malloc, sets `overrun` bytes from offset `bytes` on (refused if they would leave the
// block), copies the whole block -- `*size` bytes, at most out_len -- to `out` and frees it
hipError_t dev_debug_probe(size_t bytes, bool floating, size_t overrun, unsigned char* out, size_t out_len, size_t* size);

// the arithmetic of the mode, on the host alone (tests/cxx/devmem_owners_driver.cpp runs it against a stub allocator)
inline size_t dev_rounded(size_t bytes) {  // eight steps per octave: at most 12.5 % more than asked for
  if (bytes < 256) return 256;
  size_t step = 256;
  while ((step << 4) <= bytes) step <<= 1;
  return (bytes + step - 1) / step * step;
}
inline size_t dev_debug_size(size_t bytes) { return dev_rounded(bytes + DEBUG_TAIL); }  // what the mode asks the driver for
inline size_t dev_debug_tail_offset(size_t bytes) { return bytes; }
inline size_t dev_debug_tail_length(size_t bytes) { return dev_debug_size(bytes) - bytes; }
// index of the first byte of buf[0, n) that is not `want`, or -1
inline int64_t dev_debug_first_mismatch(const unsigned char* buf, size_t n, unsigned char want) {
  for (size_t i = 0; i < n; ++i)
    if (buf[i] != want) return (int64_t)i;
  return -1;
}
// Is a block of T filled as floating point?  float and double; a struct of doubles only says so by an overload for its
// own type next to its definition (found through its namespace: sim3::Sim3, the bundle adjuster's Cam).
template <typename T>
constexpr bool dev_block_is_floating(const T*) { return std::is_floating_point<T>::value; }

// The same idea for what else an engine creates and destroys around every re-initialisation (round 3: 2.9 of
// the 4 ms a re-initialisation of KITTI-00 took were a stream, a dozen events, a pinned scalar block and twenty
// synchronous 50-us uploads of a few KB each): idle streams, events and pinned host blocks are kept per device
// and handed out again; dev_cache_release() destroys them too.
hipError_t stream_acquire(hipStream_t* s);   // a non-blocking stream
void stream_release(hipStream_t s);          // (the caller has synchronised it)
hipError_t event_acquire(hipEvent_t* e);
void event_release(hipEvent_t e);
hipError_t host_malloc(void** p, size_t bytes);  // pinned
void host_free(void* p);

// Small host -> device copies of an initialisation go through one pinned staging block and are enqueued on the
// engine's stream (the caller synchronises once, when it has enqueued them all); large ones are copied directly.
class StagedUploads {
 public:
  ~StagedUploads() { release(); }
  // copies bytes from src (pageable) to dst (device); asynchronous on `stream` when it fits the staging block
  hipError_t put(void* dst, const void* src, size_t bytes, hipStream_t stream);
  void release();  // gives the staging block back (after the caller's synchronisation)

 private:
  static constexpr size_t BLOCK = (size_t)4 << 20, MAX_ITEM = (size_t)512 << 10;
  char* base_ = nullptr;
  size_t off_ = 0;
};

// A device block that lives for one call: freed (handed back to the cache) when it goes out of scope, on every path.
// The destructor does not synchronise: the caller has waited for whatever it queued on the block, as before a dev_free.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { dev_free(p_); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { dev_free(p_); }
  hipError_t alloc(size_t count) {  // (not zeroed; an earlier block goes first)
    dev_free(p_);
    p_ = nullptr;
    return dev_malloc_of((void**)&p_, sizeof(T) * count, dev_block_is_floating((const T*)nullptr));
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
};

// Owns many device blocks until release(): the buffers of an initialisation, of the batch, of a factorisation.
// Every block has at least one element.
class DevArena {
 public:
  DevArena() = default;
  DevArena(const DevArena&) = delete;
  DevArena& operator=(const DevArena&) = delete;
  ~DevArena() { release(); }
  // a block as dev_malloc hands it out (not zeroed: the owner writes it before it reads it)
  template <typename T>
  hipError_t raw(T*& p, size_t count) {
    void* q = nullptr;
    const hipError_t e = dev_malloc_of(&q, sizeof(T) * std::max<size_t>(count, 1),
                                       dev_block_is_floating((const typename std::remove_cv<T>::type*)nullptr));
    if (e != hipSuccess) return e;
    blocks_.push_back(q);
    p = static_cast<T*>(q);
    return hipSuccess;
  }
  // ... and zeroed: by hipMemset (stream == nullptr), else by hipMemsetAsync on `stream`
  template <typename T>
  hipError_t alloc(T*& p, size_t count, hipStream_t stream) {
    const hipError_t e = raw(p, count);
    if (e != hipSuccess) return e;
    const size_t bytes = sizeof(T) * std::max<size_t>(count, 1);
    return stream ? hipMemsetAsync(p, 0, bytes, stream) : hipMemset(p, 0, bytes);
  }
  // ... and filled from h: through `staged` when given (enqueued on `stream`), else enqueued on `stream` straight from
  // h, else (no stream) by a synchronous copy
  template <typename T, typename U>
  hipError_t upload(T*& p, const std::vector<U>& h, hipStream_t stream, StagedUploads* staged) {
    U* q = nullptr;
    const hipError_t e = raw(q, h.size());
    if (e != hipSuccess) return e;
    p = q;
    if (h.empty()) return hipSuccess;
    const size_t bytes = sizeof(U) * h.size();
    if (staged) return staged->put(q, h.data(), bytes, stream);
    if (stream) return hipMemcpyAsync(q, h.data(), bytes, hipMemcpyHostToDevice, stream);
    return hipMemcpy(q, h.data(), bytes, hipMemcpyHostToDevice);
  }
  // gives every block back (the caller has synchronised); the owner's pointers are its own to forget
  void release() {
    for (void* q : blocks_) dev_free(q);
    blocks_.clear();
  }

 private:
  std::vector<void*> blocks_;
};

}  // namespace sim3opt
