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
void dev_cache_release();  // gives every cached block back to the driver
// {blocks, bytes (as rounded)} dev_malloc has handed out and not got back, process-wide (sim3opt_device_memory_in_use)
void dev_in_use(int64_t out[2]);
// live handles of the process, of every type handle_device.hpp's handle_create makes (delta = +1 / -1; returns the new
// count): the cache is released when the last one goes (sim3opt_release_device_cache does it on request)
int handle_count(int delta);

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
    return dev_malloc((void**)&p_, sizeof(T) * count);
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
    const hipError_t e = dev_malloc(&q, sizeof(T) * std::max<size_t>(count, 1));
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
