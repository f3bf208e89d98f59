// handle_device.hpp -- the device side every C handle of the library shares, on top of devmem.hpp: the choice of the
// device, creation and destruction with the process-wide handle count, and for the batched loop-candidate stages
// (ba_batch.hip, pnp_batch.hip, match_batch.hip) the stream they own and the read-back of a solve's results.
// DESIGN.md, "Where a new batched stage plugs in".
#pragma once

#include <new>
#include <string>
#include <vector>

#include "devmem.hpp"
#include "handle_host.hpp"

namespace sim3opt {

// options.device: -1 keeps the calling thread's current device, an ordinal makes that one current
inline int select_device(int32_t device, std::string& err) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    err = "no usable HIP device (libsim3opt has no CPU fallback)";
    return SIM3OPT_ERR_NO_DEVICE;
  }
  if (device >= 0) {
    if (device >= ndev) { err = "device ordinal out of range"; return SIM3OPT_ERR_ARG; }
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
      err = std::string("hipSetDevice(opt.device): ") + hipGetErrorString(e);
      return SIM3OPT_ERR_HIP;
    }
  }
  return SIM3OPT_OK;
}

// sim3opt_*_create: the handle with its default options (NULL when there is no memory for it)
template <class H, class O>
H* handle_create(void (*defaults)(O*)) {
  H* h = new (std::nothrow) H();
  if (h) {
    defaults(&h->opt);
    handle_count(+1);
  }
  return h;
}

// sim3opt_*_destroy: the device cache goes with the last handle of the process
template <class H>
void handle_destroy(H* h) {
  if (!h) return;
  delete h;
  if (handle_count(-1) == 0) dev_cache_release();
}

// What the batch handles are made of besides their problems: the message of the last error, whether a solve's results
// are there, and a non-blocking stream of their own.  A handle keeps its device pointers, and what it knows of their
// contents, in one aggregate `dev`; its release() is close_stream(<its arenas>) and dev = Dev{}.
struct BatchHandle {
  std::string err;
  bool have_run = false;
  hipStream_t stream = nullptr;

  int open_stream() {
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return SIM3OPT_OK;
  }
  void wait() const {
    if (stream) (void)hipStreamSynchronize(stream);
  }
  // in this order: the stream runs dry, the arenas give their blocks back, the stream goes
  template <class... Arena>
  void close_stream(Arena&... arenas) {
    wait();
    (arenas.release(), ...);
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }
};

// Sizes h to count elements and enqueues their copy from d on `stream` (count 0: nothing).  A solve lists its arrays,
// synchronises once and swaps them into the handle.
template <class T>
hipError_t read_back(std::vector<T>& h, const T* d, size_t count, hipStream_t stream) {
  h.resize(count);
  return count ? hipMemcpyAsync(h.data(), d, sizeof(T) * count, hipMemcpyDeviceToHost, stream) : hipSuccess;
}

}  // namespace sim3opt
