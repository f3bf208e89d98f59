// handle_host.hpp -- what every C handle of the library does on the host before anything reaches the device: the checks
// of the arrays a caller hands over and the guard that keeps exceptions behind the C boundary.  Plain C++ with no HIP in
// it, so tests/cxx/handle_host_driver.cpp runs it under the host sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/sim3opt.h"

namespace sim3opt {

template <class T>
bool all_finite(const T* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// "" when point_ptr (n + 1 entries) starts at 0 and every problem owns at least one point, else what is wrong with it
inline std::string check_point_ptr(int32_t n, const int32_t* ptr) {
  if (ptr[0] != 0) return "point_ptr[0] must be 0";
  for (int32_t k = 0; k < n; ++k)
    if (ptr[k + 1] <= ptr[k])
      return "problem " + std::to_string(k) + (ptr[k + 1] == ptr[k] ? " has no point" : ": point_ptr is not monotone");
  return "";
}

// "" when the per-frame ptr (n + 1 entries) starts at 0 and never decreases: a frame may own nothing
inline std::string check_frame_ptr(const char* name, int32_t n, const int32_t* ptr) {
  if (ptr[0] != 0) return std::string(name) + "[0] must be 0";
  for (int32_t k = 0; k < n; ++k)
    if (ptr[k + 1] < ptr[k]) return std::string(name) + " is not monotone at frame " + std::to_string(k);
  return "";
}

// the two things a handle says when an exception reaches its C entry point `who`: "<who><tail>"
constexpr const char* NO_MEMORY = ": out of host memory";
constexpr const char* NO_MEMORY_OR_INTERNAL = ": out of host memory or internal error";

// Runs f() -- the body of a C entry point of handle b -- and returns what it returns; nothing crosses the C boundary.
template <class H, class F>
int guarded(H* b, const char* who, const char* tail, F&& f) {
  try {
    return f();
  } catch (...) {
    b->err = std::string(who) + tail;
    return SIM3OPT_ERR_ARG;
  }
}

}  // namespace sim3opt
