// handle_host_driver.cpp -- the host half every C handle shares (csrc/handle_host.hpp: all_finite, the two ragged-pointer
// checks, the guard of the C boundary) as a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer: no GPU
// and no HIP.  Arrays are heap blocks of exactly the size handed over, so that a read past an end is the sanitizer's to
// find; every message a caller can see is compared as a whole string.  match_host.hpp is included because it delegates
// its checks to the same header.
#include <cstdio>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../sim3opt_amd/csrc/handle_host.hpp"
#include "../../sim3opt_amd/csrc/match_host.hpp"

using namespace sim3opt;

static int failed = 0, checks = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    ++checks;                                                         \
    if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } \
  } while (0)

template <class T>
static void finite_cases() {
  const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
  CHECK(all_finite((const T*)nullptr, 0));  // n = 0 reads nothing
  for (size_t n : {(size_t)1, (size_t)2, (size_t)257}) {
    std::vector<T> v(n, (T)1.5);  // (exactly n elements on the heap)
    v.shrink_to_fit();
    CHECK(all_finite(v.data(), n));
    CHECK(all_finite(v.data(), 0));
    for (T bad : {nan, inf, -inf})
      for (size_t at : {(size_t)0, n - 1}) {
        std::vector<T> w(v);
        w[at] = bad;
        CHECK(!all_finite(w.data(), n));
        CHECK(all_finite(w.data() + (at == 0 ? 1 : 0), n - 1));  // ... and only that entry is to blame
      }
  }
  std::vector<T> big(3, std::numeric_limits<T>::max());
  big[1] = std::numeric_limits<T>::lowest(); big[2] = std::numeric_limits<T>::denorm_min();
  CHECK(all_finite(big.data(), 3));
}

struct Handle {
  std::string err;
};

int main() {
  finite_cases<float>();
  finite_cases<double>();

  // ---- point_ptr of the problem batches: starts at 0, every problem owns a point
  using P = std::vector<int32_t>;
  const auto point = [](const P& p) { return check_point_ptr((int32_t)p.size() - 1, p.data()); };
  CHECK(point({0, 1}) == "");
  CHECK(point({0, 4, 5, 90}) == "");
  CHECK(point({1, 4}) == "point_ptr[0] must be 0");
  CHECK(point({-1, 4}) == "point_ptr[0] must be 0");
  CHECK(point({0, 0}) == "problem 0 has no point");
  CHECK(point({0, 0, 3, 5}) == "problem 0 has no point");
  CHECK(point({0, 3, 5, 5}) == "problem 2 has no point");
  CHECK(point({0, -1}) == "problem 0: point_ptr is not monotone");
  CHECK(point({0, -2, 3, 5}) == "problem 0: point_ptr is not monotone");
  CHECK(point({0, 3, 5, 4}) == "problem 2: point_ptr is not monotone");
  CHECK(point({0, 3, 3, 2}) == "problem 1 has no point");  // (the first offence is the one named)
  {
    P many(12, 0);
    for (int i = 0; i < 12; ++i) many[i] = 2 * i;
    many[11] = many[10] - 7;
    CHECK(point(many) == "problem 10: point_ptr is not monotone");
  }

  // ---- the per-frame pointers of the matcher: start at 0, never decrease, a frame may own nothing
  const auto frame = [](const char* name, const P& p) { return check_frame_ptr(name, (int32_t)p.size() - 1, p.data()); };
  CHECK(frame("kp_ptr", {0, 0}) == "");
  CHECK(frame("kp_ptr", {0, 3, 3, 9}) == "");
  CHECK(frame("kp_ptr", {2, 3}) == "kp_ptr[0] must be 0");
  CHECK(frame("obs_ptr", {-1, 3}) == "obs_ptr[0] must be 0");
  CHECK(frame("kp_ptr", {0, -1}) == "kp_ptr is not monotone at frame 0");
  CHECK(frame("obs_ptr", {0, -1, 4, 8}) == "obs_ptr is not monotone at frame 0");
  CHECK(frame("obs_ptr", {0, 4, 8, 7}) == "obs_ptr is not monotone at frame 2");
  CHECK(frame("kp_ptr", {0, 4, 3, 2}) == "kp_ptr is not monotone at frame 1");
  {  // ... as validate_frames of match_host.hpp passes them on
    const P kp_ptr{0, 2, 2}, bad{0, 2, 1};
    const std::vector<float> kp(4, 1.f), desc(2 * sim3opt_match::DESC, 0.f), ouv(4, 1.f), od(2, 1.f);
    const auto vf = [&](const P& a, const P& b) {
      return sim3opt_match::validate_frames(2, a.data(), b.data(), kp.data(), desc.data(), ouv.data(), od.data(), 700, 600,
                                            180, 1241, 376);
    };
    CHECK(vf(kp_ptr, kp_ptr) == "");
    CHECK(vf(bad, kp_ptr) == "kp_ptr is not monotone at frame 1");
    CHECK(vf(kp_ptr, bad) == "obs_ptr is not monotone at frame 1");
    CHECK(vf(kp_ptr, P{1, 2, 2}) == "obs_ptr[0] must be 0");
  }

  // ---- the guard of the C boundary
  Handle h;
  h.err = "untouched";
  CHECK(guarded(&h, "x_solve", NO_MEMORY, [] { return 7; }) == 7 && h.err == "untouched");
  CHECK(guarded(&h, "x_solve", NO_MEMORY, [] { return (int)SIM3OPT_ERR_STATE; }) == SIM3OPT_ERR_STATE && h.err == "untouched");
  CHECK(guarded(&h, "x_solve", NO_MEMORY, [&]() -> int { h.err = "x_solve: refused"; return SIM3OPT_ERR_ARG; }) == SIM3OPT_ERR_ARG &&
        h.err == "x_solve: refused");
  CHECK(guarded(&h, "x_set_problems", NO_MEMORY, []() -> int { throw std::bad_alloc(); }) == SIM3OPT_ERR_ARG);
  CHECK(h.err == "x_set_problems: out of host memory");
  CHECK(guarded(&h, "x_solve", NO_MEMORY_OR_INTERNAL, []() -> int { throw 3; }) == SIM3OPT_ERR_ARG);
  CHECK(h.err == "x_solve: out of host memory or internal error");
  CHECK(guarded(&h, "x_debug", NO_MEMORY, []() -> int { throw 3; }) == SIM3OPT_ERR_ARG);
  CHECK(h.err == "x_debug: out of host memory");
  CHECK(guarded(&h, "x_optimize", NO_MEMORY_OR_INTERNAL, []() -> int { throw std::bad_alloc(); }) == SIM3OPT_ERR_ARG);
  CHECK(h.err == "x_optimize: out of host memory or internal error");
  {  // what the body built before it threw is unwound (the leak checker looks)
    const int rc = guarded(&h, "x_set_frames", NO_MEMORY, []() -> int {
      std::vector<double> held(1000, 1.0);
      if (held[999] > 0) throw std::bad_alloc();
      return 0;
    });
    CHECK(rc == SIM3OPT_ERR_ARG && h.err == "x_set_frames: out of host memory");
  }

  std::printf("%d checks, %d failed\n", checks, failed);
  if (failed) return 1;
  std::printf("handle host ok\n");
  return 0;
}
