// devmem_owners_driver.cpp -- DevBuf and DevArena (csrc/devmem.hpp) against a stub allocator and stub copies: no GPU and
// no HIP runtime is linked.  Built with -fsanitize=address,undefined and run by tests/test_devmem_owners.py; every
// block must be back after each scope, on the early-return path of HIPCHK too.  Then the test mode's arithmetic
// (dev_debug_size, the tail's offset and length, dev_debug_first_mismatch) on stub blocks laid out as the mode lays them
// out: a write one byte past the request is found at offset 0, a write exactly to the end is clean, a 0-byte request
// has a 256-byte tail; and the element kinds the owners pass on.  Ends with "owners ok".
#include "../../include/sim3opt.h"
#include "../../sim3opt_amd/csrc/devmem.hpp"
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
static std::set<void*> live;
static int fail_after = -1;  // the n-th allocation from now fails
static int last_floating = -1;  // the kind the last allocation was asked with
namespace sim3opt {
hipError_t dev_malloc(void** p, size_t bytes) {
  if (fail_after == 0) { fail_after = -1; return hipErrorOutOfMemory; }
  if (fail_after > 0) --fail_after;
  last_floating = dev_next_floating() ? 1 : 0;
  *p = std::malloc(bytes ? bytes : 1);
  live.insert(*p);
  return hipSuccess;
}
void dev_free(void* p) {
  if (!p) return;
  assert(live.erase(p) == 1);
  std::free(p);
}
hipError_t StagedUploads::put(void* dst, const void* src, size_t bytes, hipStream_t) { std::memcpy(dst, src, bytes); return hipSuccess; }
void StagedUploads::release() {}
}
extern "C" {
hipError_t hipMemset(void* d, int v, size_t n) { std::memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { std::memset(d, v, n); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { std::memcpy(d, s, n); return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
}
using namespace sim3opt;
namespace owners_test {
struct Pose { double q[4], t[3], s; };  // doubles only, and says so
constexpr bool dev_block_is_floating(const Pose*) { return true; }
struct Mixed { double a; int32_t n, m; };
}
// a stub block as the test mode lays it out: `bytes` of poison, then the canary up to dev_debug_size(bytes)
static std::vector<unsigned char> guarded_block(size_t bytes, bool floating) {
  std::vector<unsigned char> b(dev_debug_size(bytes), DEBUG_CANARY);
  std::memset(b.data(), floating ? DEBUG_NAN_BYTE : 0, bytes);
  return b;
}
static int64_t tail_check(const std::vector<unsigned char>& b, size_t bytes) {
  assert(dev_debug_tail_offset(bytes) + dev_debug_tail_length(bytes) == b.size());
  return dev_debug_first_mismatch(b.data() + dev_debug_tail_offset(bytes), dev_debug_tail_length(bytes), DEBUG_CANARY);
}
static void debug_arithmetic() {
  // sizes: every block has a tail of at least DEBUG_TAIL bytes, and is a size the cache hands out anyway
  for (size_t bytes : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)4095, (size_t)4096,
                       (size_t)4097, (size_t)100000, (size_t)(64u << 20)}) {
    const size_t sz = dev_debug_size(bytes);
    assert(sz == dev_rounded(sz) && sz >= bytes + DEBUG_TAIL && dev_debug_tail_length(bytes) == sz - bytes);
    assert(sz <= bytes + DEBUG_TAIL + (bytes + DEBUG_TAIL) / 8 + 256);
    assert(dev_debug_tail_offset(bytes) == bytes);
  }
  assert(dev_debug_size(0) == 256 && dev_debug_tail_length(0) == 256 && dev_debug_tail_offset(0) == 0);
  {  // 100 doubles written to the end, and not a byte further: clean
    const size_t bytes = 100 * sizeof(double);
    std::vector<unsigned char> b = guarded_block(bytes, true);
    double one = 1.0, nan_read;
    std::memcpy(&nan_read, b.data(), sizeof(double));
    assert(nan_read != nan_read);  // the poison reads as NaN
    float nan32;
    std::memcpy(&nan32, b.data() + 4, sizeof(float));
    assert(nan32 != nan32);
    for (size_t i = 0; i < 100; ++i) std::memcpy(b.data() + 8 * i, &one, 8);
    assert(tail_check(b, bytes) == -1);
    b[bytes] = 0;  // one byte past the request
    assert(tail_check(b, bytes) == 0);
    b[bytes] = DEBUG_CANARY;
    b[b.size() - 1] = 0x5A;  // the block's last byte
    assert(tail_check(b, bytes) == (int64_t)dev_debug_tail_length(bytes) - 1);
  }
  {  // integers are zeroed; an element written one past the end is found at offset 0
    const size_t bytes = 7 * sizeof(int32_t);
    std::vector<unsigned char> b = guarded_block(bytes, false);
    for (size_t i = 0; i < bytes; ++i) assert(b[i] == 0);
    const int32_t v = 3;
    std::memcpy(b.data() + bytes, &v, sizeof v);
    assert(tail_check(b, bytes) == 0);
  }
  {  // no bytes asked for: the whole block is tail
    std::vector<unsigned char> b = guarded_block(0, true);
    assert(b.size() == 256 && tail_check(b, 0) == -1);
    b[17] = 0;
    assert(tail_check(b, 0) == 17);
  }
  assert(dev_debug_first_mismatch(nullptr, 0, DEBUG_CANARY) == -1);
  // the kinds the owners pass on
  DevBuf<double> d; DevBuf<float> f; DevBuf<int32_t> i; DevBuf<unsigned long long> u; DevBuf<owners_test::Pose> p;
  DevBuf<owners_test::Mixed> m;
  assert(d.alloc(3) == hipSuccess && last_floating == 1);
  assert(i.alloc(3) == hipSuccess && last_floating == 0);
  assert(f.alloc(3) == hipSuccess && last_floating == 1);
  assert(u.alloc(3) == hipSuccess && last_floating == 0);
  assert(p.alloc(3) == hipSuccess && last_floating == 1);
  assert(m.alloc(3) == hipSuccess && last_floating == 0);
  DevArena A;
  double* x = nullptr; const float* cf = nullptr; uint8_t* b8 = nullptr; owners_test::Pose* ps = nullptr;
  assert(A.raw(x, 2) == hipSuccess && last_floating == 1);
  assert(A.raw(b8, 2) == hipSuccess && last_floating == 0);
  assert(A.alloc(ps, 2, nullptr) == hipSuccess && last_floating == 1);
  assert(A.upload(cf, std::vector<float>{1.f, 2.f}, nullptr, nullptr) == hipSuccess && last_floating == 1 && cf[1] == 2.f);
  assert(A.upload(b8, std::vector<uint8_t>{1, 2}, nullptr, nullptr) == hipSuccess && last_floating == 0);
}
static int early_return(std::string& err) {
  DevBuf<double> a, b;
  HIPCHK(a.alloc(10));
  fail_after = 0;
  HIPCHK(b.alloc(10));  // fails: a must go back
  return 0;
}
int main() {
  {
    DevBuf<double> a;
    assert(a.get() == nullptr);
    assert(a.alloc(100) == hipSuccess && live.size() == 1);
    a[99] = 1.0;
    assert(a.alloc(7) == hipSuccess && live.size() == 1);  // re-alloc frees the first
    DevBuf<double> b(std::move(a));
    assert(a.get() == nullptr && b.get() && live.size() == 1);
    DevBuf<double> c;
    assert(c.alloc(3) == hipSuccess && live.size() == 2);
    c = std::move(b);
    assert(live.size() == 1 && b.get() == nullptr);
    c = std::move(c);
    assert(live.size() == 1 && c.get());
    double* p = c + 2;
    *p = 2.0;
  }
  assert(live.empty());
  std::string err;
  assert(early_return(err) == SIM3OPT_ERR_HIP && live.empty() && !err.empty());
  {
    DevArena A;
    double* x = nullptr; float* f = nullptr; const int32_t* ci = nullptr; uint8_t* u = nullptr; int32_t* e = nullptr;
    assert(A.raw(x, 0) == hipSuccess && x);  // at least one element
    x[0] = 3.0;
    assert(A.alloc(f, 5, nullptr) == hipSuccess && f[4] == 0.f);
    assert(A.alloc(x, 9, (hipStream_t)0x10) == hipSuccess && x[8] == 0.0);
    std::vector<int32_t> h{1, 2, 3}, none;
    StagedUploads st;
    assert(A.upload(ci, h, nullptr, &st) == hipSuccess && ci[2] == 3);
    assert(A.upload(ci, h, (hipStream_t)0x10, nullptr) == hipSuccess && ci[1] == 2);
    assert(A.upload(e, h, nullptr, nullptr) == hipSuccess && e[0] == 1);
    assert(A.upload(e, none, nullptr, nullptr) == hipSuccess && e);
    std::vector<uint8_t> hu(4, 7);
    assert(A.upload(u, hu, nullptr, nullptr) == hipSuccess && u[3] == 7);
    assert(live.size() == 8);
    fail_after = 0;
    double* y = nullptr;
    assert(A.alloc(y, 4, nullptr) != hipSuccess && y == nullptr && live.size() == 8);
    A.release();
    assert(live.empty());
    A.release();
    assert(A.raw(x, 4) == hipSuccess && live.size() == 1);  // usable again; the destructor releases
  }
  assert(live.empty());
  debug_arithmetic();
  assert(live.empty());
  std::puts("owners ok");
  return 0;
}
