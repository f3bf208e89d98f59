// devmem_owners_driver.cpp -- DevBuf and DevArena (csrc/devmem.hpp) against a stub allocator and stub copies: no GPU and
// no HIP runtime is linked.  Built with -fsanitize=address,undefined and run by tests/test_devmem_owners.py; every
// block must be back after each scope, on the early-return path of HIPCHK too.  Ends with "owners ok".
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
namespace sim3opt {
hipError_t dev_malloc(void** p, size_t bytes) {
  if (fail_after == 0) { fail_after = -1; return hipErrorOutOfMemory; }
  if (fail_after > 0) --fail_after;
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
  std::puts("owners ok");
  return 0;
}
