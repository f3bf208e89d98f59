// ransac_sample.hpp -- the counter-based sampler of the batched RANSAC stages (pnp_batch.hip, essential_batch.hip).
// Host and device, and no HIP header on the host: tests/cxx/*_math_driver.cpp run the same statements on the CPU.
#pragma once
#include <cstdint>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define SIM3OPT_RANSAC_HD __host__ __device__ __forceinline__
#else
#define SIM3OPT_RANSAC_HD inline
#endif

namespace sim3opt_ransac {

SIM3OPT_RANSAC_HD uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The sample of hypothesis h: K distinct indices below n (n >= K) in exactly K draws.  Draw j picks among the n - j
// indices not yet taken: its number is stepped over the earlier picks in ascending order.  The key holds the seed,
// K and h only.
template <int K>
SIM3OPT_RANSAC_HD void ransac_sample(uint64_t seed, uint32_t h, int n, int idx[K]) {
  int sorted[K] = {};
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint64_t r = splitmix64(seed + (uint64_t)(K * (uint64_t)h + j + 1) * 0x9E3779B97F4A7C15ull);
    int i = (int)(r % (uint64_t)(n - j));
#pragma unroll
    for (int k = 0; k < j; ++k)
      if (sorted[k] <= i) ++i;
    idx[j] = i;
    // insert into the ascending list
    int v = i;
#pragma unroll
    for (int k = 0; k < j; ++k)
      if (sorted[k] > v) { const int s = sorted[k]; sorted[k] = v; v = s; }
    sorted[j] = v;
  }
}

}  // namespace sim3opt_ransac
