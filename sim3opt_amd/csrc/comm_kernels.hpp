// comm_kernels.hpp -- the three kernels of the in-process transport (Comm::kind == 3, comm_local.hip): the ranks of
// one process store their operands straight into each other's device mailboxes.  On distinct devices the peer
// pointers are peer-mapped memory (stores travel over xGMI), on one device they are ordinary pointers: the kernels
// are the same.  All three are plain wave64 grid-stride copies / folds of doubles; nothing here is ordered against
// another rank -- that is the host's business (stream synchronise, barrier: see comm_local.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int COMM_WG = 256;        // 4 waves
constexpr int COMM_MAX_PEERS = 8;   // sim3opt_set_devices admits 8 ranks
constexpr int COMM_MAX_GRID_X = 1024;

// up to 8 spans of doubles, src[i] .. src[i] + n[i]  ->  dst[i] .. (by value in the kernel arguments)
struct CommSpans {
  double* dst[COMM_MAX_PEERS];
  const double* src[COMM_MAX_PEERS];
  long long n[COMM_MAX_PEERS];
  int count;
};

// one span, spread over the x dimension of the grid; double2 stores where source and destination are both
// 16-byte aligned at the same element (an odd head and tail go one double at a time)
__device__ __forceinline__ void comm_copy_span(double* __restrict__ dst, const double* __restrict__ src, long long n) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, nt = (long long)gridDim.x * blockDim.x;
  const bool same_phase = ((reinterpret_cast<uintptr_t>(dst) ^ reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
  if (!same_phase) {
    for (long long i = t; i < n; i += nt) dst[i] = src[i];
    return;
  }
  const long long head = (reinterpret_cast<uintptr_t>(dst) & 15u) ? (n > 0 ? 1 : 0) : 0;
  const long long pairs = (n - head) / 2;
  if (t == 0 && head) dst[0] = src[0];
  const double2* s2 = reinterpret_cast<const double2*>(src + head);
  double2* d2 = reinterpret_cast<double2*>(dst + head);
  for (long long i = t; i < pairs; i += nt) d2[i] = s2[i];
  if (t == 0 && head + 2 * pairs < n) dst[n - 1] = src[n - 1];
}

// this rank's payload into every addressed peer's mailbox: one launch per collective, blockIdx.y = the peer
__global__ __launch_bounds__(COMM_WG) void k_comm_put(CommSpans s) {
  const int p = blockIdx.y;
  if (p < s.count) comm_copy_span(s.dst[p], s.src[p], s.n[p]);
}

// mailbox -> destination: the other ranks' spans of an all-gather, the segments of an exchange (the same copy under a
// name of its own: a kernel trace then tells the stores into peer memory from the local moves)
__global__ __launch_bounds__(COMM_WG) void k_comm_unpack(CommSpans s) {
  const int p = blockIdx.y;
  if (p < s.count) comm_copy_span(s.dst[p], s.src[p], s.n[p]);
}

// folds the `world` slots of this rank's mailbox (slot r at mbox + r * slot) in rank order, ((s0 + s1) + s2) + ...,
// or takes the maximum (op == 1; a NaN wins, as numpy.maximum has it): the same order on every rank, so the same bits
__global__ __launch_bounds__(COMM_WG) void k_comm_reduce(const double* __restrict__ mbox, int world, long long slot, int n,
                                                         int op, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int nt = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nt) {
    double acc = mbox[i];
    for (int r = 1; r < world; ++r) {
      const double v = mbox[(long long)r * slot + i];
      if (op == 1) acc = (acc >= v || acc != acc) ? acc : v;
      else acc = acc + v;
    }
    out[i] = acc;
  }
}
