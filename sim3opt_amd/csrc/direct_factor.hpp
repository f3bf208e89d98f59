// direct_factor.hpp -- BlockLdl: one exact sparse block Cholesky on the device (plan: direct.hpp), its buffers and
// launches, asynchronous on the caller's stream.  Owned by the LM's solver and the marginals (engine_direct.hip) and
// by the bundle adjuster (ba.hip); the kernels and their argument blocks belong to direct_factor.hip alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "devmem.hpp"
#include "direct.hpp"

namespace sim3opt {

class BlockLdl {
 public:
  BlockLdl();
  ~BlockLdl();

  // Host plan of a full-symmetric block-CSR pattern (build_direct_plan), plus the selected inversion's lists
  // when asked; forgets any earlier plan.  Reads the tuning knobs <knobs>_SUBTREE (replaces `subtree`),
  // <knobs>_WG_SUB (threads of a bottom group, 64 ... 512) and <knobs>_TRACE (time stamps of a solve).
  // False, with the reason, when the plan is refused.
  bool build_plan(int32_t nb, const int32_t* rowptr, const int32_t* colidx, int64_t max_pairs, int32_t subtree,
                  const char* knobs, bool with_selinv, std::string& why);
  // Device copies of the plan (through `staged` when given, else straight from the plan) and zeroed buffers;
  // the caller synchronises `stream`.
  hipError_t upload(hipStream_t stream, StagedUploads* staged = nullptr);
  bool ready() const { return ready_; }  // upload() succeeded
  const DirectPlan& plan() const { return plan_; }
  const SelinvPlan& selinv_plan() const { return sel_; }
  int32_t* selinv_flags() const;  // with the selected inversion: two device words for the caller's flags

  // once per linearisation: the block-CSR values of H in the layout of L, b in elimination order
  void gather(const double* vals, const double* b, hipStream_t stream);
  // (H + lambda I) = L L^T, and with x also (H + lambda I) x = b, x by block rows of H.  A non-positive pivot
  // writes `token` into *fail.
  hipError_t factor(double lambda, int32_t* fail, int32_t token, double* x, hipStream_t stream);
  // after factor(): Z = (H + lambda I)^-1 on the pattern of L; a pivot below 1e-13 max |H_dd| (raw bits) sets
  // *singular.  invert = false: the pivot check alone (no block of Z is wanted).
  void selinv(const unsigned long long* maxdiag_bits, int32_t* singular, hipStream_t stream, bool invert = true);
  // out[q] = block slot[q] of Z, transposed where trans[q] (device arrays of n)
  void pick(const int32_t* slot, const int32_t* trans, int32_t n, double* out, hipStream_t stream);
  // Blocks of Z outside the pattern (cov_kernels.hpp), with the selected inversion's plan only.  The elimination
  // tree: parent (-1: a root) and number of proper ancestors of every column.
  const std::vector<int32_t>& tree_parent() const { return parent_; }
  const std::vector<int32_t>& tree_depth() const { return depth_; }
  // after factor(): column vcol[v] of L^-1 on its root path, depth + 1 blocks from block voff[v] of W (device
  // arrays of nv; W holds wblocks blocks of 49)
  void cov_paths(const int32_t* vcol, const int32_t* voff, int32_t nv, double* W, int32_t wblocks, hipStream_t stream);
  // out[p] = sum_t W[pa[p] + t]^T W[pb[p] + t], t < plen[p] ascending (device arrays of np)
  void cov_pairs(const int32_t* pa, const int32_t* pb, const int32_t* plen, int32_t np, double* W, int32_t wblocks,
                 double* out, hipStream_t stream);
  // Diagnostic (sim3opt_debug_factor): host copies of the buffers as the last gather / factor / selinv left them; the
  // caller has synchronised.  A NULL pointer is skipped; Z only with the selected inversion's plan.
  hipError_t debug_read(double* Aperm, double* bp, double* L, double* Dinv, double* y, double* xp, double* Z) const;
  // ... and when the caller's scratch buffers go: the argument blocks forget every per-call pointer (values, b, x,
  // fail word, max |H_dd|, singular flag), so that a launch without a new gather / factor / selinv cannot reach them
  void debug_forget();
  void release();  // frees everything (the caller has synchronised) and forgets the plan

 private:
  DirectPlan plan_;
  SelinvPlan sel_;
  std::string knobs_;
  bool trace_ = false, ready_ = false;
  int wg_sub_ = 0;
  std::vector<int32_t> parent_, depth_;
  struct Dev;               // the kernels' argument blocks: device copies of the plan, the buffers
  std::unique_ptr<Dev> d_;
  DevArena mem_;  // every device block of upload()
};

// Lane sums over the factor's 7x7 block layout (lane l < 49: entry l, column-major), shared with ba.hip's PCG.
// sum over the 7 lanes that share this lane's column index c (lanes 7c .. 7c+6)
__device__ __forceinline__ double ldl_sum_over_r(double v, int c49) {
  double s = 0.0;
#pragma unroll
  for (int rr = 0; rr < 7; ++rr) s += __shfl(v, 7 * c49 + rr);
  return s;
}
// sum over the 7 lanes that share this lane's row index r (lanes r, r+7, ..., r+42)
__device__ __forceinline__ double ldl_sum_over_c(double v, int r49) {
  double s = 0.0;
#pragma unroll
  for (int cc = 0; cc < 7; ++cc) s += __shfl(v, r49 + 7 * cc);
  return s;
}

}  // namespace sim3opt
