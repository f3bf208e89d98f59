// direct_factor.hip -- BlockLdl (direct_factor.hpp): the one translation unit that holds and launches the exact
// block Cholesky kernels (direct_kernels.hpp), the selected inversion on their pattern (selinv_kernels.hpp) and the
// blocks of the inverse outside it (cov_kernels.hpp).
#include "direct_factor.hpp"

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>

#include "sim3_math.hpp"

namespace sim3opt {

using sim3::Sim3;
constexpr int WG = 256;  // the streaming kernels: 4 wavefronts of 64

#include "dev_common.hpp"
#include "direct_args.hpp"
#include "direct_kernels.hpp"
#include "selinv_kernels.hpp"
#include "cov_kernels.hpp"

struct BlockLdl::Dev {
  LdlArgs A{};
  SelArgs S{};  // (maxdiag_bits, singular: per call)
  CovArgs C{};  // (W, wblocks: per call)
  int32_t* flags = nullptr;
};

BlockLdl::BlockLdl() : d_(new Dev) {}
BlockLdl::~BlockLdl() { release(); }
int32_t* BlockLdl::selinv_flags() const { return d_->flags; }

bool BlockLdl::build_plan(int32_t nb, const int32_t* rowptr, const int32_t* colidx, int64_t max_pairs,
                          int32_t subtree, const char* knobs, bool with_selinv, std::string& why) {
  release();
  knobs_ = knobs;
  auto knob = [&](const char* name) { return std::getenv((knobs_ + name).c_str()); };
  if (const char* ev = knob("_SUBTREE")) subtree = std::atoi(ev);
  wg_sub_ = LDL_WG_SUB;
  if (const char* ev = knob("_WG_SUB")) wg_sub_ = std::max(64, std::min(LDL_WG_TOP, std::atoi(ev) / 64 * 64));
  trace_ = knob("_TRACE") != nullptr;  // tuning aid: time stamps of the top group's levels / rounds
  if (build_direct_plan(nb, rowptr, colidx, max_pairs, subtree, plan_, why, wg_sub_ / 64) &&
      (!with_selinv || build_selinv_plan(plan_, sel_, why)))
    return true;
  release();
  return false;
}

hipError_t BlockLdl::upload(hipStream_t stream, StagedUploads* staged) {
  hipError_t e = hipSuccess;
  // (after the first failure nothing more is allocated; the blocks so far go with release())
  auto up = [&](const int32_t*& dptr, const std::vector<int32_t>& h) {
    if (e == hipSuccess) e = mem_.upload(dptr, h, stream, staged);
  };
  auto alloc = [&](double*& dptr, size_t count) {
    if (e == hipSuccess) e = mem_.alloc(dptr, count, nullptr);
  };
  const DirectPlan& P = plan_;
  LdlArgs& A = d_->A;
  up(A.perm, P.perm); up(A.colptr, P.colptr); up(A.lrow, P.lrow); up(A.lcol, P.lcol);
  up(A.srcptr, P.srcptr); up(A.src, P.src); up(A.pairptr, P.pairptr); up(A.pa, P.pa); up(A.pb, P.pb);
  up(A.pcol, P.pcol); up(A.gptr, P.gptr); up(A.lcolp, P.lcolp); up(A.tpre, P.tpre); up(A.tprey, P.tprey);
  up(A.bord, P.bord); up(A.brow, P.brow); up(A.rptr, P.rptr); up(A.cells, P.cells);
  A.ntpre = (int32_t)P.tpre.size(); A.ntprey = (int32_t)P.tprey.size();
  A.nb = P.nb; A.nL = (int32_t)P.nL;
  alloc(A.Aperm, 49 * (size_t)P.nL); alloc(A.bp, 7 * (size_t)P.nb); alloc(A.L, 49 * (size_t)P.nL);
  alloc(A.Dinv, 49 * (size_t)P.nb); alloc(A.y, 7 * (size_t)P.nb); alloc(A.xp, 7 * (size_t)P.nb);
  double* p = nullptr;
  if (trace_) {
    alloc(p, 256);
    A.dbg = reinterpret_cast<long long*>(p);
  }
  if (!sel_.zptr.empty()) {  // (selected inversion planned)
    SelArgs& S = d_->S;
    up(S.zptr, sel_.zptr); up(S.za, sel_.za); up(S.zt, sel_.zt); up(S.zl, sel_.zl);
    alloc(S.Z, 49 * (size_t)P.nL);
    S.colptr = A.colptr; S.lrow = A.lrow; S.lcol = A.lcol; S.gptr = A.gptr; S.lcolp = A.lcolp;
    S.L = A.L; S.Dinv = A.Dinv; S.nb = A.nb;
    alloc(p, 1);
    d_->flags = reinterpret_cast<int32_t*>(p);
    // the elimination tree, for the blocks outside the pattern: parents have larger indices
    parent_.assign(P.nb, -1);
    depth_.assign(P.nb, 0);
    for (int32_t j = P.nb - 1; j >= 0; --j)
      if (P.colptr[j + 1] - P.colptr[j] > 1) {
        parent_[j] = P.lrow[P.colptr[j] + 1];
        depth_[j] = depth_[parent_[j]] + 1;
      }
    CovArgs& C = d_->C;
    up(C.depth, depth_);
    C.colptr = A.colptr; C.lrow = A.lrow; C.L = A.L; C.Dinv = A.Dinv; C.nb = A.nb;
  }
  ready_ = e == hipSuccess;
  return e;
}

void BlockLdl::gather(const double* vals, const double* b, hipStream_t stream) {
  LdlArgs& A = d_->A;
  A.vals = vals;
  A.b = b;
  hipLaunchKernelGGL(k_ldl_gather, dim3(std::max(1, std::min(1024, (A.nL + 3) / 4))), dim3(WG), 0, stream, A);
}

hipError_t BlockLdl::factor(double lambda, int32_t* fail, int32_t token, double* x, hipStream_t stream) {
  LdlArgs& A = d_->A;
  A.lambda = lambda;
  A.fail = fail;
  A.fail_token = token;
  A.x = x;
  const int ng = plan_.ngroups();
  if (ng > 1) hipLaunchKernelGGL((k_ldl<true, false>), dim3(ng - 1), dim3(wg_sub_), 0, stream, A, 0);
  if (x) hipLaunchKernelGGL((k_ldl<true, true>), dim3(1), dim3(LDL_WG_TOP), 0, stream, A, ng - 1);
  else hipLaunchKernelGGL((k_ldl<true, false>), dim3(1), dim3(LDL_WG_TOP), 0, stream, A, ng - 1);
  if (x && ng > 1) hipLaunchKernelGGL((k_ldl<false, true>), dim3(ng - 1), dim3(wg_sub_), 0, stream, A, 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !x || !A.dbg) return e;
  long long h[256];
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
  if ((e = hipMemcpy(h, A.dbg, sizeof(h), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  std::fprintf(stderr, "sim3opt: %s_TRACE: top group stamps [us from start] (level start / after A+B per round / "
               "... / down start / end):", knobs_.c_str());
  for (long long i = 0; i < h[255] && i < 255; ++i) std::fprintf(stderr, " %.1f", (h[i] - h[0]) * 0.01);
  std::fprintf(stderr, "\n");
  return hipSuccess;
}

void BlockLdl::selinv(const unsigned long long* maxdiag_bits, int32_t* singular, hipStream_t stream, bool invert) {
  SelArgs& S = d_->S;
  S.maxdiag_bits = maxdiag_bits;
  S.singular = singular;
  const int ng = plan_.ngroups();
  hipLaunchKernelGGL(k_selinv_pivots, dim3((7 * S.nb + WG - 1) / WG), dim3(WG), 0, stream, S);
  if (!invert) return;
  hipLaunchKernelGGL(k_selinv, dim3(1), dim3(LDL_WG_TOP), 0, stream, S, ng - 1);
  if (ng > 1) hipLaunchKernelGGL(k_selinv, dim3(ng - 1), dim3(wg_sub_), 0, stream, S, 0);
}

void BlockLdl::pick(const int32_t* slot, const int32_t* trans, int32_t n, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_selinv_pick, dim3((49 * n + WG - 1) / WG), dim3(WG), 0, stream, (const double*)d_->S.Z, slot,
                     trans, n, out);
}

void BlockLdl::cov_paths(const int32_t* vcol, const int32_t* voff, int32_t nv, double* W, int32_t wblocks,
                         hipStream_t stream) {
  CovArgs C = d_->C;
  C.W = W;
  C.wblocks = wblocks;
  if (nv > 0) hipLaunchKernelGGL(k_cov_paths, dim3((nv + COV_NW - 1) / COV_NW), dim3(WG), 0, stream, C, vcol, voff, nv);
}

void BlockLdl::cov_pairs(const int32_t* pa, const int32_t* pb, const int32_t* plen, int32_t np, double* W,
                         int32_t wblocks, double* out, hipStream_t stream) {
  CovArgs C = d_->C;
  C.W = W;
  C.wblocks = wblocks;
  if (np > 0)
    hipLaunchKernelGGL(k_cov_pairs, dim3((np + COV_NW - 1) / COV_NW), dim3(WG), 0, stream, C, pa, pb, plen, np, out);
}

hipError_t BlockLdl::debug_read(double* Aperm, double* bp, double* L, double* Dinv, double* y, double* xp,
                                double* Z) const {
  const LdlArgs& A = d_->A;
  const size_t nL = (size_t)plan_.nL, nb = (size_t)plan_.nb;
  hipError_t e = hipSuccess;
  auto get = [&](double* dst, const double* src, size_t count) {
    if (e == hipSuccess && dst && src && count) e = hipMemcpy(dst, src, sizeof(double) * count, hipMemcpyDeviceToHost);
  };
  get(Aperm, A.Aperm, 49 * nL); get(bp, A.bp, 7 * nb); get(L, A.L, 49 * nL); get(Dinv, A.Dinv, 49 * nb);
  get(y, A.y, 7 * nb); get(xp, A.xp, 7 * nb); get(Z, d_->S.Z, 49 * nL);
  return e;
}

void BlockLdl::debug_forget() {
  LdlArgs& A = d_->A;
  A.vals = nullptr; A.b = nullptr; A.x = nullptr; A.fail = nullptr;
  d_->S.maxdiag_bits = nullptr; d_->S.singular = nullptr;
}

void BlockLdl::release() {
  mem_.release();
  *d_ = Dev{};
  plan_ = DirectPlan();
  sel_ = SelinvPlan();
  parent_.clear();
  depth_.clear();
  ready_ = false;
}

}  // namespace sim3opt
