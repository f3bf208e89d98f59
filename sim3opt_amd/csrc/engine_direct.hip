// engine_direct.hip -- exact sparse block Cholesky (LinearSolverEigen = SimplicialLDLT, kitti_surf.cpp:553-554)
// and the selected inversion on its pattern (marginal covariances, SparseOptimizer::computeMarginals)
#include "engine_impl.hpp"

namespace sim3opt {

#include "direct_kernels.hpp"
#include "selinv_kernels.hpp"

void Engine::direct_gather() {
  ldl.vals = d_vals;
  ldl.b = d_b;
  hipLaunchKernelGGL(k_ldl_gather, dim3(std::max(1, std::min(1024, (ldl.nL + 3) / 4))), dim3(WG), 0, stream, ldl);
}

// plan (host, once per initialize) + buffers; leaves use_direct false when the factorisation
// would be too expensive (the PCG takes over) unless the caller insists
int Engine::direct_init(const Structure& s, std::string& err) {
  const bool forced = opt.linear_solver == 1;
  if (comm.world > 1) {
    if (forced) {
      err = "linear_solver = 1: the exact factorisation runs on one GPU (small graphs are not sharded)";
      return SIM3OPT_ERR_ARG;
    }
    return SIM3OPT_OK;
  }
  // automatic: only where a factorisation costs less than a few PCG iterations would
  int64_t max_pairs = forced ? 30000000 : 300000;
  int32_t subtree = 0;
  if (opt.direct_max_pairs > 0) max_pairs = opt.direct_max_pairs;
  if (const char* ev = std::getenv("SIM3OPT_DIRECT_SUBTREE")) subtree = std::atoi(ev);
  if (const char* ev = std::getenv("SIM3OPT_DIRECT_WG_SUB")) ldl_wg_sub = std::max(64, std::min(LDL_WG_TOP, std::atoi(ev) / 64 * 64));
  if (!forced && nb > 60000) return SIM3OPT_OK;
  std::string why;
  if (!build_direct_plan(nb, s.rowptr.data(), s.colidx.data(), max_pairs, subtree, dplan, why,
                         ldl_wg_sub / 64)) {
    dplan = DirectPlan();
    if (forced) {
      err = "linear_solver = 1: " + why;
      return SIM3OPT_ERR_ARG;
    }
    if (opt.verbose) std::fprintf(stderr, "sim3opt: no exact factorisation (%s): PCG\n", why.c_str());
    return SIM3OPT_OK;
  }
  int rc = SIM3OPT_OK;
#define DCHK(call) do { rc = (call); if (rc) return rc; } while (0)
  DCHK(direct_up(ldl.perm, dplan.perm, err));
  DCHK(direct_up(ldl.colptr, dplan.colptr, err));
  DCHK(direct_up(ldl.lrow, dplan.lrow, err));
  DCHK(direct_up(ldl.lcol, dplan.lcol, err));
  DCHK(direct_up(ldl.srcptr, dplan.srcptr, err));
  DCHK(direct_up(ldl.src, dplan.src, err));
  DCHK(direct_up(ldl.pairptr, dplan.pairptr, err));
  DCHK(direct_up(ldl.pa, dplan.pa, err));
  DCHK(direct_up(ldl.pb, dplan.pb, err));
  DCHK(direct_up(ldl.pcol, dplan.pcol, err));
  DCHK(direct_up(ldl.gptr, dplan.gptr, err));
  DCHK(direct_up(ldl.lcolp, dplan.lcolp, err));
  DCHK(direct_up(ldl.tpre, dplan.tpre, err));
  DCHK(direct_up(ldl.tprey, dplan.tprey, err));
  ldl.ntpre = (int32_t)dplan.tpre.size();
  ldl.ntprey = (int32_t)dplan.tprey.size();
  DCHK(direct_up(ldl.bord, dplan.bord, err));
  DCHK(direct_up(ldl.brow, dplan.brow, err));
  DCHK(direct_up(ldl.rptr, dplan.rptr, err));
  DCHK(direct_up(ldl.cells, dplan.cells, err));
  ldl.nb = nb;
  ldl.nL = (int32_t)dplan.nL;
  DCHK(direct_alloc(ldl.Aperm, (size_t)49 * dplan.nL, err));
  DCHK(direct_alloc(ldl.bp, (size_t)7 * nb, err));
  DCHK(direct_alloc(ldl.L, (size_t)49 * dplan.nL, err));
  DCHK(direct_alloc(ldl.Dinv, (size_t)49 * nb, err));
  DCHK(direct_alloc(ldl.y, (size_t)7 * nb, err));
  DCHK(direct_alloc(ldl.xp, (size_t)7 * nb, err));
#undef DCHK
  ldl.dbg = nullptr;
  if (std::getenv("SIM3OPT_DIRECT_TRACE")) {  // tuning aid: per-level time stamps of the top group
    double* p = nullptr;
    int rc2 = direct_alloc(p, 256, err);
    if (rc2) return rc2;
    ldl.dbg = reinterpret_cast<long long*>(p);
  }
  if (opt.verbose)
    std::fprintf(stderr,
                 "sim3opt: exact block Cholesky: %d columns, %lld blocks in L, %lld block products, "
                 "tree height %d, %d groups\n",
                 nb, (long long)dplan.nL, (long long)dplan.npairs, dplan.height, dplan.ngroups());
  use_direct = true;
  return SIM3OPT_OK;
}

// (H + lambda I) x = b, exactly; x in d_x.  A non-positive pivot raises d_sc->fail (read by the
// caller together with the trial's chi2: no extra round trip).
int Engine::direct_solve(double lambda, std::string& err) {
  // (no reset of d_sc->fail: a failing factorisation stores this solve's token there, older values differ)
  fail_token = fail_token >= (1 << 30) ? 2 : fail_token + 1;
  ldl.fail_token = fail_token;
  ldl.vals = d_vals;
  ldl.b = d_b;
  ldl.x = d_x;
  ldl.sc = d_sc;
  ldl.lambda = lambda;
  const int ng = dplan.ngroups();
  if (ng > 1)
    hipLaunchKernelGGL((k_ldl<true, false>), dim3(ng - 1), dim3(ldl_wg_sub), 0, stream, ldl, 0);
  hipLaunchKernelGGL((k_ldl<true, true>), dim3(1), dim3(LDL_WG_TOP), 0, stream, ldl, ng - 1);
  if (ng > 1)
    hipLaunchKernelGGL((k_ldl<false, true>), dim3(ng - 1), dim3(ldl_wg_sub), 0, stream, ldl, 0);
  HIPCHK(hipGetLastError());
  if (ldl.dbg) {
    long long h[256];
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipMemcpy(h, ldl.dbg, sizeof(h), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "sim3opt: direct solve, top group stamps [us from start] (level start / after A+B per round / ... / down start / end):");
    for (long long i = 0; i < h[255] && i < 255; ++i) std::fprintf(stderr, " %.1f", (h[i] - h[0]) * 0.01);
    std::fprintf(stderr, "\n");
  }
  return SIM3OPT_OK;
}

// ---- marginal covariances ----

int Engine::marginal_init(std::string& err) {
  if (!marg_refused.empty()) {
    err = marg_refused;
    return SIM3OPT_ERR_STATE;
  }
  // the plan the LM's factorisation would use (same knobs), but with the limit of an explicit request
  int64_t max_pairs = opt.direct_max_pairs > 0 ? opt.direct_max_pairs : 30000000;
  int32_t subtree = 0;
  if (const char* ev = std::getenv("SIM3OPT_DIRECT_SUBTREE")) subtree = std::atoi(ev);
  m_wg_sub = LDL_WG_SUB;
  if (const char* ev = std::getenv("SIM3OPT_DIRECT_WG_SUB")) m_wg_sub = std::max(64, std::min(LDL_WG_TOP, std::atoi(ev) / 64 * 64));
  std::string why;
  if (!build_direct_plan(nb, st.rowptr.data(), st.colidx.data(), max_pairs, subtree, mplan, why, m_wg_sub / 64) ||
      !build_selinv_plan(mplan, msel, why)) {
    mplan = DirectPlan();
    msel = SelinvPlan();
    marg_refused = "marginals: " + why;
    err = marg_refused;
    return SIM3OPT_ERR_STATE;
  }
  mpos.assign(nb, 0);
  for (int32_t j = 0; j < nb; ++j) mpos[mplan.perm[j]] = j;
  // (uploads straight from the plan's vectors, which live as long as the engine)
  auto up = [&](const int32_t*& dptr, const std::vector<int32_t>& h) -> int {
    int32_t* p = nullptr;
    HIPCHK(dev_malloc((void**)&p, sizeof(int32_t) * std::max<size_t>(h.size(), 1)));
    direct_owned.push_back(p);
    if (!h.empty()) HIPCHK(hipMemcpyAsync(p, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice, stream));
    dptr = p;
    return SIM3OPT_OK;
  };
  int rc = SIM3OPT_OK;
#define MCHK(call) do { rc = (call); if (rc) return rc; } while (0)
  LdlArgs& A = mldl;
  A = LdlArgs{};
  MCHK(up(A.perm, mplan.perm));
  MCHK(up(A.colptr, mplan.colptr));
  MCHK(up(A.lrow, mplan.lrow));
  MCHK(up(A.lcol, mplan.lcol));
  MCHK(up(A.srcptr, mplan.srcptr));
  MCHK(up(A.src, mplan.src));
  MCHK(up(A.pairptr, mplan.pairptr));
  MCHK(up(A.pa, mplan.pa));
  MCHK(up(A.pb, mplan.pb));
  MCHK(up(A.pcol, mplan.pcol));
  MCHK(up(A.gptr, mplan.gptr));
  MCHK(up(A.lcolp, mplan.lcolp));
  MCHK(up(A.rptr, mplan.rptr));
  MCHK(up(A.cells, mplan.cells));
  MCHK(up(m_zptr, msel.zptr));
  MCHK(up(m_za, msel.za));
  MCHK(up(m_zt, msel.zt));
  MCHK(up(m_zl, msel.zl));
  A.nb = nb;
  A.nL = (int32_t)mplan.nL;
  MCHK(direct_alloc(A.Aperm, (size_t)49 * mplan.nL, err));
  MCHK(direct_alloc(A.bp, (size_t)7 * nb, err));
  MCHK(direct_alloc(A.L, (size_t)49 * mplan.nL, err));
  MCHK(direct_alloc(A.Dinv, (size_t)49 * nb, err));
  MCHK(direct_alloc(A.y, (size_t)7 * nb, err));
  MCHK(direct_alloc(m_Z, (size_t)49 * mplan.nL, err));
  const size_t nsc = (sizeof(DevScalars) + sizeof(double) - 1) / sizeof(double);
  double* scp = nullptr;  // (zeroed: a DevScalars of its own, then the singularity flag)
  MCHK(direct_alloc(scp, nsc + 1, err));
#undef MCHK
  m_sc = reinterpret_cast<DevScalars*>(scp);
  m_singular = reinterpret_cast<int32_t*>(scp + nsc);
  A.sc = m_sc;
  A.dbg = nullptr;  // (x, xp: the backward solve does not run)
  HIPCHK(hipStreamSynchronize(stream));
  if (opt.verbose)
    std::fprintf(stderr, "sim3opt: marginals: %d columns, %lld blocks of L / Z, %lld + %lld block products, %d groups\n",
                 nb, (long long)mplan.nL, (long long)mplan.npairs, (long long)msel.nprod, mplan.ngroups());
  marg_ready = true;
  return SIM3OPT_OK;
}

int Engine::marginals(double lambda, int32_t n, const int32_t* row_a, const int32_t* row_b, double* cov,
                      std::string& err) {
  if (comm.world > 1) {
    err = "marginals: one GPU only (the graph is partitioned over ranks)";
    return SIM3OPT_ERR_STATE;
  }
  if (!(lambda >= 0.0) || !(lambda < DBL_MAX)) {
    err = "marginals: lambda must be finite and >= 0";
    return SIM3OPT_ERR_ARG;
  }
  if (!marg_ready) {
    int rc = marginal_init(err);
    if (rc) return rc;
  }
  // the requested blocks: Z(a, b) is block (pos a, pos b) of Z, stored in the lower triangle
  std::vector<int32_t> slot(std::max(n, 1)), trans(std::max(n, 1));
  for (int32_t q = 0; q < n; ++q) {
    if (row_a[q] < 0 || row_b[q] < 0 || row_a[q] >= nb || row_b[q] >= nb) {
      err = "marginals: fixed vertex in a pair";
      return SIM3OPT_ERR_ARG;
    }
    const int32_t pa = mpos[row_a[q]], pb = mpos[row_b[q]];
    const int32_t i = std::max(pa, pb), j = std::min(pa, pb);
    const auto b = mplan.lrow.begin() + mplan.colptr[j], e = mplan.lrow.begin() + mplan.colptr[j + 1];
    const auto it = std::lower_bound(b, e, i);
    if (it == e || *it != i) {
      err = "marginals: pair outside the pattern of the factor (not a vertex with itself or an edge)";
      return SIM3OPT_ERR_ARG;
    }
    slot[q] = (int32_t)(it - mplan.lrow.begin());
    trans[q] = pa < pb ? 1 : 0;
  }
  int rc = linearize(err);  // H (and b, unused) at the current estimates
  if (rc) return rc;
  LdlArgs& A = mldl;
  A.vals = d_vals;
  A.b = d_b;
  A.lambda = lambda;
  A.fail_token = 1;
  HIPCHK(hipMemsetAsync(&m_sc->fail, 0, sizeof(int32_t), stream));
  HIPCHK(hipMemsetAsync(m_singular, 0, sizeof(int32_t), stream));
  const int ng = mplan.ngroups();
  hipLaunchKernelGGL(k_ldl_gather, dim3(std::max(1, std::min(1024, (A.nL + 3) / 4))), dim3(WG), 0, stream, A);
  if (ng > 1) hipLaunchKernelGGL((k_ldl<true, false>), dim3(ng - 1), dim3(m_wg_sub), 0, stream, A, 0);
  hipLaunchKernelGGL((k_ldl<true, false>), dim3(1), dim3(LDL_WG_TOP), 0, stream, A, ng - 1);
  SelArgs S{A.colptr, A.lrow, A.lcol, A.gptr, A.lcolp, m_zptr, m_za, m_zt, m_zl, A.L, A.Dinv, m_Z, nb,
            d_sc, m_singular};
  hipLaunchKernelGGL(k_selinv_pivots, dim3((7 * nb + WG - 1) / WG), dim3(WG), 0, stream, S);
  hipLaunchKernelGGL(k_selinv, dim3(1), dim3(LDL_WG_TOP), 0, stream, S, ng - 1);
  if (ng > 1) hipLaunchKernelGGL(k_selinv, dim3(ng - 1), dim3(m_wg_sub), 0, stream, S, 0);
  HIPCHK(hipGetLastError());
  int32_t *d_idx = nullptr;
  double* d_out = nullptr;
  int32_t fail = 0, singular = 0;
  hipError_t e = dev_malloc((void**)&d_idx, sizeof(int32_t) * 2 * (size_t)std::max(n, 1));
  if (e == hipSuccess) e = dev_malloc((void**)&d_out, sizeof(double) * 49 * (size_t)std::max(n, 1));
  if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_idx, slot.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_idx + n, trans.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess && n > 0) {
    hipLaunchKernelGGL(k_selinv_pick, dim3((49 * n + WG - 1) / WG), dim3(WG), 0, stream, (const double*)m_Z,
                       (const int32_t*)d_idx, (const int32_t*)(d_idx + n), n, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess && n > 0) e = hipMemcpyAsync(cov, d_out, sizeof(double) * 49 * n, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&fail, &m_sc->fail, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&singular, m_singular, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (d_idx) dev_free(d_idx);
  if (d_out) dev_free(d_out);
  if (e != hipSuccess) {
    err = std::string("marginals: ") + hipGetErrorString(e);
    return SIM3OPT_ERR_HIP;
  }
  bool finite = true;
  for (size_t k = 0; k < (size_t)49 * n && finite; ++k) finite = std::isfinite(cov[k]);
  if (fail || singular || !finite) {
    err = fail ? "marginals: H + lambda I is not positive definite (a non-positive pivot)"
          : singular ? "marginals: H + lambda I is numerically singular (a pivot below 1e-13 max |H_dd|)"
                     : "marginals: non-finite result";
    err += ": no fixed vertex, a masked degree of freedom, or lambda too small for this H";
    return SIM3OPT_ERR_STATE;
  }
  return SIM3OPT_OK;
}

int engine_marginals(Engine* e, double lambda, int32_t n, const int32_t* row_a, const int32_t* row_b, double* cov,
                     std::string& err) {
  return e->marginals(lambda, n, row_a, row_b, cov, err);
}

}  // namespace sim3opt
