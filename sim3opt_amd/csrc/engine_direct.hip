// engine_direct.hip -- when the LM solves exactly (LinearSolverEigen = SimplicialLDLT, kitti_surf.cpp:553-554), and
// the marginal covariances (SparseOptimizer::computeMarginals); the factorisations are BlockLdl's (direct_factor.hpp)
#include "engine_impl.hpp"

namespace sim3opt {

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
  if (opt.direct_max_pairs > 0) max_pairs = opt.direct_max_pairs;
  if (!forced && nb > 60000) return SIM3OPT_OK;
  std::string why;
  if (!lm_factor.build_plan(nb, s.rowptr.data(), s.colidx.data(), max_pairs, 0, "SIM3OPT_DIRECT", false, why)) {
    if (forced) {
      err = "linear_solver = 1: " + why;
      return SIM3OPT_ERR_ARG;
    }
    if (opt.verbose) std::fprintf(stderr, "sim3opt: no exact factorisation (%s): PCG\n", why.c_str());
    return SIM3OPT_OK;
  }
  HIPCHK(lm_factor.upload(stream, &staged));  // (init synchronises once at its end)
  const DirectPlan& P = lm_factor.plan();
  if (opt.verbose)
    std::fprintf(stderr,
                 "sim3opt: exact block Cholesky: %d columns, %lld blocks in L, %lld block products, "
                 "tree height %d, %d groups\n",
                 nb, (long long)P.nL, (long long)P.npairs, P.height, P.ngroups());
  use_direct = true;
  return SIM3OPT_OK;
}

// (H + lambda I) x = b, exactly; x in d_x.  A non-positive pivot raises d_sc->fail (read by the
// caller together with the trial's chi2: no extra round trip).
int Engine::direct_solve(double lambda, std::string& err) {
  // (no reset of d_sc->fail: a failing factorisation stores this solve's token there, older values differ)
  fail_token = fail_token >= (1 << 30) ? 2 : fail_token + 1;
  HIPCHK(lm_factor.factor(lambda, &d_sc->fail, fail_token, d_x, stream));
  return SIM3OPT_OK;
}

// ---- marginal covariances ----

int Engine::marginal_init(std::string& err) {
  if (!marg_refused.empty()) {
    err = marg_refused;
    return SIM3OPT_ERR_STATE;
  }
  // the plan the LM's factorisation would use (same knobs), but with the limit of an explicit request
  const int64_t max_pairs = opt.direct_max_pairs > 0 ? opt.direct_max_pairs : 30000000;
  std::string why;
  if (!marg_factor.build_plan(nb, st.rowptr.data(), st.colidx.data(), max_pairs, 0, "SIM3OPT_DIRECT", true, why)) {
    marg_refused = "marginals: " + why;
    err = marg_refused;
    return SIM3OPT_ERR_STATE;
  }
  const DirectPlan& P = marg_factor.plan();
  mpos.assign(nb, 0);
  for (int32_t j = 0; j < nb; ++j) mpos[P.perm[j]] = j;
  HIPCHK(marg_factor.upload(stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (opt.verbose)
    std::fprintf(stderr, "sim3opt: marginals: %d columns, %lld blocks of L / Z, %lld + %lld block products, %d groups\n",
                 nb, (long long)P.nL, (long long)P.npairs, (long long)marg_factor.selinv_plan().nprod, P.ngroups());
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
  if (!marg_factor.ready()) {
    int rc = marginal_init(err);
    if (rc) return rc;
  }
  // the requested blocks: Z(a, b) is block (pos a, pos b) of Z, stored in the lower triangle
  const DirectPlan& P = marg_factor.plan();
  std::vector<int32_t> slot(std::max(n, 1)), trans(std::max(n, 1));
  for (int32_t q = 0; q < n; ++q) {
    if (row_a[q] < 0 || row_b[q] < 0 || row_a[q] >= nb || row_b[q] >= nb) {
      err = "marginals: fixed vertex in a pair";
      return SIM3OPT_ERR_ARG;
    }
    const int32_t pa = mpos[row_a[q]], pb = mpos[row_b[q]];
    const int32_t i = std::max(pa, pb), j = std::min(pa, pb);
    const auto b = P.lrow.begin() + P.colptr[j], e = P.lrow.begin() + P.colptr[j + 1];
    const auto it = std::lower_bound(b, e, i);
    if (it == e || *it != i) {
      err = "marginals: pair outside the pattern of the factor (not a vertex with itself or an edge)";
      return SIM3OPT_ERR_ARG;
    }
    slot[q] = (int32_t)(it - P.lrow.begin());
    trans[q] = pa < pb ? 1 : 0;
  }
  int rc = linearize(err);  // H (and b, unused) at the current estimates
  if (rc) return rc;
  int32_t* flags = marg_factor.selinv_flags();  // the factor's fail word, the singular flag
  HIPCHK(hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), stream));
  marg_factor.gather(d_vals, d_b, stream);
  HIPCHK(marg_factor.factor(lambda, flags, 1, nullptr, stream));
  marg_factor.selinv(&d_sc->maxdiag_bits, flags + 1, stream);
  HIPCHK(hipGetLastError());
  int32_t *d_idx = nullptr;
  double* d_out = nullptr;
  int32_t hflags[2] = {0, 0};
  hipError_t e = dev_malloc((void**)&d_idx, sizeof(int32_t) * 2 * (size_t)std::max(n, 1));
  if (e == hipSuccess) e = dev_malloc((void**)&d_out, sizeof(double) * 49 * (size_t)std::max(n, 1));
  if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_idx, slot.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_idx + n, trans.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess && n > 0) {
    marg_factor.pick(d_idx, d_idx + n, n, d_out, stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess && n > 0) e = hipMemcpyAsync(cov, d_out, sizeof(double) * 49 * n, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (d_idx) dev_free(d_idx);
  if (d_out) dev_free(d_out);
  if (e != hipSuccess) {
    err = std::string("marginals: ") + hipGetErrorString(e);
    return SIM3OPT_ERR_HIP;
  }
  const int32_t fail = hflags[0], singular = hflags[1];
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
