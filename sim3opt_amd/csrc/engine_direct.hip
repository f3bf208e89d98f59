// engine_direct.hip -- when the LM solves exactly (LinearSolverEigen = SimplicialLDLT, kitti_surf.cpp:553-554), and
// the marginal covariances (SparseOptimizer::computeMarginals) with the gate of candidate edges on top of them; the
// factorisations are BlockLdl's (direct_factor.hpp)
#include "engine_impl.hpp"
#include "sim3_jac.hpp"

#include <unordered_map>

namespace sim3opt {

#include "gate_kernels.hpp"

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

// The blocks (row_a[q], row_b[q]) of Z = (H + lambda I)^-1 behind sim3opt_marginals (any_pair false: a pair outside
// the pattern of the factor is refused), sim3opt_covariances (any pair of free vertices) and sim3opt_gate_edges
// (fixed_zero: a fixed endpoint, row -1, gives a zero block).  One linearisation, one factorisation; pairs on the
// pattern are picked from the selected inversion (skipped when there is none), the others are computed once per
// unordered pair -- block rows ascending -- by k_cov_paths / k_cov_pairs in chunks whose workspace stays within
// options.cov_workspace_mb, and transposed for the reversed pair.
int Engine::cov_blocks(const char* who, bool any_pair, bool fixed_zero, double lambda, int32_t n,
                       const int32_t* row_a, const int32_t* row_b, double* cov, std::string& err) {
  const std::string pre = std::string(who) + ": ";
  if (comm.world > 1) {
    err = pre + "one GPU only (the graph is partitioned over ranks)";
    return SIM3OPT_ERR_STATE;
  }
  if (!(lambda >= 0.0) || !(lambda < DBL_MAX)) {
    err = pre + "lambda must be finite and >= 0";
    return SIM3OPT_ERR_ARG;
  }
  // options.cov_solver (covariances and the gate only): 1 = columns of the inverse by PCG, 2 = that where the plan of
  // the exact factorisation is refused (engine_columns.hip)
  if (any_pair && opt.cov_solver == 1) return cov_blocks_columns(pre, fixed_zero, lambda, n, row_a, row_b, cov, err);
  if (!marg_factor.ready()) {
    int rc = marginal_init(err);
    if (rc == SIM3OPT_ERR_STATE && any_pair && opt.cov_solver == 2 && !marg_refused.empty())
      return cov_blocks_columns(pre, fixed_zero, lambda, n, row_a, row_b, cov, err);
    if (rc) return rc;
  }
  for (int64_t& v : cov_stats) v = 0;
  // the requested blocks: Z(a, b) is block (pos a, pos b) of Z, stored in the lower triangle
  const DirectPlan& P = marg_factor.plan();
  const std::vector<int32_t>& parent = marg_factor.tree_parent();
  const std::vector<int32_t>& depth = marg_factor.tree_depth();
  enum { ZERO = 0, ON = 1, OFF = 2 };
  std::vector<int32_t> kind(std::max(n, 1)), where(std::max(n, 1)), flip(std::max(n, 1));
  std::vector<int32_t> slot, trans;                  // pairs on the pattern, request order
  std::vector<std::pair<int32_t, int32_t>> off;      // unordered pairs outside it, block rows ascending, first use
  std::unordered_map<int64_t, int32_t> off_index;    // lo * nb + hi -> index into off
  for (int32_t q = 0; q < n; ++q) {
    if (fixed_zero && (row_a[q] < 0 || row_b[q] < 0)) {
      kind[q] = ZERO;
      continue;
    }
    if (row_a[q] < 0 || row_b[q] < 0 || row_a[q] >= nb || row_b[q] >= nb) {
      err = pre + "fixed vertex in a pair";
      return SIM3OPT_ERR_ARG;
    }
    const int32_t pa = mpos[row_a[q]], pb = mpos[row_b[q]];
    const int32_t i = std::max(pa, pb), j = std::min(pa, pb);
    const auto b = P.lrow.begin() + P.colptr[j], e = P.lrow.begin() + P.colptr[j + 1];
    const auto it = std::lower_bound(b, e, i);
    if (it != e && *it == i) {
      kind[q] = ON;
      where[q] = (int32_t)slot.size();
      slot.push_back((int32_t)(it - P.lrow.begin()));
      trans.push_back(pa < pb ? 1 : 0);
      continue;
    }
    if (!any_pair) {
      err = pre + "pair outside the pattern of the factor (not a vertex with itself or an edge)";
      return SIM3OPT_ERR_ARG;
    }
    kind[q] = OFF;
    flip[q] = row_a[q] > row_b[q] ? 1 : 0;
    const int32_t lo = std::min(row_a[q], row_b[q]), hi = std::max(row_a[q], row_b[q]);
    const auto ins = off_index.emplace((int64_t)lo * nb + hi, (int32_t)off.size());
    if (ins.second) off.push_back({lo, hi});
    where[q] = ins.first->second;
  }
  const int32_t n_on = (int32_t)slot.size(), n_off = (int32_t)off.size();
  // ---- chunks of the pairs outside the pattern: index arrays [vcol, voff | pa, pb, plen] per chunk ----
  struct Chunk { int32_t iv, nv, ip, np, p0, blocks; };
  std::vector<Chunk> chunks;
  std::vector<int32_t> idx;  // everything the device reads, one upload: slot, trans, then the chunks' arrays
  idx.insert(idx.end(), slot.begin(), slot.end());
  idx.insert(idx.end(), trans.begin(), trans.end());
  if (n_off > 0) {
    const double lim = opt.cov_workspace_mb * 1048576.0 / 392.0;
    const int64_t limit = (int64_t)std::max(1.0, std::min(lim, 1073741824.0));
    std::vector<int32_t> voff_of(nb, -1), members, vcol, voff, ca, cb, cl;
    int64_t total = 0;
    int32_t p0 = 0;
    auto flush = [&]() {
      Chunk c;
      c.nv = (int32_t)vcol.size(); c.np = (int32_t)ca.size(); c.p0 = p0; c.blocks = (int32_t)total;
      c.iv = (int32_t)idx.size();
      idx.insert(idx.end(), vcol.begin(), vcol.end());
      idx.insert(idx.end(), voff.begin(), voff.end());
      c.ip = (int32_t)idx.size();
      idx.insert(idx.end(), ca.begin(), ca.end());
      idx.insert(idx.end(), cb.begin(), cb.end());
      idx.insert(idx.end(), cl.begin(), cl.end());
      chunks.push_back(c);
      p0 += c.np;
      for (int32_t r : members) voff_of[r] = -1;
      members.clear(); vcol.clear(); voff.clear(); ca.clear(); cb.clear(); cl.clear();
      total = 0;
    };
    for (const auto& pr : off) {
      const int32_t ra = pr.first, rb = pr.second, ja = mpos[ra], jb = mpos[rb];
      auto need_of = [&]() {
        return (int64_t)(voff_of[ra] < 0 ? depth[ja] + 1 : 0) + (voff_of[rb] < 0 ? depth[jb] + 1 : 0);
      };
      if (total + need_of() > limit && !ca.empty()) flush();
      if (total + need_of() > limit) {
        err = pre + "options.cov_workspace_mb is too small for the root paths of one pair of this graph";
        return SIM3OPT_ERR_STATE;
      }
      for (const int32_t r : {ra, rb})
        if (voff_of[r] < 0) {
          voff_of[r] = (int32_t)total;
          members.push_back(r);
          vcol.push_back(mpos[r]);
          voff.push_back((int32_t)total);
          total += depth[mpos[r]] + 1;
        }
      // the common suffix of the two root paths starts at the lowest common ancestor (none: another tree)
      int32_t x = ja, y = jb;
      while (depth[x] > depth[y]) x = parent[x];
      while (depth[y] > depth[x]) y = parent[y];
      while (x != y && x >= 0) { x = parent[x]; y = parent[y]; }
      const int32_t len = x >= 0 && x == y ? depth[x] + 1 : 0;
      ca.push_back(voff_of[ra] + (len ? depth[ja] - depth[x] : 0));
      cb.push_back(voff_of[rb] + (len ? depth[jb] - depth[x] : 0));
      cl.push_back(len);
    }
    if (!ca.empty()) flush();
  }
  int64_t wblocks = 1;
  for (const Chunk& c : chunks) {
    wblocks = std::max<int64_t>(wblocks, c.blocks);
    cov_stats[1] += c.nv;
  }
  cov_stats[0] = (int64_t)chunks.size();
  cov_stats[2] = n_off;
  cov_stats[3] = n_on;
  cov_stats[4] = n_off > 0 ? wblocks * 392 : 0;
  cov_stats[5] = n_on > 0 ? 1 : 0;
  const sim3opt_kernel_times kt0 = kt;  // (not one of the optimiser's linearisations: the counters stay)
  int rc = linearize(err);  // H (and b, unused) at the current estimates
  kt = kt0;
  if (rc) return rc;
  int32_t* flags = marg_factor.selinv_flags();  // the factor's fail word, the singular flag
  HIPCHK(hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), stream));
  marg_factor.gather(d_vals, d_b, stream);
  HIPCHK(marg_factor.factor(lambda, flags, 1, nullptr, stream));
  marg_factor.selinv(&d_sc->maxdiag_bits, flags + 1, stream, n_on > 0);
  HIPCHK(hipGetLastError());
  const int32_t n_out = n_on + n_off;
  int32_t hflags[2] = {0, 0};
  std::vector<double> out((size_t)49 * std::max(n_out, 1));
  DevBuf<int32_t> d_idx;
  DevBuf<double> d_out, d_W;
  // (the launches above and below are on the stream: whatever ends this, they are done before the three blocks go)
  auto body = [&]() -> int {
    HIPCHK(d_idx.alloc(std::max<size_t>(idx.size(), 1)));
    HIPCHK(d_out.alloc(49 * (size_t)std::max(n_out, 1)));
    if (n_off > 0) HIPCHK(d_W.alloc(49 * (size_t)wblocks));
    if (!idx.empty())
      HIPCHK(hipMemcpyAsync(d_idx, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, stream));
    if (n_on > 0) {
      marg_factor.pick(d_idx, d_idx + n_on, n_on, d_out, stream);
      HIPCHK(hipGetLastError());
    }
    for (const Chunk& c : chunks) {
      marg_factor.cov_paths(d_idx + c.iv, d_idx + c.iv + c.nv, c.nv, d_W, (int32_t)wblocks, stream);
      marg_factor.cov_pairs(d_idx + c.ip, d_idx + c.ip + c.np, d_idx + c.ip + 2 * c.np, c.np, d_W, (int32_t)wblocks,
                            d_out + (size_t)49 * (n_on + c.p0), stream);
      HIPCHK(hipGetLastError());
    }
    if (n_out > 0) HIPCHK(hipMemcpyAsync(out.data(), d_out, sizeof(double) * 49 * n_out, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, stream));
    return SIM3OPT_OK;
  };
  rc = body();
  const hipError_t es = hipStreamSynchronize(stream);
  if (rc) return rc;
  HIPCHK(es);
  const int32_t fail = hflags[0], singular = hflags[1];
  bool finite = true;
  for (size_t k = 0; k < (size_t)49 * n_out && finite; ++k) finite = std::isfinite(out[k]);
  if (fail || singular || !finite) {
    err = pre + (fail ? "H + lambda I is not positive definite (a non-positive pivot)"
                 : singular ? "H + lambda I is numerically singular (a pivot below 1e-13 max |H_dd|)"
                            : "non-finite result");
    err += ": no fixed vertex, a masked degree of freedom, or lambda too small for this H";
    return SIM3OPT_ERR_STATE;
  }
  for (int32_t q = 0; q < n; ++q) {
    double* dst = cov + (size_t)49 * q;
    if (kind[q] == ZERO) {
      for (int k = 0; k < 49; ++k) dst[k] = 0.0;
      continue;
    }
    const double* src = out.data() + (size_t)49 * (kind[q] == ON ? where[q] : n_on + where[q]);
    if (kind[q] == OFF && flip[q]) {
      for (int c = 0; c < 7; ++c)
        for (int r = 0; r < 7; ++r) dst[r + 7 * c] = src[c + 7 * r];
    } else {
      std::memcpy(dst, src, sizeof(double) * 49);
    }
  }
  return SIM3OPT_OK;
}

int Engine::marginals(double lambda, int32_t n, const int32_t* row_a, const int32_t* row_b, double* cov,
                      std::string& err) {
  return cov_blocks("marginals", false, false, lambda, n, row_a, row_b, cov, err);
}

// e, S = J Sigma J^T + Omega^-1 and d2 = e^T S^-1 e of candidate edges (vertex indices v0 / v1, their block rows or
// -1; infoinv: Omega^-1, n x 49): nothing of the graph, the estimates or the LM's state is written
int Engine::gate_edges(double lambda, int32_t n, const int32_t* v0, const int32_t* v1, const int32_t* row0,
                       const int32_t* row1, const Sim3* meas, const double* infoinv, double* e_out, double* S_out,
                       double* d2_out, std::string& err) {
  std::vector<int32_t> ra((size_t)3 * std::max(n, 1)), rb((size_t)3 * std::max(n, 1));
  for (int32_t q = 0; q < n; ++q) {
    ra[3 * q] = row0[q]; rb[3 * q] = row0[q];
    ra[3 * q + 1] = row0[q]; rb[3 * q + 1] = row1[q];
    ra[3 * q + 2] = row1[q]; rb[3 * q + 2] = row1[q];
  }
  std::vector<double> sigma((size_t)147 * std::max(n, 1));
  int rc = cov_blocks("gate_edges", true, true, lambda, 3 * n, ra.data(), rb.data(), sigma.data(), err);
  if (rc || n == 0) return rc;
  const size_t m = (size_t)n;
  // one device buffer: measurements (8 m), Sigma (147 m), Omega^-1 (49 m), then e (7 m), S (49 m), d2 (m)
  DevBuf<double> d_buf;
  DevBuf<int32_t> d_v;
  std::vector<double> res(57 * m);
  auto body = [&]() -> int {
    HIPCHK(d_buf.alloc(261 * m));
    HIPCHK(d_v.alloc(2 * m));
    double *d_meas_c = d_buf, *d_sigma = d_buf + 8 * m, *d_oi = d_buf + 155 * m, *d_e = d_buf + 204 * m,
           *d_S = d_buf + 211 * m, *d_d2 = d_buf + 260 * m;
    static_assert(sizeof(Sim3) == 8 * sizeof(double), "Sim3 is eight doubles");
    HIPCHK(hipMemcpyAsync(d_sigma, sigma.data(), sizeof(double) * 147 * m, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_oi, infoinv, sizeof(double) * 49 * m, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_meas_c, meas, sizeof(Sim3) * m, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_v, v0, sizeof(int32_t) * m, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_v + m, v1, sizeof(int32_t) * m, hipMemcpyHostToDevice, stream));
    GateArgs G{n, d_v, d_v + m, reinterpret_cast<const Sim3*>(d_meas_c), d_sigma, d_oi, d_states, mopts(),
               opt.jacobians, opt.dof_mask, opt.fd_delta, d_e, d_S, d_d2};
    hipLaunchKernelGGL(k_gate_edges, dim3((n + WG - 1) / WG), dim3(WG), 0, stream, G);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(res.data(), d_e, sizeof(double) * 57 * m, hipMemcpyDeviceToHost, stream));
    return SIM3OPT_OK;
  };
  rc = body();
  const hipError_t es = hipStreamSynchronize(stream);  // (the copies and the launch are done before the blocks go)
  if (rc) return rc;
  HIPCHK(es);
  for (size_t k = 0; k < 57 * m; ++k)
    if (!std::isfinite(res[k])) {
      err = "gate_edges: the innovation covariance J Sigma J^T + Omega^-1 of a candidate is not positive definite";
      return SIM3OPT_ERR_STATE;
    }
  std::memcpy(e_out, res.data(), sizeof(double) * 7 * m);
  std::memcpy(S_out, res.data() + 7 * m, sizeof(double) * 49 * m);
  std::memcpy(d2_out, res.data() + 56 * m, sizeof(double) * m);
  return SIM3OPT_OK;
}

// ---- diagnostic read-out of the factorisation (include/sim3opt.h, sim3opt_debug_factor) ----
// The launches are BlockLdl's own -- gather, factor, selinv -- on scratch copies of injected values, with a fail word,
// a singular flag, an x and a max |H_dd| of the call's own: d_vals, d_b, d_x, the DevScalars, fail_token, the cached
// chi2, kt and the schedule counters are never written.  What the call does overwrite is the context's Aperm / bp (put
// back by a gather of the real system after injected values) and its L, Dinv, y, xp, Z, which every user recomputes
// before reading them.
int Engine::debug_factor(int32_t context, double lambda, const double* vals, const double* b, bool with_solve,
                         bool with_selinv, double* Aperm, double* bp, double* L, double* Dinv, double* y, double* xp,
                         double* x, int32_t* fail, double* Z, int32_t* singular, int32_t* bord, int32_t* brow,
                         std::string& err) {
  const std::string pre = "debug_factor: ";
  if (comm.active()) {
    err = pre + "a partitioned graph holds this rank's share only (one GPU, please)";
    return SIM3OPT_ERR_STATE;
  }
  if (context != 0 && context != 1) {
    err = pre + "context must be 0 (the LM's solver) or 1 (the marginals')";
    return SIM3OPT_ERR_ARG;
  }
  if (context == 0 && with_selinv) {
    err = pre + "the selected inversion belongs to context 1 (the LM's factor has no plan for it)";
    return SIM3OPT_ERR_ARG;
  }
  if (!(lambda >= 0.0) || !(lambda < DBL_MAX)) {
    err = pre + "lambda must be finite and >= 0";
    return SIM3OPT_ERR_ARG;
  }
  if (context == 0 && !use_direct) {
    err = pre + "context 0 needs the exact solver (this graph's LM solves by PCG)";
    return SIM3OPT_ERR_STATE;
  }
  if ((!vals || !b) && !linearized) {
    err = pre + "call sim3opt_linearize (or optimize) first, or inject both vals and b";
    return SIM3OPT_ERR_STATE;
  }
  if (context == 1 && !marg_factor.ready()) {
    int rc = marginal_init(err);
    if (rc) return rc;
  }
  BlockLdl& F = context == 0 ? lm_factor : marg_factor;
  const DirectPlan& P = F.plan();
  HIPCHK(hipStreamSynchronize(stream));
  // scratch: [vals | b | x | max |H_dd| bits | fail, singular]
  const size_t nv = vals ? (size_t)49 * nnzb : 0, nbv = b ? (size_t)n : 0, nx = (size_t)n;
  DevBuf<double> d_buf;  // (declared before the body: it outlives debug_forget and the gather of the real system)
  HIPCHK(d_buf.alloc(nv + nbv + nx + 2));
  double *d_v = d_buf, *d_bb = d_buf + nv, *d_xs = d_bb + nbv;
  unsigned long long* d_bits = reinterpret_cast<unsigned long long*>(d_xs + nx);
  int32_t* d_flags = reinterpret_cast<int32_t*>(d_bits + 1);
  int32_t hflags[2] = {0, 0};
  unsigned long long hbits = 0;
  auto body = [&]() -> int {
    HIPCHK(hipMemsetAsync(d_xs, 0, sizeof(double) * (nx + 2), stream));
    if (vals) HIPCHK(hipMemcpyAsync(d_v, vals, sizeof(double) * nv, hipMemcpyHostToDevice, stream));
    if (b) HIPCHK(hipMemcpyAsync(d_bb, b, sizeof(double) * nbv, hipMemcpyHostToDevice, stream));
    const unsigned long long* bits_src = &d_sc->maxdiag_bits;
    if (with_selinv && vals) {
      // max |H_dd| of the injected diagonal blocks (the first block of a row), as k_diag_reduce would report it
      double m = 0.0;
      for (int32_t i = 0; i < nb; ++i)
        for (int d = 0; d < 7; ++d) m = std::max(m, std::fabs(vals[(size_t)49 * st.rowptr[i] + 8 * d]));
      std::memcpy(&hbits, &m, sizeof(double));
      HIPCHK(hipMemcpyAsync(d_bits, &hbits, sizeof(hbits), hipMemcpyHostToDevice, stream));
      bits_src = d_bits;
    }
    HIPCHK(hipStreamSynchronize(stream));  // (the uploads read the caller's and this frame's memory)
    F.gather(vals ? d_v : d_vals, b ? d_bb : d_b, stream);
    HIPCHK(F.factor(lambda, d_flags, 1, with_solve ? d_xs : nullptr, stream));
    if (with_selinv) {
      F.selinv(bits_src, d_flags + 1, stream, true);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(F.debug_read(Aperm, bp, L, Dinv, y, with_solve ? xp : nullptr, with_selinv ? Z : nullptr));
    if (with_solve) HIPCHK(hipMemcpy(x, d_xs, sizeof(double) * nx, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hflags, d_flags, sizeof(hflags), hipMemcpyDeviceToHost));
    return SIM3OPT_OK;
  };
  int rc = body();
  // the argument blocks point into the scratch buffer: forget that before it goes (every user sets the pointers
  // again -- gather, factor, selinv -- before it launches) ...
  const hipError_t es = hipStreamSynchronize(stream);
  F.debug_forget();
  // ... and the context starts every later trial from the real system's blocks again
  if ((vals || b) && linearized && es == hipSuccess) {
    F.gather(d_vals, d_b, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (rc == SIM3OPT_OK) HIPCHK(e2);
  }
  if (rc) return rc;
  *fail = hflags[0];
  if (with_selinv) *singular = hflags[1];
  if (bord) std::memcpy(bord, P.bord.data(), sizeof(int32_t) * P.bord.size());
  if (brow) std::memcpy(brow, P.brow.data(), sizeof(int32_t) * P.brow.size());
  return SIM3OPT_OK;
}

int engine_debug_factor_dims(Engine* e, int32_t context, int32_t* nb, int64_t* nL, int64_t* nnzb, std::string& err) {
  if (e->comm.active()) {
    err = "debug_factor_dims: a partitioned graph holds this rank's share only (one GPU, please)";
    return SIM3OPT_ERR_STATE;
  }
  if (context != 0 && context != 1) {
    err = "debug_factor_dims: context must be 0 (the LM's solver) or 1 (the marginals')";
    return SIM3OPT_ERR_ARG;
  }
  if (context == 0 && !e->use_direct) {
    err = "debug_factor_dims: context 0 needs the exact solver (this graph's LM solves by PCG)";
    return SIM3OPT_ERR_STATE;
  }
  if (context == 1 && !e->marg_factor.ready()) {
    int rc = e->marginal_init(err);
    if (rc) return rc;
  }
  const DirectPlan& P = (context == 0 ? e->lm_factor : e->marg_factor).plan();
  *nb = P.nb;
  *nL = P.nL;
  *nnzb = e->nnzb;
  return SIM3OPT_OK;
}

int engine_debug_factor(Engine* e, int32_t context, double lambda, const double* vals, const double* b, bool with_solve,
                        bool with_selinv, double* Aperm, double* bp, double* L, double* Dinv, double* y, double* xp,
                        double* x, int32_t* fail, double* Z, int32_t* singular, int32_t* bord, int32_t* brow,
                        std::string& err) {
  return e->debug_factor(context, lambda, vals, b, with_solve, with_selinv, Aperm, bp, L, Dinv, y, xp, x, fail, Z,
                         singular, bord, brow, err);
}

int engine_marginals(Engine* e, double lambda, int32_t n, const int32_t* row_a, const int32_t* row_b, double* cov,
                     std::string& err) {
  return e->marginals(lambda, n, row_a, row_b, cov, err);
}

int engine_covariances(Engine* e, double lambda, int32_t n, const int32_t* row_a, const int32_t* row_b, double* cov,
                       std::string& err) {
  return e->cov_blocks("covariances", true, false, lambda, n, row_a, row_b, cov, err);
}

void engine_covariance_stats(const Engine* e, int64_t out[6]) {
  for (int k = 0; k < 6; ++k) out[k] = e->cov_stats[k];
}

int engine_gate_edges(Engine* e, double lambda, int32_t n, const int32_t* v0, const int32_t* v1, const int32_t* row0,
                      const int32_t* row1, const sim3::Sim3* meas, const double* infoinv, double* e_out, double* S_out,
                      double* d2_out, std::string& err) {
  return e->gate_edges(lambda, n, v0, v1, row0, row1, meas, infoinv, e_out, S_out, d2_out, err);
}

}  // namespace sim3opt
