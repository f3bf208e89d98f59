// engine_pcg.hip -- preconditioned CG on (H + lambda I) x = b (LinearSolverEigen::solve, kitti_surf.cpp:553-554, on graphs
// too large to factor) and the halo exchange of its row-partitioned form.  ONE driver, Engine::pcg_run, handed the
// PcgView of the systems it works on: the engine's own vectors and scalars (pcg_attempt: one system, K = 1 of every
// kernel) or the buffers of batch_alloc (pcg_batch: up to KB systems in lock-step, per system the same operations
// in the same order, so its solutions are bit for bit those of sequential solves).
#include "engine_impl.hpp"

namespace sim3opt {

#include "spmv_kernel.hpp"
#include "pcg_kernels.hpp"

void Engine::jacobi(int lo, int hi, const int32_t* rowptr, double* vals, double lambda, double* Minv, double omega,
                    const double* diagH, const double* W, float* vals32, DevScalars* sc, double* diag64_out,
                    float* diag32_out) {
  hipLaunchKernelGGL(k_jacobi, dim3(std::max(1, (hi - lo + WG - 1) / WG)), dim3(WG), 0, stream, lo, hi, rowptr, vals,
                     lambda, Minv, sc ? sc : d_sc, omega, diagH, W, vals32, diag64_out, diag32_out);
}

// ||r||^2 and ||b||^2 over this rank's rows into out2[0..1] (device; fixed summation order)
void Engine::norms2(const double* r, const double* b, double* part_a, double* part_b, double* out2) {
  const int gn = grid_for(7 * (int64_t)(r1 - r0), WG);
  hipLaunchKernelGGL(k_norms2, dim3(gn), dim3(WG), 0, stream, 7 * r0, 7 * r1, r, b, part_a, part_b);
  hipLaunchKernelGGL(k_final_sum2<1>, dim3(1), dim3(WG), 0, stream, (const double*)part_a, (const double*)part_b, gn, 0,
                     out2, 0);
}

// Partition of level l and its exchange plan (see LevelPart).
int Engine::level_part_init(int l, int32_t nb_l, const int32_t* rowptr_l, const int32_t* colidx_l,
                            const std::vector<int32_t>& row_begin_l, std::string& err) {
  LevelPart& lp = parts[l];
  lp.row_begin = row_begin_l;
  lp.lo = row_begin_l[comm.rank];
  lp.hi = row_begin_l[comm.rank + 1];
  lp.offs.resize(comm.world + 1);
  lp.blk_offs.resize(comm.world + 1);
  for (int r = 0; r <= comm.world; ++r) {
    lp.offs[r] = 7 * (int64_t)row_begin_l[r];
    lp.blk_offs[r] = 49 * (int64_t)rowptr_l[row_begin_l[r]];
  }
  if (!opt.halo_exchange || !comm.can_exchange()) return SIM3OPT_OK;
  std::vector<int32_t> srows, sseg, rrows, rseg;
  if (comm.world <= 1) {
    // one rank with forced collectives (the transport's self-test): a plan that sends a few of the rank's rows
    // to itself, so that pack -> grouped send / receive -> unpack run as they do between neighbours
    if (!comm.force) return SIM3OPT_OK;
    for (int32_t i = 0; i < std::min<int32_t>(nb_l, 64); ++i) srows.push_back(i);
    rrows = srows;
    sseg = {0, (int32_t)srows.size()};
    rseg = sseg;
    lp.self_test = true;
  } else {
    halo_plan(nb_l, rowptr_l, colidx_l, comm.world, row_begin_l.data(), comm.rank, srows, sseg, rrows, rseg);
  }
  lp.n_send = (int32_t)srows.size();
  lp.n_recv = (int32_t)rrows.size();
  // Neighbour exchange or whole-vector all-gather: decided from the boundary rows of ALL ranks, so that every
  // rank takes the same branch (a collective all ranks must enter alike).  A partition without locality --
  // insertion order of a graph that wanders -- has nearly every row on its boundary, towards nearly every
  // rank: the plain all-gather is cheaper then.
  {
    std::vector<int32_t> brows, bseg;
    boundary_rows(nb_l, rowptr_l, colidx_l, comm.world, row_begin_l.data(), brows, bseg);
    lp.neighbour = lp.self_test || 4 * (int64_t)brows.size() < 3 * (int64_t)nb_l;
  }
  if (opt.verbose)
    std::fprintf(stderr, "sim3opt: rank %d of %d, level %d: rows [%d, %d) of %d; sends %d rows, receives %d: %s\n",
                 comm.rank, comm.world, l, lp.lo, lp.hi, nb_l, lp.n_send, lp.n_recv,
                 lp.neighbour ? "neighbour exchange" : "whole-vector all-gather");
  if (!lp.neighbour) return SIM3OPT_OK;
  lp.send_offs.resize(comm.world + 1);
  lp.recv_offs.resize(comm.world + 1);
  for (int r = 0; r <= comm.world; ++r) {
    lp.send_offs[r] = 7 * (int64_t)sseg[r];
    lp.recv_offs[r] = 7 * (int64_t)rseg[r];
  }
  HIPCHK(upload(lp.d_send, srows));
  HIPCHK(upload(lp.d_recv, rrows));
  HIPCHK(mem.raw(lp.d_sbuf, 7 * std::max<size_t>(srows.size(), 1)));
  HIPCHK(mem.raw(lp.d_rbuf, 7 * std::max<size_t>(rrows.size(), 1)));
  return SIM3OPT_OK;
}

// every rank's copy of `vec` (a vector of level l) gets the entries of the foreign rows its own rows' blocks
// refer to: packed, sent to exactly the ranks that read them, unpacked (two ~5 us launches around the grouped
// send / receive) -- or the all-gather of the whole vector where no neighbour plan applies
int Engine::exchange_level(int l, double* vec, std::string& err) {
  if (!comm.active() || l >= n_sharded) return SIM3OPT_OK;
  LevelPart& lp = parts[l];
  if (!lp.neighbour) return comm.allgatherv(vec, lp.offs, stream, err);
  if (lp.n_send > 0)
    hipLaunchKernelGGL(k_rows_gather, dim3((7 * lp.n_send + WG - 1) / WG), dim3(WG), 0, stream, lp.n_send,
                       (const int32_t*)lp.d_send, (const double*)vec, lp.d_sbuf);
  int rc = comm.exchange(lp.d_sbuf, lp.send_offs, lp.d_rbuf, lp.recv_offs, stream, err);
  if (rc) return rc;
  if (lp.n_recv > 0)
    hipLaunchKernelGGL(k_rows_scatter, dim3((7 * lp.n_recv + WG - 1) / WG), dim3(WG), 0, stream, lp.n_recv,
                       (const int32_t*)lp.d_recv, (const double*)lp.d_rbuf, vec);
  if (lp.self_test) return comm.allgatherv(vec, lp.offs, stream, err);  // (one rank: both transports' paths)
  return SIM3OPT_OK;
}

// q = (H + lambda I) v; partials of v.q in d_part_a and, with rvec, of rvec.v in d_part_b
// With a start/stop event pair the dispatch itself is timestamped (hipExtLaunchKernelGGL):
// no extra barrier packets, so the figure agrees with rocprofv3's kernel trace.
void Engine::spmv_raw(double lambda, const double* v, double* q, const double* rvec, DevScalars* scp,
              hipEvent_t ev0, hipEvent_t ev1) {
  const int g = spmv_grid();
#define SPAN_CASE(CH, NTV)                                                                       \
hipExtLaunchKernelGGL((k_spmv_span<CH, NTV, 0>), dim3(g), dim3(WG), 0, stream, ev0, ev1, 0, nb, \
                      d_wrow, d_rowptr, d_colidx, d_vals, v, q, lambda, d_part_a, rvec,         \
                      d_part_b, scp, (const double*)nullptr, 1, (const int32_t*)nullptr, 1.0, BatchStrides{0, 0, 0, 0, 0}, (const float*)nullptr)
#define SPAN_PLAIN(CH, NTV)                                                                     \
hipLaunchKernelGGL((k_spmv_span<CH, NTV, 0>), dim3(g), dim3(WG), 0, stream, nb, d_wrow,       \
                   d_rowptr, d_colidx, d_vals, v, q, lambda, d_part_a, rvec, d_part_b, scp,     \
                   (const double*)nullptr, 1, (const int32_t*)nullptr, 1.0, BatchStrides{0, 0, 0, 0, 0}, (const float*)nullptr)
  if (!ev0) {  // plain launch: capturable into a hipGraph
    if (spmv_chunk <= 4) { if (spmv_nt) SPAN_PLAIN(4, true); else SPAN_PLAIN(4, false); }
    else { if (spmv_nt) SPAN_PLAIN(8, true); else SPAN_PLAIN(8, false); }
    return;
  }
  if (spmv_chunk <= 4) { if (spmv_nt) SPAN_CASE(4, true); else SPAN_CASE(4, false); }
  else { if (spmv_nt) SPAN_CASE(8, true); else SPAN_CASE(8, false); }
#undef SPAN_PLAIN
#undef SPAN_CASE
}

// the PCG's SpMV on the first `live` systems of a view: w = A v, the partials of w.v (and rvec.v)
int Engine::pcg_spmv(const PcgView& V, int live, const double* v, const double* rvec, bool timed, std::string& err) {
  if (!V.batch) {
    hipEvent_t a = nullptr, b = nullptr;
    if (timed && opt.time_kernels) {
      int rc = pool_get(a, b, err);
      if (rc) return rc;
    }
    spmv_raw(V.lam[0], v, V.q, rvec, V.sc, a, b);
    return SIM3OPT_OK;
  }
  const BatchStrides bs{V.vs, V.ms, 0, 0, V.pstride};  // (the dampings travel in V.sc)
  BATCH_DISPATCH(live, hipLaunchKernelGGL((k_spmv_span<8, true, 0, double, KS, false>), dim3(span_grid), dim3(WG), 0, stream,
                     nb, d_wrow, d_rowptr, d_colidx, (const double*)d_vals, v, V.q, 0.0, V.part_a, rvec, V.part_b, V.sc,
                     (const double*)nullptr, 1, (const int32_t*)nullptr, 1.0, bs, (const float*)nullptr));
  return SIM3OPT_OK;
}

// k_final_sum2 leaves [w.z, r.z] of system s in sc[s].tmp_pq, tmp_rz: out2 = &sc->tmp_pq, this many doubles apart
constexpr int SC_DOUBLES = (int)(sizeof(DevScalars) / sizeof(double));
static_assert(sizeof(DevScalars) % sizeof(double) == 0 &&
                  offsetof(DevScalars, tmp_rz) == offsetof(DevScalars, tmp_pq) + sizeof(double),
              "DevScalars: tmp_pq and tmp_rz adjacent, the struct a whole number of doubles");

int Engine::agree_on_fail(std::string& err) {  // multi-GPU: fail on any rank = fail on all
  hipLaunchKernelGGL(k_fail_to_double, dim3(1), dim3(1), 0, stream, d_sc);
  int rc = comm.allreduce(&d_sc->tmp_pq, 1, 1, stream, err);
  if (rc) return rc;
  hipLaunchKernelGGL(k_double_to_fail, dim3(1), dim3(1), 0, stream, d_sc);
  return SIM3OPT_OK;
}

int Engine::pcg(double lambda, int32_t* iters, double* rel_res, bool* ok, std::string& err) {
  last_capped = false;
  if (use_direct) {  // exact step; `ok` is settled later from d_sc->fail (see optimize)
    *iters = 0;
    *rel_res = 0.0;
    *ok = true;
    return direct_solve(lambda, err);
  }
  *iters = 0;
  int32_t probe_iters = 0;  // iterations of an abandoned block-Jacobi probe: work done, reported
  if (use_amg && adaptive_prec) {
    // damping-dominated system?  (see adaptive_prec above)
    if (trace_stale) {
      int rc = fetch_scalars(err);
      if (rc) return rc;
      mean_diag = n > 0 ? h_sc->trace / (double)n : 0.0;
      trace_stale = false;
    }
    const double gate = bj_gate >= 0.0 ? bj_gate : 0.05 * mean_diag;
    if (mean_diag > 0.0 && lambda >= gate) {
      bool abandoned = false;
      int rc = pcg_attempt(lambda, 0, iters, rel_res, ok, nullptr, err, bj_budget, &abandoned);
      if (rc) return rc;
      if (opt.verbose >= 2)
        std::fprintf(stderr, "  lambda %.3g >= %.3g (mean |H_dd| %.3g): block-Jacobi first: %s after %d iterations\n",
                     lambda, gate, mean_diag, abandoned ? "abandoned" : "done", *iters);
      if (!abandoned) {
        ++n_bj_solves;
        if (*ok && *iters <= bj_budget / 4) bj_gate = std::min(gate, 0.5 * lambda);
        else bj_gate = std::min(gate, lambda);
        return SIM3OPT_OK;
      }
      ++n_bj_abandoned;
      probe_iters = *iters;
      bj_gate = 2.0 * lambda;  // not before the damping has doubled
    }
  }
  if (use_amg || use_chain) {
    // the block-tridiagonal factorisation (or the multigrid's coarsest-level inverse) can meet a
    // non-positive pivot when H is numerically semi-definite (cond ~1e12 in the reference's
    // as-written arithmetic): retry with block-Jacobi
    bool broke = false;
    int rc = pcg_attempt(lambda, use_amg ? 2 : 1, iters, rel_res, ok, &broke, err);
    if (rc) return rc;
    *iters += probe_iters;
    probe_iters = 0;
    // A CG breakdown (r.z < 0, p.Ap <= 0) or a residual that is not small although the M^-1 norm
    // says so, with the over-corrected cycle: the over-correction is safe only while the (inexact)
    // coarse solves stay within (0, 2) of the exact ones -- measured on config 3: 1.8 / 1.6 always,
    // 1.9 / 1.7 not.  Before blaming the system (and making LM reject the trial), solve again with
    // the plain cycle; keep it if that was the cure.
    if (use_amg && !broke && amg_over_on && (!*ok || last_true_rel > 1e-3)) {
      if (opt.verbose)
        std::fprintf(stderr, "sim3opt: multigrid PCG broke down (ok %d, ||r||/||b|| %.1e): again without over-correction\n",
                     (int)*ok, last_true_rel);
      amg_over_on = false;
      pcg_graph_kind = -1;  // (a captured iteration has the factors baked into its launches)
      const int32_t spent = *iters;
      rc = pcg_attempt(lambda, 2, iters, rel_res, ok, &broke, err);
      if (rc) return rc;
      *iters += spent;
      if (!*ok) {  // not the preconditioner's fault: the system is not positive definite
        amg_over_on = true;
        pcg_graph_kind = -1;
      }
    }
    if (!broke) return SIM3OPT_OK;
  }
  {
    const int32_t spent = *iters;  // (of a preconditioner whose set-up met a non-positive pivot)
    int rc = pcg_attempt(lambda, 0, iters, rel_res, ok, nullptr, err);
    *iters += spent;
    return rc;
  }
}

// prec: 0 block-Jacobi, 1 chain segments, 2 aggregation multigrid
// probe_budget > 0 (block-Jacobi tried first on a damping-dominated system): after 8 iterations the
// reduction reached so far predicts the total; if that exceeds the budget -- or the budget runs out --
// *abandoned is set and the caller solves again with the hierarchy
// rhs, rel_tol: another right-hand side and tolerance than d_b and options.pcg_rel_tol (the columns of the inverse)
int Engine::pcg_attempt(double lambda, int prec, int32_t* iters, double* rel_res, bool* ok, bool* chain_broke,
                        std::string& err, int probe_budget, bool* abandoned, const double* rhs, double rel_tol) {
  PcgView& V = pv_one;
  V.nsys = 1;
  V.lam[0] = lambda;
  V.tol[0] = rhs ? rel_tol : opt.pcg_rel_tol;
  V.b = rhs ? rhs : d_b;
  const DevScalars& h = *h_sc;
  bool broke = false;
  int rc = pcg_run(V, prec, 1, prec == 2, &broke, err, probe_budget, abandoned);
  if (rc) return rc;
  if (broke) {
    if (opt.verbose)
      std::fprintf(stderr, "sim3opt: %s set-up met a non-positive pivot (lambda %.3g): block-Jacobi for this solve\n",
                   prec == 2 ? "multigrid" : "chain", lambda);
    if (chain_broke) *chain_broke = true;
    *ok = false;
    *iters = 0;
    *rel_res = 0.0;
    return SIM3OPT_OK;
  }
  *iters = h.iter;
  *rel_res = h.rel_res();
  *ok = !h.fail;
  if (abandoned && *abandoned) return SIM3OPT_OK;  // (the probe ran out of budget, or is predicted to)
  last_true_rel = prec == 2 && !h.fail ? h.true_rel() : 0.0;
  if (prec == 2 && !h.fail && opt.verbose)
    std::fprintf(stderr, "sim3opt: multigrid PCG: %d iterations, ||r||_Minv ratio %.2e, ||r||_2 / ||b||_2 %.2e\n", h.iter,
                 *rel_res, last_true_rel);
  // stopped by the cap, not by the tolerance: an inexact step (sim3opt_iter_stats::pcg_capped); LM's gain
  // ratio decides what becomes of it -- the exact solver it stands in for has no such state
  last_capped = h.capped(V.tol[0]);
  return SIM3OPT_OK;
}

// Solves (H + lams[s] I) x_s = b, s < nsys <= KB, together; x_s is left in b_x + s * b_vs.  *usable = false:
// some system broke down or failed the true-residual check -- the caller then solves the trials one by one
// (the sequential path has the fall-backs: plain cycle instead of the over-corrected one, block-Jacobi).
// cols (columns of the inverse, engine_columns.hip): system s solves for ITS right-hand side cols->g + s * stride to
// its own tolerance, all at lams[0] -- so ONE set-up (smoother inverses, FP32 diagonals, dense coarsest inverse: slot
// 0, the caller has set the per-system strides of the batch's views to 0) serves them all, and the batches of a call
// that follow the first (cols->setup false) run none.  The 2-norm check is the caller's, on the true residual.
int Engine::pcg_batch(const double* lams, int nsys, int32_t* iters, double* rel_res, bool* capped, bool* usable,
                      std::string& err, const BatchRhs* cols) {
  *usable = false;
  int rc = batch_alloc(err);
  if (rc) return rc;
  PcgView& V = pv_batch;
  V.nsys = nsys;
  for (int s = 0; s < KB; ++s) {
    V.tol[s] = cols ? cols->tol[std::min(s, nsys - 1)] : opt.pcg_rel_tol;
    V.lam[s] = lams[std::min(s, nsys - 1)];
  }
  V.b = cols ? cols->g : d_b;
  V.bstride = cols ? cols->stride : 0;
  bool broke = false;
  rc = pcg_run(V, 2, cols ? (cols->setup ? 1 : 0) : nsys, !cols, &broke, err);
  if (rc || broke) return rc;  // (a non-positive pivot of some set-up: not usable)
  bool good = true;
  for (int s = 0; s < nsys; ++s) {
    const DevScalars& h = h_bsc[s];
    const double true_rel = cols ? 0.0 : h.true_rel();
    if (h.fail || true_rel > 1e-3) good = false;
    iters[s] = h.iter;
    rel_res[s] = h.rel_res();
    capped[s] = h.capped(V.tol[s]);
    if (opt.verbose)
      std::fprintf(stderr, "sim3opt: batched multigrid PCG, system %d of %d: lambda %.6g, %d iterations, ||r||_Minv ratio %.2e, "
                   "||r||_2 / ||b||_2 %.2e\n", s, nsys, lams[s], h.iter, rel_res[s], true_rel);
  }
  kt.n_batched_solves += nsys;
  kt.n_batches += 1;
  *usable = good;
  return SIM3OPT_OK;
}

// the numbers of preconditioner `prec` at the dampings V.lam (a batch: for its first nsetup systems)
int Engine::pcg_setup(PcgView& V, int prec, int nsetup, std::string& err) {
  const int nloc = r1 - r0, nseg = (nloc + chain_seg - 1) / chain_seg;
  if (prec == 2) {
    if (amg_stale) {
      int rc = amg_setup(err);
      if (rc) return rc;
    }
    if (V.batch) batch_prepare(nsetup);
    else amg_prepare(V.lam[0]);
  } else if (prec == 1) {
    hipLaunchKernelGGL(k_chain_factor, dim3(std::max(1, (nseg + 63) / 64)), dim3(64), 0, stream, r0, r1, chain_seg,
                       d_rowptr, d_vals, d_sub_first, d_sub_cnt, V.lam[0], V.Minv, d_Gm, V.sc);
  } else {
    hipLaunchKernelGGL(k_jacobi, dim3(std::max(1, (nloc + WG - 1) / WG)), dim3(WG), 0, stream, r0, r1, d_rowptr,
                       d_vals, V.lam[0], V.Minv, V.sc, 1.0, (const double*)nullptr, (const double*)nullptr);
  }
  return SIM3OPT_OK;
}

// The solve (see engine_impl.hpp).  prec: 0 block-Jacobi, 1 chain segments, 2 aggregation multigrid.
int Engine::pcg_run(PcgView& V, int prec, int nsetup, bool check_true, bool* setup_broke, std::string& err,
                    int probe_budget, bool* abandoned) {
  const bool use_chain = prec == 1, use_mg = prec == 2;
  const bool probe = probe_budget > 0;
  const int nsys = V.nsys;
  DevScalars* const h0 = V.h_sc;  // (system 0: the one system, or the batch's first)
  double* const zin = use_mg ? V.az : V.z;  // preconditioned residual the PCG consumes
  // r.z: from the SpMV's own pass over r -- or, with the multiplicative multigrid cycle, from the
  // cycle's last kernel, which holds r and writes z (the SpMV then skips its load of r)
  const double* const spmv_r = use_mg && !amg_additive ? nullptr : V.r;
  const int nloc = r1 - r0;
  const int gv = grid_for((nloc + 8) / 9, 4);  // 36 block rows per workgroup pass
  const int gs = spmv_grid();
  const bool multi = comm.active();
  // [w.z, r.z] summed once by k_final_sum2 (multi-GPU: then all-reduced) instead of by every
  // workgroup of the PCG step when the SpMV leaves more partials than a workgroup sums for free; a batch always
  const bool pre_sum = V.batch || multi || gs > MAX_GRID;
  const double* const part_d = pre_sum ? nullptr : V.part_a;
  const double* const part_g = pre_sum ? nullptr : V.part_b;
  const BatchStrides bs{V.vs, V.ms, 0, 0, V.pstride};
  *setup_broke = false;
  // automatic cap: small systems may need ~n iterations for an (almost) exact step like the
  // reference's Cholesky (chains are ill-conditioned); large ones get a truncated-Newton budget
  // (round 3: a cap of 4000 for the multigrid path was tried for the one system in twenty of the
  // as-written arithmetic on config 3 that stops at 1000 -- it stops at 4000 as well, relative residual
  // 2e-3: numerically indefinite without a detectable breakdown; the cap stays)
  int max_it = opt.pcg_max_iters > 0 ? opt.pcg_max_iters
                                     : (n <= 50000 ? std::max(100, 2 * n) : 1000);
  if (probe) max_it = std::min(max_it, probe_budget);
  const int nseg = (nloc + chain_seg - 1) / chain_seg;
  const int gc = grid_for(nseg, 4);  // chain apply: one wavefront per segment
  const double* Minv_arg = use_chain ? nullptr : V.Minv;
  int rc = SIM3OPT_OK;
  for (int s = 0; s < V.nsc; ++s) {
    DevScalars& h = V.h_sc[s];
    if (V.batch) std::memset(&h, 0, sizeof(DevScalars));
    h.rz[0] = h.rz[1] = h.alpha[0] = h.alpha[1] = h.rz0 = 0.0;
    h.iter = 0;
    h.max_iter = max_it;
    h.done = s < nsys ? 0 : 1;  // (an unused slot: finished from the start, its vectors stay zero)
    h.stop = h.fail = 0;
    h.tol2 = V.tol[s] * V.tol[s];
    h.lambda = V.lam[s];
  }
  if (V.batch) {
    HIPCHK(hipMemcpyAsync(V.sc, V.h_sc, sizeof(DevScalars) * V.nsc, hipMemcpyHostToDevice, stream));
  } else {
    // chi2 / scale / maxdiag live in the same struct: only the PCG fields are reset
    HIPCHK(hipMemcpyAsync(&V.sc->rz[0], &h0->rz[0], offsetof(DevScalars, chi2), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(&V.sc->iter, &h0->iter, offsetof(DevScalars, tmp_pq) - offsetof(DevScalars, iter),
                          hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(&V.sc->lambda, &h0->lambda, sizeof(double), hipMemcpyHostToDevice, stream));
  }
  rc = pcg_setup(V, prec, nsetup, err);
  if (rc) return rc;
  if (V.cv) V.cv->nsys = nsys;
  if (V.bstride)
    BATCH_DISPATCH(nsys, hipLaunchKernelGGL((k_pcg_init<KS, true>), dim3(gv), dim3(WG), 0, stream, r0, r1, V.b, Minv_arg,
                       V.x, V.r, V.z, V.p, V.s, bs, V.bstride));
  else
    BATCH_DISPATCH(nsys, hipLaunchKernelGGL((k_pcg_init<KS, false>), dim3(gv), dim3(WG), 0, stream, r0, r1, V.b, Minv_arg,
                       V.x, V.r, V.z, V.p, V.s, bs, (int64_t)0));
  // z = M^-1 r beyond the block-Jacobi part the step has written; sc: launches after `done` return at once
  auto apply_prec = [&](const DevScalars* sc) -> int {
    if (use_chain)
      hipLaunchKernelGGL(k_chain_apply, dim3(gc), dim3(WG), 0, stream, r0, r1, chain_seg, V.Minv, d_Gm, V.r, V.z, sc);
    if (use_mg && V.batch) amg_cycle(*V.cv, 0, V.z, V.az);
    else if (use_mg) return amg_apply(err);  // (one system: several ranks' exchanges are in there)
    return SIM3OPT_OK;
  };
  if (use_chain || use_mg) {
    if (multi) {
      rc = agree_on_fail(err);
      if (rc) return rc;
    }
    rc = fetch_scalars(V, err);  // did the factorisation succeed?
    if (rc) return rc;
    for (int s = 0; s < nsys; ++s)
      if (V.h_sc[s].fail) {
        *setup_broke = true;
        return SIM3OPT_OK;
      }
    rc = apply_prec(nullptr);
    if (rc) return rc;
  }
  HIPCHK(hipGetLastError());
  if (multi && !use_mg) {  // (the multigrid cycle gathers its own operands)
    rc = exchange_rows(V.z, err);
    if (rc) return rc;
  }
  // Iterations per look into DevScalars.  Without a rate -- the first chunk of a solve, pcg_check_every = 1, the
  // probe, several ranks (their collectives need the same count on every rank) -- a fixed number: pcg_check_every,
  // for the multigrid at most 4 (an iteration is ~1 ms of GPU work and its coarse launches run even after `done`).
  // With one (PcgRate) the share sched_frac of the iterations still predicted, at most `cap`: long chunks while the
  // end is far, single iterations next to it.  The prediction sizes chunks and nothing else: `done`, `stop` and
  // `fail` are raised on the device, a wrong guess costs a poll or an idle iteration.
  const int pce = std::max(1, opt.pcg_check_every);
  const int chunk = use_mg ? std::min(4, pce) : (probe ? 8 : pce);
  const bool predict = !multi && !probe && pce > 1;
  const int cap = use_mg ? (pce >= 4 ? std::min(pce, std::max(4, sched_cap_mg)) : pce) : pce;
  int it = 0, par = 0;
  int live = V.batch ? nsys : 1;  // systems the launches carry: [0, live)
  // the launches of one iteration up to the step, the one that decides (launch number itn; < 0: captured)
  auto iterate = [&](int parity, int itn, bool timed) -> int {
    int rc2 = pcg_spmv(V, live, zin, spmv_r, timed, err);
    if (rc2) return rc2;
    if (pre_sum)  // [w.z, r.z] -> tmp_pq, tmp_rz (adjacent) of every system
      BATCH_DISPATCH(live, hipLaunchKernelGGL((k_final_sum2<KS>), dim3(1), dim3(WG), 0, stream, (const double*)V.part_a,
                         (const double*)V.part_b, gs, V.pstride, &V.sc->tmp_pq, SC_DOUBLES));
    if (multi) {  // one 2-double all-reduce
      rc2 = comm.allreduce(&V.sc->tmp_pq, 2, 0, stream, err);
      if (rc2) return rc2;
    }
    BATCH_DISPATCH(live, hipLaunchKernelGGL((k_pcg_step<KS>), dim3(gv), dim3(WG), 0, stream, r0, r1, parity, itn, part_d,
                       part_g, gs, V.pstride, Minv_arg, (const double*)zin, V.z, (const double*)V.q, V.p, V.s, V.x, V.r,
                       V.sc, bs));
    return SIM3OPT_OK;
  };
  // Launch-bound regime (small graphs: two ~3 us kernels per iteration; one system): replay a captured
  // hipGraph of PCG_GRAPH_ITERS iterations instead of enqueueing them one by one.  The first
  // iteration stays eager (it carries it == 0); captured steps read the counter, the damping and
  // the stopping state from DevScalars, so one instantiated graph serves every solve.
  const bool graphed = !V.batch && !multi && !opt.time_kernels && opt.pcg_graph && max_it > PCG_GRAPH_ITERS && !probe;
  if (graphed && (!pcg_graph || pcg_graph_kind != prec)) {
    if (pcg_graph) { (void)hipGraphExecDestroy(pcg_graph); pcg_graph = nullptr; }
    // a multigrid iteration is ~20 launches: shorter graphs waste fewer no-op launches after
    // convergence
    graph_iters = use_mg ? 4 : PCG_GRAPH_ITERS;
    hipGraph_t gr = nullptr;
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    for (int c = 0; c < graph_iters; ++c) {  // (single GPU here: no collectives inside)
      (void)iterate((1 + c) & 1, -1, false);
      (void)apply_prec(V.sc);
    }
    {  // (a failed launch inside the region must not leave the stream capturing)
      const hipError_t le = hipGetLastError();
      const hipError_t ce = hipStreamEndCapture(stream, &gr);
      if (le != hipSuccess || ce != hipSuccess) {
        if (gr) (void)hipGraphDestroy(gr);
        err = std::string("PCG graph capture: ") + hipGetErrorString(le != hipSuccess ? le : ce);
        return SIM3OPT_ERR_HIP;
      }
    }
    HIPCHK(hipGraphInstantiate(&pcg_graph, gr, nullptr, nullptr, 0));
    (void)hipGraphDestroy(gr);
    pcg_graph_kind = prec;
  }
  // enqueues `count` iterations -- whole replays of the captured graph where it applies (then fewer than asked
  // for unless count is a multiple of graph_iters), one by one otherwise
  // A chunk ends with k_pcg_step, the launch that decides: z = M^-1 r of a chunk's last step (chain segments, the
  // multigrid cycle: ~0.3 ms of coarse launches that run whether the solve has finished or not) is enqueued at the
  // head of the next chunk -- so the step that finds the tolerance met is not followed by a cycle nobody reads.
  // (Several ranks: the cycle's collectives and the exchange of z stay where they were.)
  const bool defer_prec = !multi && (use_chain || use_mg);
  bool prec_pending = false;
  auto enqueue = [&](int count) -> int {
    if (prec_pending) {
      int rc2 = apply_prec(V.sc);
      if (rc2) return rc2;
      prec_pending = false;
    }
    if (graphed && it > 0 && par == 1 && count >= graph_iters) {
      // steps past max_iter cannot happen: the step that reaches it raises `stop`, and the
      // following launches of the replay are no-ops
      const int reps = count / graph_iters;
      for (int k = 0; k < reps; ++k) HIPCHK(hipGraphLaunch(pcg_graph, stream));
      it += reps * graph_iters;
      sched_stats[0] += reps * graph_iters;
      return SIM3OPT_OK;
    }
    for (int c = 0; c < count; ++c) {
      int rc2 = iterate(par, it, true);
      if (rc2) return rc2;
      if (defer_prec && c + 1 == count) {
        prec_pending = true;
      } else {
        rc2 = apply_prec(V.sc);
        if (rc2) return rc2;
      }
      if (multi && !use_mg) {  // the next SpMV gathers z from the neighbouring ranks
        rc2 = exchange_rows(V.z, err);
        if (rc2) return rc2;
      }
      par ^= 1;
      ++it;
    }
    sched_stats[0] += count;
    HIPCHK(hipGetLastError());
    return SIM3OPT_OK;
  };
  // the timed SpMV launches of the one-system solve (time_kernels: the event pool) are counted against the work
  // counter of the looks
  auto note_work = [&]() {
    if (!V.batch && !opt.time_kernels) spmv_work_seen = h0->n_spmv_work;
  };
  // a look with nothing queued behind it: the scalars are fresh and every recorded event complete
  auto poll_sync = [&]() -> int {
    int rc2 = fetch_scalars(V, err);
    if (rc2) return rc2;
    sched_stats[2] += 1;
    if (!V.batch && opt.time_kernels) return pool_drain(err);
    note_work();
    return SIM3OPT_OK;
  };
  // The captured graph starts at par == 1.  An eager chunk of several iterations on that path is cut by one where
  // it would end at par == 0, so that whole graphs can be replayed again should the prediction grow (single
  // iterations next to the end are left alone: two of them restore the parity).
  auto keep_parity = [&](int n) { return graphed && it > 0 && n > 1 && n < graph_iters && ((par ^ (n & 1)) == 0) ? n - 1 : n; };
  auto finished = [](const DevScalars& h) { return h.done || h.stop || h.fail; };
  PcgRate rate[KB];
  int seen = 0;  // iterations that were enqueued before the look V.h_sc holds (seen < it: chunks still in the queue)
  const int64_t enq0 = sched_stats[0];
  // The set-up's fetch above has just read the scalars and no step has run since: with a prediction to make up
  // for it the loop's first look is left out (it would only drain the queue the first cycle sits in).
  bool have = predict && (use_chain || use_mg);
  long long work0 = have ? h0->n_spmv_work : -1;
  if (have) note_work();
  for (;;) {
    if (!have) {
      rc = poll_sync();
      if (rc) return rc;
      seen = it;
    }
    have = false;
    if (work0 < 0) work0 = h0->n_spmv_work;
    // systems still iterating: [0, live).  The dampings of a batch ascend with the trial, so the systems finish from
    // the tail as a rule; the launches that follow carry the first `live` systems only (per system the same
    // operations whatever K is: the results do not depend on when the others finished)
    live = 0;
    for (int s = 0; s < nsys; ++s)
      if (!finished(V.h_sc[s])) live = s + 1;
    if (opt.verbose >= 3)
      for (int s = 0; s < nsys; ++s) {
        const DevScalars& h = V.h_sc[s];
        char who[40] = "  pcg look:";
        if (V.batch) std::snprintf(who, sizeof(who), "  batch look: system %d,", s);
        std::fprintf(stderr, "%s enqueued %d, seen %d, iter %d, r.z %.6e of %.6e (tol2 %.3e), done %d\n", who, it, seen,
                     h.iter, std::fabs(h.gam_last), h.rz0, h.tol2, h.done);
      }
    if (live == 0 || seen >= max_it) break;
    if (probe && it >= 8 && h0->rz0 > 0.0) {
      // squared M^-1-norm reduction after `it` iterations -> iterations to the tolerance at that rate
      const double ratio = std::fabs(h0->gam_last) / h0->rz0;
      const double need = ratio > 0.0 && ratio < 1.0 ? it * std::log(h0->tol2) / std::log(ratio) : 1e30;
      if (need > probe_budget) break;
    }
    // iterations predicted to be needed beyond the `it` enqueued, per system: a chunk ends where the first of the live
    // systems is predicted to finish -- so that `live` shrinks then and not up to three K-system iterations later
    double rem = -1.0;
    if (predict) {
      double xmin = DBL_MAX;
      for (int s = 0; s < live; ++s) {
        const DevScalars& h = V.h_sc[s];
        if (finished(h)) continue;
        rate[s].look(h.iter, h.rz0, h.gam_last);
        const double x = rate[s].remaining(h.tol2 * h.rz0);
        xmin = x < 0.0 ? -1.0 : std::min(xmin, x);
        if (x < 0.0) break;
      }
      if (xmin >= 0.0) rem = std::max(0.0, xmin - (double)(it - seen));
    }
    int todo = graphed && it == 0 ? 1 : std::min(sched_chunk(rem, chunk, cap), max_it - it);
    if (seen < it && (todo <= 0 || rem == 0.0)) continue;  // all that is predicted is in the queue: wait for it
    if (graphed && it > 0 && par == 1 && todo >= graph_iters) todo -= todo % graph_iters;
    todo = keep_parity(todo);
    if (V.batch) V.cv->nsys = live;
    rc = enqueue(todo);
    if (rc) return rc;
    // more than this chunk predicted: the look at it goes into a pinned slot and is waited for with the next
    // chunk in the queue
    int ahead = rem >= 0.0 ? std::min(sched_ahead(rem - todo, cap), max_it - it) : 0;
    if (graphed && par == 1 && ahead >= graph_iters) ahead -= ahead % graph_iters;
    ahead = keep_parity(ahead);
    if (ahead >= 2) {
      rc = poll_async(V.sc, V.nsc, err);
      if (rc) return rc;
      seen = it;
      rc = enqueue(ahead);
      if (rc) return rc;
      rc = poll_wait(V.h_sc, V.nsc, err);
      if (rc) return rc;
      note_work();
      have = true;
    }
  }
  // iterations enqueued that found the solve finished (V.h_sc: the last look of this solve; a batch: K-system
  // iterations that found every system finished)
  auto count_idle = [&]() {
    sched_stats[1] += std::max<int64_t>(0, (sched_stats[0] - enq0) - (int64_t)(h0->n_spmv_work - work0));
  };
  // stopped on a look that had a chunk queued behind it: the SpMV events are read once the stream has been waited for
  bool drain_late = !V.batch && opt.time_kernels && seen < it;
  if (probe && abandoned && !h0->done && !h0->fail) {  // (ran out of budget or predicted to)
    *abandoned = true;
    count_idle();
    kt.n_pcg_vec += h0->iter;
    return SIM3OPT_OK;
  }
  // The stopping test is in the M^-1 norm.  A multigrid cycle is symmetric by construction but
  // positive definite only within limits (over-correction, inexact coarse solves): should it
  // ever lose definiteness, r.z can vanish while r has not.  So the 2-norm of the (recursive)
  // residual is checked against ||b|| once per solve: two more small launches per system and one read-back.
  bool checked[KB] = {false, false, false, false}, any_checked = false;
  for (int s = 0; s < nsys; ++s) any_checked |= checked[s] = check_true && !V.h_sc[s].fail;
  if (drain_late && !any_checked) {
    HIPCHK(hipStreamSynchronize(stream));
    rc = pool_drain(err);
    if (rc) return rc;
    drain_late = false;
  }
  if (multi) {  // every rank updates its replica of all estimates
    rc = comm.allgatherv(V.x, offs, stream, err);  // (the whole step: every replica updates every estimate)
    if (rc) return rc;
    rc = agree_on_fail(err);
    if (rc) return rc;
    rc = fetch_scalars(V, err);
    if (rc) return rc;
  }
  if (any_checked || V.batch) {  // (a batch: this look always, checked or not)
    for (int s = 0; s < nsys; ++s)
      if (checked[s])
        norms2(V.r + (size_t)s * V.vs, V.b + (size_t)s * V.bstride, V.part_a, V.part_b, &V.sc[s].tmp_pq);
    HIPCHK(hipGetLastError());
    if (multi) {
      rc = comm.allreduce(&V.sc->tmp_pq, 2, 0, stream, err);
      if (rc) return rc;
    }
    rc = fetch_scalars(V, err);
    if (rc) return rc;
    if (drain_late) {
      rc = pool_drain(err);
      if (rc) return rc;
    }
  }
  count_idle();
  int it_max = 0;
  for (int s = 0; s < nsys; ++s) it_max = std::max(it_max, (int)V.h_sc[s].iter);
  kt.n_pcg_vec += it_max;
  return SIM3OPT_OK;
}

// ---- several right-hand sides at once: the rejected trials of one LM iteration (OptimizationAlgorithmLevenberg::solve,
// reached from kitti_surf.cpp:675) solve (H + lambda_k I) x_k = b for a known sequence lambda_k; after the first
// rejection the next ones are solved together -- one pass over the blocks for K vectors, K vectors per coarse launch --
// and evaluated in g2o's order (lm_trial_solve decides and hands them out).  The batch's buffers, the two views of them
// (pv_batch for pcg_run, cv_batch for the cycle of engine_amg.hip) and its per-system set-up ----
// buffers of the batched solve, allocated at its first use (single GPU, multigrid path)
int Engine::batch_alloc(std::string& err) {
  if (batch_ready) return SIM3OPT_OK;
  const int nl = (int)amg.size();
  // (schedule only -- the results do not depend on it: which levels run one system per grid slice)
  if (const char* ev = std::getenv("SIM3OPT_BATCH_SLICE_BLOCKS")) b_slice_blocks = std::atoll(ev);
  b_vs = pad64(n);
  double** v0[] = {&b_x, &b_r, &b_z, &b_p, &b_q, &b_s, &b_az};
  for (double** v : v0) HIPCHK(batch_mem.alloc(*v, (size_t)KB * b_vs, stream));
  // what the cycle (engine_amg.hip) works on for a batch: KB systems per level
  CycleView& V = cv_batch;
  V = CycleView();
  V.batch = true;
  V.lv.assign(nl, CycleLevel());
  for (int l = 0; l < nl; ++l) {
    CycleLevel& B = V.lv[l];
    const AmgLevel& L = amg[l];
    B.vs = l == 0 ? b_vs : pad64(7 * (int64_t)L.nb);
    B.ms = (int64_t)49 * L.nb;
    HIPCHK(batch_mem.alloc(B.Minv, (size_t)KB * B.ms, stream));
    if (l == 0) {
      B.r = b_r; B.x = b_z; B.t = b_az;
    } else {
      HIPCHK(batch_mem.alloc(B.r, (size_t)KB * B.vs, stream));
      HIPCHK(batch_mem.alloc(B.x, (size_t)KB * B.vs, stream));
      HIPCHK(batch_mem.alloc(B.t, (size_t)KB * B.vs, stream));
      HIPCHK(batch_mem.alloc(B.diag32, (size_t)KB * B.ms, stream));
    }
  }
  const size_t nc = (size_t)7 * amg[nl - 1].nb;
  b_as = (int64_t)(nc * nc);
  HIPCHK(batch_mem.alloc(b_Ainv, (size_t)KB * b_as, stream));
  HIPCHK(batch_mem.alloc(b_diag64, (size_t)KB * 49 * amg[nl - 1].nb, stream));
  HIPCHK(batch_mem.alloc(b_part_a, (size_t)KB * SPAN_GRID_MAX, stream));
  HIPCHK(batch_mem.alloc(b_part_b, (size_t)KB * SPAN_GRID_MAX, stream));
  HIPCHK(batch_mem.alloc(d_bsc, (size_t)KB, stream));
  HIPCHK(host_malloc((void**)&h_bsc, sizeof(DevScalars) * KB));
  V.sc = d_bsc;
  V.Ainv = b_Ainv;
  V.as = b_as;
  V.rz_part = b_part_b;
  V.part = SPAN_GRID_MAX;
  // ... and what the PCG (engine_pcg.hip) works on
  PcgView& P = pv_batch;
  P = PcgView();
  P.batch = true;
  P.nsc = KB;
  P.x = b_x; P.r = b_r; P.z = b_z; P.p = b_p; P.q = b_q; P.s = b_s; P.az = b_az;
  P.vs = b_vs;
  P.Minv = V.lv[0].Minv;
  P.ms = V.lv[0].ms;
  P.sc = d_bsc;
  P.h_sc = h_bsc;
  P.part_a = b_part_a;
  P.part_b = b_part_b;
  P.pstride = SPAN_GRID_MAX;
  P.cv = &cv_batch;
  batch_ready = true;
  return SIM3OPT_OK;
}

void Engine::batch_release() {
  batch_mem.release();
  if (h_bsc) host_free(h_bsc);
  h_bsc = nullptr;
  d_bsc = nullptr;
  cv_batch = CycleView();
  pv_batch = PcgView();
  batch_ready = false;
}

void Engine::batch_prepare(int nsetup) {
  const int nl = (int)amg.size();
  for (int s = 0; s < nsetup; ++s) {
    for (int l = 0; l < nl; ++l) {
      const AmgLevel& L = amg[l];
      const CycleLevel& B = cv_batch.lv[l];
      jacobi(0, L.nb, L.rowptr, L.vals, pv_batch.lam[s], B.Minv + (size_t)s * B.ms, amg_omega, L.diagH, L.W, nullptr,
             d_bsc + s, l == nl - 1 ? b_diag64 + (size_t)s * 49 * L.nb : nullptr,
             l > 0 ? B.diag32 + (size_t)s * B.ms : nullptr);
    }
    dense_inverse(b_diag64 + (size_t)s * 49 * amg[nl - 1].nb, b_Ainv + (size_t)s * b_as, d_bsc + s);
  }
}

// The solve of LM trial q at damping lambda; ni is the factor the next rejection applies.  After a rejection g2o's
// rule fixes the dampings of the next trials (lambda *= ni, ni *= 2 per rejection), so the systems of the trials
// that may follow are solved TOGETHER -- one pass over the blocks for all of them -- and handed to the trials one
// after the other, evaluated exactly as before; a trial that is accepted leaves the rest unused.
// Only systems the hierarchy would solve anyway: a damping-dominated one (lambda >= the block-Jacobi gate,
// adaptive_prec) is cheaper on its own.
// ... and only while this iteration's solves behave: a batch runs until its LAST system is done, every iteration
// at the price of all of them, and one failing system sends the whole batch to the sequential path's fall-backs --
// in the as-written arithmetic (solves of hundreds of iterations, break-downs, a capped one) that made the
// reference_arithmetic leg 1.7x SLOWER; there the trials stay sequential.
int Engine::lm_trial_solve(int q, double lambda, double ni, const double** x, int32_t* iters, double* rel_res,
                           bool* ok, std::string& err) {
  TrialBatch& B = trial_batch;
  bool from_batch = q > 0 && B.next < B.n && B.lam[B.next] == lambda;
  if (!from_batch) {
    B.n = B.next = 0;
    const bool calm = B.prev_ok && !B.prev_capped && B.prev_pit > 0 && B.prev_pit <= 100;
    const int cap = q >= 1 && calm ? std::min(batch_capacity(), opt.max_trials - q) : 0;
    if (cap >= 2) {
      double gate = DBL_MAX;
      if (adaptive_prec && !trace_stale && mean_diag > 0.0) gate = bj_gate >= 0.0 ? bj_gate : 0.05 * mean_diag;
      int nsys = 0;
      double l = lambda, nu = ni;
      while (nsys < cap && l < gate && std::isfinite(l)) {
        B.lam[nsys++] = l;
        l *= nu;
        nu *= 2.0;
      }
      if (nsys >= 2) {
        bool usable = false;
        int rc = pcg_batch(B.lam, nsys, B.iters, B.rel, B.capped, &usable, err);
        if (rc) return rc;
        if (usable) {
          B.n = nsys;
          from_batch = true;
        }
      }
    }
  }
  if (from_batch) {
    const int s = B.next++;
    *x = b_x + (size_t)s * b_vs;
    *iters = B.iters[s];
    *rel_res = B.rel[s];
    *ok = true;
    last_capped = B.capped[s];
  } else {
    *x = d_x;
    int rc = pcg(lambda, iters, rel_res, ok, err);
    if (rc) return rc;
  }
  B.prev_ok = *ok;
  B.prev_capped = last_capped;
  B.prev_pit = *iters;
  return SIM3OPT_OK;
}

// ---- diagnostic read-outs (see engine_impl.hpp) ----
int SolverSnapshot::take(Engine& e, std::string& err, bool vectors) {
  eng = &e;
  HIPCHK(hipStreamSynchronize(e.stream));
  if (vectors) {
    const size_t nn = (size_t)e.n;
    HIPCHK(vec.alloc(3 * nn + SPAN_GRID_MAX + DL_DOUBLES));
    const size_t vb = sizeof(double) * nn;
    HIPCHK(hipMemcpy(vec, e.d_x, vb, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(vec + nn, e.d_p, vb, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(vec + 2 * nn, e.d_q, vb, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(vec + 3 * nn, e.d_part_a, sizeof(double) * SPAN_GRID_MAX, hipMemcpyDeviceToDevice));
    if (e.d_dl)
      HIPCHK(hipMemcpy(vec + 3 * nn + SPAN_GRID_MAX, e.d_dl, sizeof(double) * DL_DOUBLES, hipMemcpyDeviceToDevice));
    has_dl = e.d_dl != nullptr;
    HIPCHK(hipDeviceSynchronize());  // (device-to-device copies may return before they are done)
  }
  h_one = *e.h_sc;
  HIPCHK(hipMemcpy(&d_one, e.d_sc, sizeof(DevScalars), hipMemcpyDeviceToHost));
  batch = e.batch_ready;
  if (batch) {
    std::memcpy(h_batch, e.h_bsc, sizeof(h_batch));
    HIPCHK(hipMemcpy(d_batch, e.d_bsc, sizeof(d_batch), hipMemcpyDeviceToHost));
  }
  kt = e.kt;
  std::memcpy(sched, e.sched_stats, sizeof(sched));
  work_seen = e.spmv_work_seen;
  true_rel = e.last_true_rel;
  capped = e.last_capped;
  chi_known = e.chi_known;
  chi_cache = e.chi_cache;
  return SIM3OPT_OK;
}

int SolverSnapshot::put_back(int rc, std::string& err) {
  Engine& e = *eng;
  bool ok = hipStreamSynchronize(e.stream) == hipSuccess;
  ok = ok && hipMemcpy(e.d_sc, &d_one, sizeof(DevScalars), hipMemcpyHostToDevice) == hipSuccess;
  *e.h_sc = h_one;
  if (batch) {
    ok = ok && hipMemcpy(e.d_bsc, d_batch, sizeof(d_batch), hipMemcpyHostToDevice) == hipSuccess;
    std::memcpy(e.h_bsc, h_batch, sizeof(h_batch));
  }
  if (vec.get()) {
    const size_t nn = (size_t)e.n, vb = sizeof(double) * nn;
    ok = ok && hipMemcpy(e.d_x, vec, vb, hipMemcpyDeviceToDevice) == hipSuccess;
    ok = ok && hipMemcpy(e.d_p, vec + nn, vb, hipMemcpyDeviceToDevice) == hipSuccess;
    ok = ok && hipMemcpy(e.d_q, vec + 2 * nn, vb, hipMemcpyDeviceToDevice) == hipSuccess;
    ok = ok && hipMemcpy(e.d_part_a, vec + 3 * nn, sizeof(double) * SPAN_GRID_MAX, hipMemcpyDeviceToDevice) == hipSuccess;
    if (has_dl)
      ok = ok && hipMemcpy(e.d_dl, vec + 3 * nn + SPAN_GRID_MAX, sizeof(double) * DL_DOUBLES, hipMemcpyDeviceToDevice) ==
                     hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;  // (device-to-device copies may return before they are done)
  }
  e.kt = kt;
  std::memcpy(e.sched_stats, sched, sizeof(sched));
  e.spmv_work_seen = work_seen;
  e.last_true_rel = true_rel;
  e.last_capped = capped;
  e.chi_known = chi_known;
  e.chi_cache = chi_cache;
  if (rc == SIM3OPT_OK && !ok) {
    err = "restoring the solver's scalars failed";
    rc = SIM3OPT_ERR_HIP;
  }
  return rc;
}

int Engine::diag_begin(PcgView& V, const double* lambda, int nrhs, const DevScalars* from, std::string& err) {
  // no system done among the first nrhs (level-0 launches test it), no failure yet, their damping
  DevScalars s[KB];
  for (int k = 0; k < V.nsc; ++k) {
    s[k] = from[k];
    s[k].rz[0] = s[k].rz[1] = s[k].alpha[0] = s[k].alpha[1] = s[k].rz0 = 0.0;
    s[k].iter = 0;
    s[k].done = k < nrhs ? 0 : 1;
    s[k].stop = s[k].fail = 0;
    s[k].lambda = lambda[std::min(k, nrhs - 1)];
  }
  HIPCHK(hipMemcpy(V.sc, s, sizeof(DevScalars) * V.nsc, hipMemcpyHostToDevice));
  return SIM3OPT_OK;
}

int Engine::precond_apply(int prec, double lambda, int32_t nrhs, const double* r, double* z, std::string& err) {
  if (!linearized) {
    err = "precond_apply: call sim3opt_linearize (or optimize) first";
    return SIM3OPT_ERR_STATE;
  }
  if (comm.world > 1) {
    err = "precond_apply: one GPU only";
    return SIM3OPT_ERR_STATE;
  }
  if ((prec == 2 && !use_amg) || (prec == 1 && !use_chain)) {
    err = "precond_apply: this graph was not initialised with that preconditioner";
    return SIM3OPT_ERR_STATE;
  }
  const int nloc = r1 - r0;
  const int gv = grid_for((nloc + 8) / 9, 4);
  const int nseg = (nloc + chain_seg - 1) / chain_seg;
  SolverSnapshot snap;
  int rc = snap.take(*this, err);
  if (rc) return rc;
  auto body = [&]() -> int {
    int rc2 = diag_begin(pv_one, &lambda, 1, &snap.d_one, err);
    if (rc2) return rc2;
    pv_one.lam[0] = lambda;
    rc2 = pcg_setup(pv_one, prec, 1, err);
    if (rc2) return rc2;
    HIPCHK(hipGetLastError());
    rc2 = fetch_scalars(err);
    if (rc2) return rc2;
    if (h_sc->fail) {
      err = "precond_apply: the set-up met a non-positive pivot";
      return SIM3OPT_ERR_STATE;
    }
    for (int32_t q = 0; q < nrhs; ++q) {
      // r -> d_r and d_z = Minv_0 r, the arithmetic k_pcg_step leaves them with (d_q: staging, a solve rewrites it)
      HIPCHK(hipMemcpyAsync(d_q, r + (size_t)q * n, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL((k_pcg_init<1, false>), dim3(gv), dim3(WG), 0, stream, r0, r1, (const double*)d_q,
                         prec == 1 ? (const double*)nullptr : (const double*)d_Minv, d_x, d_r, d_z, d_p, d_s,
                         BatchStrides{0, 0, 0, 0, 0}, (int64_t)0);
      const double* res = d_z;
      if (prec == 1) {
        hipLaunchKernelGGL(k_chain_apply, dim3(grid_for(nseg, 4)), dim3(WG), 0, stream, r0, r1, chain_seg, d_Minv, d_Gm,
                           d_r, d_z, (const DevScalars*)d_sc);
      } else if (prec == 2) {
        rc2 = amg_apply(err);
        if (rc2) return rc2;
        res = d_az;
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(stream));
      HIPCHK(hipMemcpy(z + (size_t)q * n, res, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return SIM3OPT_OK;
  };
  return snap.put_back(body(), err);
}

int engine_precond_apply(Engine* e, int32_t prec, double lambda, int32_t nrhs, const double* r, double* z,
                         std::string& err) {
  return e->precond_apply(prec, lambda, nrhs, r, z, err);
}

int Engine::spmv_spans(int32_t* n_spans, int32_t* wrow, std::string& err) {
  *n_spans = 4 * span_grid;
  if (!wrow) return SIM3OPT_OK;
  HIPCHK(hipStreamSynchronize(stream));
  HIPCHK(hipMemcpy(wrow, d_wrow, sizeof(int32_t) * (size_t)(4 * span_grid + 1), hipMemcpyDeviceToHost));
  return SIM3OPT_OK;
}

int Engine::operator_apply(int32_t nrhs, const double* lambda, const double* p, const double* rvec, double* q,
                           double* pq, double* rp, std::string& err) {
  if (!linearized) {
    err = "operator_apply: call sim3opt_linearize (or optimize) first";
    return SIM3OPT_ERR_STATE;
  }
  if (comm.world > 1) {
    err = "operator_apply: one GPU only";
    return SIM3OPT_ERR_STATE;
  }
  if (nrhs > 1 && (!use_amg || amg.empty())) {
    err = "operator_apply: several systems need the batch buffers of a multigrid graph";
    return SIM3OPT_ERR_STATE;
  }
  PcgView& V = nrhs > 1 ? pv_batch : pv_one;
  int rc = nrhs > 1 ? batch_alloc(err) : SIM3OPT_OK;
  if (rc) return rc;
  SolverSnapshot snap;  // (after batch_alloc: the batch's scalars are in it)
  rc = snap.take(*this, err);
  if (rc) return rc;
  auto body = [&]() -> int {
    int rc2 = diag_begin(V, lambda, nrhs, V.batch ? snap.d_batch : &snap.d_one, err);
    if (rc2) return rc2;
    // p -> what a solve hands its SpMV (d_z; a batch: b_az), rvec -> r; the dampings travel in the scalars as in a solve
    double* const in = V.batch ? V.az : V.z;
    const size_t bytes = sizeof(double) * (size_t)n;
    for (int k = 0; k < nrhs; ++k) {
      V.lam[k] = lambda[k];
      HIPCHK(hipMemcpyAsync(in + (size_t)k * V.vs, p + (size_t)k * n, bytes, hipMemcpyHostToDevice, stream));
      if (rvec) HIPCHK(hipMemcpyAsync(V.r + (size_t)k * V.vs, rvec + (size_t)k * n, bytes, hipMemcpyHostToDevice, stream));
    }
    rc2 = pcg_spmv(V, nrhs, in, rvec ? V.r : nullptr, false, err);
    if (rc2) return rc2;
    BATCH_DISPATCH(nrhs, hipLaunchKernelGGL((k_final_sum2<KS>), dim3(1), dim3(WG), 0, stream, (const double*)V.part_a,
                       (const double*)V.part_b, spmv_grid(), V.pstride, &V.sc->tmp_pq, SC_DOUBLES));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    DevScalars s[KB];
    HIPCHK(hipMemcpy(s, V.sc, sizeof(DevScalars) * V.nsc, hipMemcpyDeviceToHost));
    for (int k = 0; k < nrhs; ++k) {
      HIPCHK(hipMemcpy(q + (size_t)k * n, V.q + (size_t)k * V.vs, bytes, hipMemcpyDeviceToHost));
      pq[k] = s[k].tmp_pq;
      if (rp) rp[k] = s[k].tmp_rz;
    }
    return SIM3OPT_OK;
  };
  return snap.put_back(body(), err);
}

int engine_spmv_spans(Engine* e, int32_t* n_spans, int32_t* wrow, std::string& err) {
  return e->spmv_spans(n_spans, wrow, err);
}

int engine_operator_apply(Engine* e, int32_t nrhs, const double* lambda, const double* p, const double* rvec, double* q,
                          double* pq, double* rp, std::string& err) {
  return e->operator_apply(nrhs, lambda, p, rvec, q, pq, rp, err);
}

int engine_bench_spmv(Engine* e, int32_t reps, double* ms_mean, std::string& err) {
  if (!e->linearized) {
    err = "bench_spmv: call sim3opt_linearize (or optimize) first";
    return SIM3OPT_ERR_STATE;
  }
  // p = b as a representative dense vector
  HIPCHK(hipMemcpyAsync(e->d_p, e->d_b, sizeof(double) * (size_t)e->n, hipMemcpyDeviceToDevice,
                        e->stream));
  for (int i = 0; i < 3; ++i) e->spmv_raw(0.0, e->d_p, e->d_q, e->d_b, nullptr);
  HIPCHK(hipEventRecord(e->ev_a, e->stream));
  for (int i = 0; i < reps; ++i) e->spmv_raw(0.0, e->d_p, e->d_q, e->d_b, nullptr);
  HIPCHK(hipEventRecord(e->ev_b, e->stream));
  HIPCHK(hipEventSynchronize(e->ev_b));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e->ev_a, e->ev_b));
  *ms_mean = reps > 0 ? ms / reps : 0.0;
  return SIM3OPT_OK;
}

int engine_bench_stream(Engine* e, int32_t mode, int32_t reps, double* ms_mean, std::string& err) {
  const size_t n = (size_t)49 * (size_t)e->nnzb;
  const int g = 2048;
  auto launch = [&]() {
    if (mode == 0) hipLaunchKernelGGL(k_stream_read<0>, dim3(g), dim3(WG), 0, e->stream, e->d_vals, n, e->d_q);
    else if (mode == 1) hipLaunchKernelGGL(k_stream_read<1>, dim3(g), dim3(WG), 0, e->stream, e->d_vals, n, e->d_q);
    else hipLaunchKernelGGL(k_stream_read<2>, dim3(g), dim3(WG), 0, e->stream, e->d_vals, n, e->d_q);
  };
  for (int i = 0; i < 3; ++i) launch();
  HIPCHK(hipEventRecord(e->ev_a, e->stream));
  for (int i = 0; i < reps; ++i) launch();
  HIPCHK(hipEventRecord(e->ev_b, e->stream));
  HIPCHK(hipEventSynchronize(e->ev_b));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e->ev_a, e->ev_b));
  *ms_mean = reps > 0 ? ms / reps : 0.0;
  return SIM3OPT_OK;
}

}  // namespace sim3opt
