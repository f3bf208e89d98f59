// engine_pcg.hip -- preconditioned CG on (H + lambda I) x = b (LinearSolverEigen::solve, kitti_surf.cpp:553-554, on graphs
// too large to factor) and the halo exchange of its row-partitioned form
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
  hipLaunchKernelGGL(k_final_sum2, dim3(1), dim3(WG), 0, stream, part_a, part_b, gn, out2);
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
  HIPCHK(upload(staged, stream, lp.d_send, srows));
  HIPCHK(upload(staged, stream, lp.d_recv, rrows));
  HIPCHK(dev_malloc((void**)&lp.d_sbuf, sizeof(double) * 7 * std::max<size_t>(srows.size(), 1)));
  HIPCHK(dev_malloc((void**)&lp.d_rbuf, sizeof(double) * 7 * std::max<size_t>(rrows.size(), 1)));
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

int Engine::spmv_launch(double lambda, const double* z, const double* rv, std::string& err) {  // the PCG's SpMV: w = A z, w.z (and r.z)
  hipEvent_t a = nullptr, b = nullptr;
  if (opt.time_kernels) {
    int rc = pool_get(a, b, err);
    if (rc) return rc;
  }
  spmv_raw(lambda, z, d_q, rv, d_sc, a, b);
  return SIM3OPT_OK;
}

// Preconditioned CG on (H + lambda I) x = b in the single-reduction form (k_pcg_step); the
// result stays in d_x.  Two launches and one reduction point per iteration; the host only looks at
// one small struct between chunks of iterations (see `chunk` in pcg_attempt).
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
int Engine::pcg_attempt(double lambda, int prec, int32_t* iters, double* rel_res, bool* ok,
                bool* chain_broke, std::string& err, int probe_budget, bool* abandoned) {
  const bool use_chain = prec == 1, use_mg = prec == 2;
  const bool probe = probe_budget > 0;
  double* const zin = use_mg ? d_az : d_z;  // preconditioned residual the PCG consumes
  // r.z: from the SpMV's own pass over r -- or, with the multiplicative multigrid cycle, from the
  // cycle's last kernel, which holds r and writes z (the SpMV then skips its load of r)
  const double* const spmv_r = use_mg && !amg_additive ? nullptr : d_r;
  const int nloc = r1 - r0;
  const int gj = std::max(1, (nloc + WG - 1) / WG);
  const int gv = grid_for((nloc + 8) / 9, 4);  // 36 block rows per workgroup pass
  const int gs = spmv_grid();
  const bool multi = comm.active();
  // [w.z, r.z] summed once by k_final_sum2 (multi-GPU: then all-reduced) instead of by every
  // workgroup of the PCG step when the SpMV leaves more partials than a workgroup sums for free
  const bool pre_sum = multi || gs > MAX_GRID;
  const double* scal = pre_sum ? &d_sc->tmp_pq : nullptr;
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
  const double* Minv_arg = use_chain ? nullptr : d_Minv;
  int rc = SIM3OPT_OK;
  h_sc->rz[0] = h_sc->rz[1] = h_sc->alpha[0] = h_sc->alpha[1] = h_sc->rz0 = 0.0;
  h_sc->iter = 0;
  h_sc->max_iter = max_it;
  h_sc->done = h_sc->stop = h_sc->fail = 0;
  h_sc->tol2 = opt.pcg_rel_tol * opt.pcg_rel_tol;
  h_sc->lambda = lambda;
  // chi2 / scale / maxdiag live in the same struct: only the PCG fields are reset
  HIPCHK(hipMemcpyAsync(&d_sc->rz[0], &h_sc->rz[0], offsetof(DevScalars, chi2), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(&d_sc->iter, &h_sc->iter, offsetof(DevScalars, tmp_pq) - offsetof(DevScalars, iter),
                        hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(&d_sc->lambda, &h_sc->lambda, sizeof(double), hipMemcpyHostToDevice, stream));
  if (use_mg) {
    if (amg_stale) {
      rc = amg_setup(err);
      if (rc) return rc;
    }
    amg_prepare(lambda);
  } else if (use_chain) {
    hipLaunchKernelGGL(k_chain_factor, dim3(std::max(1, (nseg + 63) / 64)), dim3(64), 0, stream,
                       r0, r1, chain_seg, d_rowptr, d_vals, d_sub_first, d_sub_cnt, lambda,
                       d_Minv, d_Gm, d_sc);
  } else {
    hipLaunchKernelGGL(k_jacobi, dim3(gj), dim3(WG), 0, stream, r0, r1, d_rowptr, d_vals, lambda,
                       d_Minv, d_sc, 1.0, (const double*)nullptr, (const double*)nullptr);
  }
  hipLaunchKernelGGL(k_pcg_init, dim3(gv), dim3(WG), 0, stream, r0, r1, d_b, Minv_arg, d_x, d_r,
                     d_z, d_p, d_s);
  if (use_chain || use_mg) {
    if (multi) {
      rc = agree_on_fail(err);
      if (rc) return rc;
    }
    rc = fetch_scalars(err);  // did the factorisation succeed?
    if (rc) return rc;
    if (h_sc->fail) {
      if (opt.verbose)
        std::fprintf(stderr, "sim3opt: %s set-up met a non-positive pivot (lambda %.3g): block-Jacobi for this solve\n",
                     use_mg ? "multigrid" : "chain", lambda);
      if (chain_broke) *chain_broke = true;
      *ok = false;
      *iters = 0;
      *rel_res = 0.0;
      return SIM3OPT_OK;
    }
    if (use_chain)
      hipLaunchKernelGGL(k_chain_apply, dim3(gc), dim3(WG), 0, stream, r0, r1, chain_seg, d_Minv,
                         d_Gm, d_r, d_z, (const DevScalars*)nullptr);
    else {
      rc = amg_apply(err);
      if (rc) return rc;
    }
  }
  HIPCHK(hipGetLastError());
  if (multi && !use_mg) {  // (the multigrid cycle gathers its own operands)
    rc = exchange_rows(d_z, err);
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
  // Launch-bound regime (small graphs: two ~3 us kernels per iteration): replay a captured
  // hipGraph of PCG_GRAPH_ITERS iterations instead of enqueueing them one by one.  The first
  // iteration stays eager (it carries it == 0); captured steps read the counter, the damping and
  // the stopping state from DevScalars, so one instantiated graph serves every solve.
  const bool graphed = !multi && !opt.time_kernels && opt.pcg_graph && max_it > PCG_GRAPH_ITERS && !probe;
  if (graphed && (!pcg_graph || pcg_graph_kind != prec)) {
    if (pcg_graph) { (void)hipGraphExecDestroy(pcg_graph); pcg_graph = nullptr; }
    // a multigrid iteration is ~20 launches: shorter graphs waste fewer no-op launches after
    // convergence
    graph_iters = use_mg ? 4 : PCG_GRAPH_ITERS;
    hipGraph_t gr = nullptr;
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    for (int c = 0; c < graph_iters; ++c) {
      spmv_raw(lambda, zin, d_q, spmv_r, d_sc);
      if (pre_sum)
        hipLaunchKernelGGL(k_final_sum2, dim3(1), dim3(WG), 0, stream, d_part_a, d_part_b, gs,
                           &d_sc->tmp_pq);
      hipLaunchKernelGGL(k_pcg_step, dim3(gv), dim3(WG), 0, stream, r0, r1, (1 + c) & 1, -1,
                         scal, d_part_a, d_part_b, gs, Minv_arg,
                         (const double*)zin, d_z, d_q, d_p, d_s, d_x, d_r, d_sc);
      if (use_chain)
        hipLaunchKernelGGL(k_chain_apply, dim3(gc), dim3(WG), 0, stream, r0, r1, chain_seg,
                           d_Minv, d_Gm, d_r, d_z, (const DevScalars*)d_sc);
      if (use_mg) (void)amg_apply(err);  // single GPU here: no collectives inside
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
  auto apply_prec = [&]() -> int {
    if (use_chain)
      hipLaunchKernelGGL(k_chain_apply, dim3(gc), dim3(WG), 0, stream, r0, r1, chain_seg,
                         d_Minv, d_Gm, d_r, d_z, (const DevScalars*)d_sc);
    if (use_mg) return amg_apply(err);
    return SIM3OPT_OK;
  };
  auto enqueue = [&](int count) -> int {
    if (prec_pending) {
      int rc2 = apply_prec();
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
      int rc2 = spmv_launch(lambda, zin, spmv_r, err);
      if (rc2) return rc2;
      if (pre_sum)  // [w.z, r.z] -> tmp_pq, tmp_rz (adjacent)
        hipLaunchKernelGGL(k_final_sum2, dim3(1), dim3(WG), 0, stream, d_part_a, d_part_b, gs,
                           &d_sc->tmp_pq);
      if (multi) {  // one 2-double all-reduce
        rc2 = comm.allreduce(&d_sc->tmp_pq, 2, 0, stream, err);
        if (rc2) return rc2;
      }
      hipLaunchKernelGGL(k_pcg_step, dim3(gv), dim3(WG), 0, stream, r0, r1, par, it, scal,
                         d_part_a, d_part_b, gs, Minv_arg, (const double*)zin, d_z, d_q, d_p, d_s,
                         d_x, d_r, d_sc);
      if (defer_prec && c + 1 == count) {
        prec_pending = true;
      } else {
        rc2 = apply_prec();
        if (rc2) return rc2;
      }
      if (multi && !use_mg) {  // the next SpMV gathers z from the neighbouring ranks
        rc2 = exchange_rows(d_z, err);
        if (rc2) return rc2;
      }
      par ^= 1;
      ++it;
    }
    sched_stats[0] += count;
    HIPCHK(hipGetLastError());
    return SIM3OPT_OK;
  };
  // a look with nothing queued behind it: h_sc is fresh and every recorded event complete
  auto poll_sync = [&]() -> int {
    int rc2 = fetch_scalars(err);
    if (rc2) return rc2;
    sched_stats[2] += 1;
    if (opt.time_kernels) return pool_drain(err);
    spmv_work_seen = h_sc->n_spmv_work;
    return SIM3OPT_OK;
  };
  // The captured graph starts at par == 1.  An eager chunk of several iterations on that path is cut by one where
  // it would end at par == 0, so that whole graphs can be replayed again should the prediction grow (single
  // iterations next to the end are left alone: two of them restore the parity).
  auto keep_parity = [&](int n) { return graphed && it > 0 && n > 1 && n < graph_iters && ((par ^ (n & 1)) == 0) ? n - 1 : n; };
  PcgRate rate;
  int seen = 0;  // iterations that were enqueued before the look h_sc holds (seen < it: chunks still in the queue)
  const int64_t enq0 = sched_stats[0];
  // The set-up's fetch above has just read the scalars and no step has run since: with a prediction to make up
  // for it the loop's first look is left out (it would only drain the queue the first cycle sits in).
  bool have = predict && (use_chain || use_mg);
  long long work0 = have ? h_sc->n_spmv_work : -1;
  if (have && !opt.time_kernels) spmv_work_seen = h_sc->n_spmv_work;
  for (;;) {
    if (!have) {
      rc = poll_sync();
      if (rc) return rc;
      seen = it;
    }
    have = false;
    if (work0 < 0) work0 = h_sc->n_spmv_work;
    if (opt.verbose >= 3)
      std::fprintf(stderr, "  pcg look: enqueued %d, seen %d, iter %d, r.z %.6e of %.6e (tol2 %.3e), done %d\n", it, seen,
                   h_sc->iter, std::fabs(h_sc->gam_last), h_sc->rz0, h_sc->tol2, h_sc->done);
    if (h_sc->done || h_sc->stop || h_sc->fail || seen >= max_it) break;
    if (probe && it >= 8 && h_sc->rz0 > 0.0) {
      // squared M^-1-norm reduction after `it` iterations -> iterations to the tolerance at that rate
      const double ratio = std::fabs(h_sc->gam_last) / h_sc->rz0;
      const double need = ratio > 0.0 && ratio < 1.0 ? it * std::log(h_sc->tol2) / std::log(ratio) : 1e30;
      if (need > probe_budget) break;
    }
    double rem = -1.0;  // iterations predicted to be needed beyond the `it` enqueued
    if (predict) {
      rate.look(h_sc->iter, h_sc->rz0, h_sc->gam_last);
      const double x = rate.remaining(h_sc->tol2 * h_sc->rz0);
      if (x >= 0.0) rem = std::max(0.0, x - (double)(it - seen));
    }
    int todo = graphed && it == 0 ? 1 : std::min(sched_chunk(rem, chunk, cap), max_it - it);
    if (seen < it && (todo <= 0 || rem == 0.0)) continue;  // all that is predicted is in the queue: wait for it
    if (graphed && it > 0 && par == 1 && todo >= graph_iters) todo -= todo % graph_iters;
    todo = keep_parity(todo);
    rc = enqueue(todo);
    if (rc) return rc;
    // more than this chunk predicted: the look at it goes into a pinned slot and is waited for with the next
    // chunk in the queue
    int ahead = rem >= 0.0 ? std::min(sched_ahead(rem - todo, cap), max_it - it) : 0;
    if (graphed && par == 1 && ahead >= graph_iters) ahead -= ahead % graph_iters;
    ahead = keep_parity(ahead);
    if (ahead >= 2) {
      rc = poll_async(d_sc, 1, err);
      if (rc) return rc;
      seen = it;
      rc = enqueue(ahead);
      if (rc) return rc;
      rc = poll_wait(h_sc, 1, err);
      if (rc) return rc;
      if (!opt.time_kernels) spmv_work_seen = h_sc->n_spmv_work;
      have = true;
    }
  }
  // iterations enqueued that found the solve finished (h_sc: the last look of this solve)
  auto count_idle = [&]() {
    sched_stats[1] += std::max<int64_t>(0, (sched_stats[0] - enq0) - (int64_t)(h_sc->n_spmv_work - work0));
  };
  // stopped on a look that had a chunk queued behind it: the SpMV events are read once the stream has been waited for
  bool drain_late = opt.time_kernels && seen < it;
  if (probe && abandoned && !h_sc->done && !h_sc->fail) {  // (ran out of budget or predicted to)
    *abandoned = true;
    count_idle();
    kt.n_pcg_vec += h_sc->iter;
    *iters = h_sc->iter;
    *rel_res = h_sc->rz0 > 0 ? std::sqrt(std::fabs(h_sc->gam_last) / h_sc->rz0) : 0.0;
    *ok = true;
    return SIM3OPT_OK;
  }
  if (drain_late && !(use_mg && !h_sc->fail)) {
    HIPCHK(hipStreamSynchronize(stream));
    rc = pool_drain(err);
    if (rc) return rc;
    drain_late = false;
  }
  if (multi) {  // every rank updates its replica of all estimates
    rc = comm.allgatherv(d_x, offs, stream, err);  // (the whole step: every replica updates every estimate)
    if (rc) return rc;
    rc = agree_on_fail(err);
    if (rc) return rc;
    rc = fetch_scalars(err);
    if (rc) return rc;
  }
  last_true_rel = 0.0;
  if (use_mg && !h_sc->fail) {
    // The stopping test is in the M^-1 norm.  A multigrid cycle is symmetric by construction but
    // positive definite only within limits (over-correction, inexact coarse solves): should it
    // ever lose definiteness, r.z can vanish while r has not.  So the 2-norm of the (recursive)
    // residual is checked against ||b|| once per solve: two more small launches and one read-back.
    const int gn = grid_for(7 * (int64_t)nloc, WG);
    hipLaunchKernelGGL(k_norms2, dim3(gn), dim3(WG), 0, stream, 7 * r0, 7 * r1, d_r, d_b, d_part_a, d_part_b);
    hipLaunchKernelGGL(k_final_sum2, dim3(1), dim3(WG), 0, stream, d_part_a, d_part_b, gn, &d_sc->tmp_pq);
    HIPCHK(hipGetLastError());
    if (multi) {
      rc = comm.allreduce(&d_sc->tmp_pq, 2, 0, stream, err);
      if (rc) return rc;
    }
    rc = fetch_scalars(err);
    if (rc) return rc;
    if (drain_late) {
      rc = pool_drain(err);
      if (rc) return rc;
    }
    last_true_rel = h_sc->tmp_rz > 0 ? std::sqrt(h_sc->tmp_pq / h_sc->tmp_rz) : 0.0;
    if (opt.verbose)
      std::fprintf(stderr, "sim3opt: multigrid PCG: %d iterations, ||r||_Minv ratio %.2e, ||r||_2 / ||b||_2 %.2e\n",
                   h_sc->iter, h_sc->rz0 > 0 ? std::sqrt(std::fabs(h_sc->gam_last) / h_sc->rz0) : 0.0, last_true_rel);
  }
  count_idle();
  kt.n_pcg_vec += h_sc->iter;
  *iters = h_sc->iter;
  // r.z seen by the last executed step, i.e. of the residual BEFORE that step's update
  *rel_res = h_sc->rz0 > 0 ? std::sqrt(std::fabs(h_sc->gam_last) / h_sc->rz0) : 0.0;
  *ok = !h_sc->fail;
  // stopped by the cap, not by the tolerance: an inexact step (sim3opt_iter_stats::pcg_capped); LM's gain
  // ratio decides what becomes of it -- the exact solver it stands in for has no such state
  last_capped = !h_sc->fail && h_sc->iter >= max_it && *rel_res > opt.pcg_rel_tol;
  return SIM3OPT_OK;
}

// ---- diagnostic read-outs (see engine_impl.hpp) ----
int Engine::diag_begin(double lambda, DevScalars& saved_d, DevScalars& saved_h, std::string& err) {
  HIPCHK(hipStreamSynchronize(stream));
  saved_h = *h_sc;
  HIPCHK(hipMemcpy(&saved_d, d_sc, sizeof(DevScalars), hipMemcpyDeviceToHost));
  // the PCG fields as pcg_attempt sets them: not done (level-0 launches test it), no failure yet, this damping
  DevScalars s = saved_d;
  s.rz[0] = s.rz[1] = s.alpha[0] = s.alpha[1] = s.rz0 = 0.0;
  s.iter = 0;
  s.done = s.stop = s.fail = 0;
  s.lambda = lambda;
  HIPCHK(hipMemcpy(d_sc, &s, sizeof(DevScalars), hipMemcpyHostToDevice));
  return SIM3OPT_OK;
}

int Engine::diag_end(const DevScalars& saved_d, const DevScalars& saved_h, std::string& err) {
  HIPCHK(hipStreamSynchronize(stream));
  HIPCHK(hipMemcpy(d_sc, &saved_d, sizeof(DevScalars), hipMemcpyHostToDevice));
  *h_sc = saved_h;
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
  DevScalars sd, sh;
  int rc = diag_begin(lambda, sd, sh, err);
  if (rc) return rc;
  auto body = [&]() -> int {
    if (prec == 2) {
      if (amg_stale) {
        int rc2 = amg_setup(err);
        if (rc2) return rc2;
      }
      amg_prepare(lambda);
    } else if (prec == 1) {
      hipLaunchKernelGGL(k_chain_factor, dim3(std::max(1, (nseg + 63) / 64)), dim3(64), 0, stream, r0, r1, chain_seg,
                         d_rowptr, d_vals, d_sub_first, d_sub_cnt, lambda, d_Minv, d_Gm, d_sc);
    } else {
      hipLaunchKernelGGL(k_jacobi, dim3(std::max(1, (nloc + WG - 1) / WG)), dim3(WG), 0, stream, r0, r1, d_rowptr,
                         d_vals, lambda, d_Minv, d_sc, 1.0, (const double*)nullptr, (const double*)nullptr);
    }
    HIPCHK(hipGetLastError());
    int rc2 = fetch_scalars(err);
    if (rc2) return rc2;
    if (h_sc->fail) {
      err = "precond_apply: the set-up met a non-positive pivot";
      return SIM3OPT_ERR_STATE;
    }
    for (int32_t q = 0; q < nrhs; ++q) {
      // r -> d_r and d_z = Minv_0 r, the arithmetic k_pcg_step leaves them with (d_q: staging, a solve rewrites it)
      HIPCHK(hipMemcpyAsync(d_q, r + (size_t)q * n, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL(k_pcg_init, dim3(gv), dim3(WG), 0, stream, r0, r1, (const double*)d_q,
                         prec == 1 ? (const double*)nullptr : (const double*)d_Minv, d_x, d_r, d_z, d_p, d_s);
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
  rc = body();
  std::string err2;
  const int rc_end = diag_end(sd, sh, err2);
  if (rc == SIM3OPT_OK && rc_end) {
    err = err2;
    rc = rc_end;
  }
  return rc;
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
  DevScalars sd, sh;
  int rc = diag_begin(lambda[0], sd, sh, err);
  if (rc) return rc;
  auto body = [&]() -> int {
    if (nrhs > 1) return operator_apply_batch(nrhs, lambda, p, rvec, q, pq, rp, err);
    // p -> d_z (what the PCG hands its SpMV), rvec -> d_r; the damping travels in d_sc as in pcg_attempt
    const size_t bytes = sizeof(double) * (size_t)n;
    HIPCHK(hipMemcpyAsync(d_z, p, bytes, hipMemcpyHostToDevice, stream));
    if (rvec) HIPCHK(hipMemcpyAsync(d_r, rvec, bytes, hipMemcpyHostToDevice, stream));
    const int gs = spmv_grid();
    spmv_raw(lambda[0], d_z, d_q, rvec ? d_r : nullptr, d_sc);
    // (k_pcg_step adds the partials by sum_partials in every workgroup, or reads the pair k_final_sum2 left when there
    // are more than MAX_GRID of them: the same FUNCTION on the same arrays, count and block size, hence the same value
    // -- one launch serves both; the in-step summation itself is exercised by the iterates of sim3opt_solve only)
    hipLaunchKernelGGL(k_final_sum2, dim3(1), dim3(WG), 0, stream, d_part_a, d_part_b, gs, &d_sc->tmp_pq);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipMemcpy(q, d_q, bytes, hipMemcpyDeviceToHost));
    double two[2];
    HIPCHK(hipMemcpy(two, &d_sc->tmp_pq, sizeof(two), hipMemcpyDeviceToHost));
    pq[0] = two[0];
    if (rp) rp[0] = two[1];
    return SIM3OPT_OK;
  };
  rc = body();
  std::string err2;
  const int rc_end = diag_end(sd, sh, err2);
  if (rc == SIM3OPT_OK && rc_end) {
    err = err2;
    rc = rc_end;
  }
  return rc;
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
