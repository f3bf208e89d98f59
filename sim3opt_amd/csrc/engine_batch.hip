// engine_batch.hip -- the multigrid-preconditioned CG for several right-hand sides at once: the rejected
// trials of one LM iteration (OptimizationAlgorithmLevenberg::solve, reached from kitti_surf.cpp:675) solve
// (H + lambda_k I) x_k = b for a known sequence lambda_k; after the first rejection the next ones are solved
// together -- one pass over the blocks for K vectors, K vectors per coarse launch -- and evaluated in g2o's
// order (Engine::lm_trial_solve, at the end, decides and hands them out).  Here: the buffers, the PCG loop for K
// systems (batch_kernels.hpp) and its K-system SpMV; the preconditioner is the ONE multigrid cycle of
// engine_amg.hip, handed the batch's view (cv_batch).  Per system the arithmetic is that of Engine::pcg_attempt
// with the multigrid preconditioner, operation by operation: the K solutions are bit for bit those of K
// sequential solves.
#include "engine_impl.hpp"

namespace sim3opt {

#include "spmv_kernel.hpp"
#include "batch_kernels.hpp"

static inline int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

// buffers of the batched solve, allocated at its first use (single GPU, multigrid path)
int Engine::batch_alloc(std::string& err) {
  if (batch_ready) return SIM3OPT_OK;
  const int nl = (int)amg.size();
  auto alloc = [&](double*& p, size_t count) -> int {
    HIPCHK(dev_malloc((void**)&p, sizeof(double) * std::max<size_t>(count, 1)));
    batch_owned.push_back(p);
    HIPCHK(hipMemsetAsync(p, 0, sizeof(double) * std::max<size_t>(count, 1), stream));
    return SIM3OPT_OK;
  };
  // (schedule only -- the results do not depend on it: which levels run one system per grid slice)
  if (const char* ev = std::getenv("SIM3OPT_BATCH_SLICE_BLOCKS")) b_slice_blocks = std::atoll(ev);
  b_vs = pad64(n);
  double** v0[] = {&b_x, &b_r, &b_z, &b_p, &b_q, &b_s, &b_az};
  for (double** v : v0) {
    int rc = alloc(*v, (size_t)KB * b_vs);
    if (rc) return rc;
  }
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
    int rc = alloc(B.Minv, (size_t)KB * B.ms);
    if (rc) return rc;
    if (l == 0) {
      B.r = b_r; B.x = b_z; B.t = b_az;
    } else {
      if ((rc = alloc(B.r, (size_t)KB * B.vs))) return rc;
      if ((rc = alloc(B.x, (size_t)KB * B.vs))) return rc;
      if ((rc = alloc(B.t, (size_t)KB * B.vs))) return rc;
      HIPCHK(dev_malloc((void**)&B.diag32, sizeof(float) * (size_t)KB * B.ms));
      batch_owned.push_back(B.diag32);
      HIPCHK(hipMemsetAsync(B.diag32, 0, sizeof(float) * (size_t)KB * B.ms, stream));
    }
  }
  const size_t nc = (size_t)7 * amg[nl - 1].nb;
  b_as = (int64_t)(nc * nc);
  int rc = alloc(b_Ainv, (size_t)KB * b_as);
  if (rc) return rc;
  if ((rc = alloc(b_diag64, (size_t)KB * 49 * amg[nl - 1].nb))) return rc;
  if ((rc = alloc(b_part_a, (size_t)KB * SPAN_GRID_MAX))) return rc;
  if ((rc = alloc(b_part_b, (size_t)KB * SPAN_GRID_MAX))) return rc;
  HIPCHK(dev_malloc((void**)&d_bsc, sizeof(DevScalars) * KB));
  batch_owned.push_back(d_bsc);
  HIPCHK(hipMemsetAsync(d_bsc, 0, sizeof(DevScalars) * KB, stream));
  HIPCHK(host_malloc((void**)&h_bsc, sizeof(DevScalars) * KB));
  V.sc = d_bsc;
  V.Ainv = b_Ainv;
  V.as = b_as;
  V.rz_part = b_part_b;
  V.part = SPAN_GRID_MAX;
  batch_ready = true;
  return SIM3OPT_OK;
}

void Engine::batch_release() {
  for (void* p : batch_owned)
    if (p) dev_free(p);
  batch_owned.clear();
  if (h_bsc) host_free(h_bsc);
  h_bsc = nullptr;
  d_bsc = nullptr;
  cv_batch = CycleView();
  batch_ready = false;
}

// Solves (H + lams[s] I) x_s = b, s < nsys <= KB, together; x_s is left in b_x + s * b_vs.  *usable = false:
// some system broke down or failed the true-residual check -- the caller then solves the trials one by one
// (the sequential path has the fall-backs: plain cycle instead of the over-corrected one, block-Jacobi).
// cols (columns of the inverse, engine_columns.hip): system s solves for ITS right-hand side cols->g + s * stride to
// its own tolerance, all at lams[0] -- so ONE set-up (smoother inverses, FP32 diagonals, dense coarsest inverse: slot
// 0, the caller has set the per-system strides of cv_batch to 0) serves them all, and the batches of a call that
// follow the first (cols->setup false) run none.  The 2-norm check is the caller's, on the true residual.
int Engine::pcg_batch(const double* lams, int nsys, int32_t* iters, double* rel_res, bool* capped, bool* usable,
                      std::string& err, const BatchRhs* cols) {
  *usable = false;
  int rc = batch_alloc(err);
  if (rc) return rc;
  if (amg_stale) {
    rc = amg_setup(err);
    if (rc) return rc;
  }
  const int nl = (int)amg.size();
  const int max_it = opt.pcg_max_iters > 0 ? opt.pcg_max_iters : (n <= 50000 ? std::max(100, 2 * n) : 1000);
  for (int s = 0; s < KB; ++s) {
    DevScalars& h = h_bsc[s];
    std::memset(&h, 0, sizeof(DevScalars));
    h.max_iter = max_it;
    h.tol2 = cols ? cols->tol[std::min(s, nsys - 1)] * cols->tol[std::min(s, nsys - 1)] : opt.pcg_rel_tol * opt.pcg_rel_tol;
    h.lambda = s < nsys ? lams[s] : lams[nsys - 1];
    h.done = s < nsys ? 0 : 1;  // (an unused slot: finished from the start, its vectors stay zero)
  }
  HIPCHK(hipMemcpyAsync(d_bsc, h_bsc, sizeof(DevScalars) * KB, hipMemcpyHostToDevice, stream));
  // per system: damped diagonal blocks, smoother inverses, dense inverse of the coarsest level (amg_prepare)
  const int nsetup = cols ? (cols->setup ? 1 : 0) : nsys;
  for (int s = 0; s < nsetup; ++s) {
    for (int l = 0; l < nl; ++l) {
      const AmgLevel& L = amg[l];
      const CycleLevel& B = cv_batch.lv[l];
      jacobi(0, L.nb, L.rowptr, L.vals, lams[s], B.Minv + (size_t)s * B.ms, amg_omega, L.diagH, L.W, nullptr,
             d_bsc + s, l == nl - 1 ? b_diag64 + (size_t)s * 49 * L.nb : nullptr,
             l > 0 ? B.diag32 + (size_t)s * B.ms : nullptr);
    }
    dense_inverse(b_diag64 + (size_t)s * 49 * amg[nl - 1].nb, b_Ainv + (size_t)s * b_as, d_bsc + s);
  }
  const int gv = grid_for((nb + 8) / 9, 4);
  const int gs = span_grid;
  const CycleLevel& B0 = cv_batch.lv[0];
  BatchStrides bs0{b_vs, B0.ms, 0, 0, SPAN_GRID_MAX};
  cv_batch.nsys = nsys;
  if (cols)
    BATCH_DISPATCH(nsys, hipLaunchKernelGGL((k_pcg_init_k<KS, true>), dim3(gv), dim3(WG), 0, stream, 0, nb, cols->g,
                       (const double*)B0.Minv, b_x, b_r, b_z, b_p, b_s, bs0, cols->stride));
  else
    BATCH_DISPATCH(nsys, hipLaunchKernelGGL((k_pcg_init_k<KS>), dim3(gv), dim3(WG), 0, stream, 0, nb, (const double*)d_b,
                       (const double*)B0.Minv, b_x, b_r, b_z, b_p, b_s, bs0, (int64_t)0));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_bsc, d_bsc, sizeof(DevScalars) * KB, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (int s = 0; s < nsys; ++s)
    if (h_bsc[s].fail) return SIM3OPT_OK;  // a non-positive pivot of some set-up: not usable
  amg_cycle(cv_batch, 0, b_z, b_az);
  // chunks and looks as in pcg_attempt: the prediction is per system, a chunk ends where the first of the live
  // systems is predicted to finish -- so that `live` shrinks then and not up to three K-system iterations later
  const int pce = std::max(1, opt.pcg_check_every);
  const int chunk = std::min(4, pce);
  const bool predict = pce > 1;
  const int cap = pce >= 4 ? std::min(pce, std::max(4, sched_cap_mg)) : pce;
  int it = 0, par = 0, seen = 0, live = 0;
  // (the cycle after a chunk's last step goes to the head of the next chunk, as in pcg_attempt: the step that
  // finishes the last live system is not followed by a K-system cycle nobody reads)
  bool cycle_pending = false;
  auto enqueue = [&](int count) -> int {
    if (cycle_pending) amg_cycle(cv_batch, 0, b_z, b_az);
    cycle_pending = false;
    for (int c = 0; c < count; ++c) {
      BATCH_DISPATCH(live, hipLaunchKernelGGL((k_spmv_span<8, true, 0, double, KS, false>), dim3(gs), dim3(WG), 0, stream,
                         nb, d_wrow, d_rowptr, d_colidx, (const double*)d_vals, (const double*)b_az, b_q, 0.0, b_part_a,
                         (const double*)nullptr, b_part_b, d_bsc, (const double*)nullptr, 1, (const int32_t*)nullptr, 1.0,
                         bs0, (const float*)nullptr));
      BATCH_DISPATCH(live, hipLaunchKernelGGL((k_final_sum2_k<KS>), dim3(1), dim3(WG), 0, stream, (const double*)b_part_a,
                         (const double*)b_part_b, gs, SPAN_GRID_MAX, d_bsc));
      BATCH_DISPATCH(live, hipLaunchKernelGGL((k_pcg_step_k<KS>), dim3(gv), dim3(WG), 0, stream, 0, nb, par, it,
                         (const double*)B0.Minv, (const double*)b_az, b_z, (const double*)b_q, b_p, b_s, b_x, b_r, d_bsc,
                         bs0));
      if (c + 1 == count) cycle_pending = true;
      else amg_cycle(cv_batch, 0, b_z, b_az);
      par ^= 1;
      ++it;
    }
    sched_stats[0] += count;
    HIPCHK(hipGetLastError());
    return SIM3OPT_OK;
  };
  PcgRate rate[KB];
  const int64_t enq0 = sched_stats[0];
  // (the set-up's look above is the loop's first: no step has run since)
  bool have = predict;
  for (;;) {
    if (!have) {
      HIPCHK(hipMemcpyAsync(h_bsc, d_bsc, sizeof(DevScalars) * KB, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      sched_stats[2] += 1;
      seen = it;
    }
    have = false;
    // systems still iterating: [0, live).  The dampings ascend with the trial, so the systems finish from the
    // tail as a rule; the launches that follow carry the first `live` systems only (per system the same
    // operations whatever K is: the results do not depend on when the others finished)
    live = 0;
    for (int s = 0; s < nsys; ++s)
      if (!(h_bsc[s].done || h_bsc[s].stop || h_bsc[s].fail)) live = s + 1;
    if (opt.verbose >= 3)
      for (int s = 0; s < nsys; ++s)
        std::fprintf(stderr, "  batch look: system %d, enqueued %d, seen %d, iter %d, r.z %.6e of %.6e (tol2 %.3e), done %d\n", s,
                     it, seen, h_bsc[s].iter, std::fabs(h_bsc[s].gam_last), h_bsc[s].rz0, h_bsc[s].tol2, h_bsc[s].done);
    if (live == 0 || seen >= max_it) break;
    double rem = -1.0;  // iterations beyond the `it` enqueued until the first of the live systems finishes
    if (predict) {
      double xmin = DBL_MAX;
      for (int s = 0; s < live; ++s) {
        const DevScalars& h = h_bsc[s];
        if (h.done || h.stop || h.fail) continue;
        rate[s].look(h.iter, h.rz0, h.gam_last);
        const double x = rate[s].remaining(h.tol2 * h.rz0);
        xmin = x < 0.0 ? -1.0 : std::min(xmin, x);
        if (x < 0.0) break;
      }
      if (xmin >= 0.0) rem = std::max(0.0, xmin - (double)(it - seen));
    }
    const int todo = std::min(sched_chunk(rem, chunk, cap), max_it - it);
    if (seen < it && (todo <= 0 || rem == 0.0)) continue;  // all that is predicted is in the queue: wait for it
    cv_batch.nsys = live;
    rc = enqueue(todo);
    if (rc) return rc;
    const int ahead = rem >= 0.0 ? std::min(sched_ahead(rem - todo, cap), max_it - it) : 0;
    if (ahead >= 2) {  // no system is predicted to finish in the next chunk either: look without draining the queue
      rc = poll_async(d_bsc, KB, err);
      if (rc) return rc;
      seen = it;
      rc = enqueue(ahead);
      if (rc) return rc;
      rc = poll_wait(h_bsc, KB, err);
      if (rc) return rc;
      have = true;
    }
  }
  // what the stopping test claims, checked in the 2-norm per system (see pcg_attempt)
  bool good = true;
  for (int s = 0; s < nsys; ++s) {
    if (h_bsc[s].fail) { good = false; continue; }
    if (!cols) norms2(b_r + (size_t)s * b_vs, d_b, b_part_a, b_part_b, &d_bsc[s].tmp_pq);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_bsc, d_bsc, sizeof(DevScalars) * KB, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  // (the batch's counter starts at zero: K-system iterations that found every system finished)
  sched_stats[1] += std::max<int64_t>(0, (sched_stats[0] - enq0) - (int64_t)h_bsc[0].n_spmv_work);
  int it_max = 0;
  for (int s = 0; s < nsys; ++s) {
    const DevScalars& h = h_bsc[s];
    const double true_rel = !cols && h.tmp_rz > 0 ? std::sqrt(h.tmp_pq / h.tmp_rz) : 0.0;
    if (h.fail || true_rel > 1e-3) good = false;
    iters[s] = h.iter;
    rel_res[s] = h.rz0 > 0 ? std::sqrt(std::fabs(h.gam_last) / h.rz0) : 0.0;
    capped[s] = !h.fail && h.iter >= max_it && rel_res[s] > (cols ? cols->tol[s] : opt.pcg_rel_tol);
    it_max = std::max(it_max, (int)h.iter);
    if (opt.verbose)
      std::fprintf(stderr, "sim3opt: batched multigrid PCG, system %d of %d: lambda %.6g, %d iterations, ||r||_Minv ratio %.2e, "
                   "||r||_2 / ||b||_2 %.2e\n", s, nsys, lams[s], h.iter, rel_res[s], true_rel);
  }
  kt.n_pcg_vec += it_max;
  kt.n_batched_solves += nsys;
  kt.n_batches += 1;
  *usable = good;
  return SIM3OPT_OK;
}

// Diagnostic read-out (Engine::operator_apply brackets it): q_s = (H + lambda_s I) p_s, p_s . q_s and rvec_s . p_s by
// the SpMV launch of pcg_batch and its sum.  pcg_batch itself always passes rvec = nullptr (its r.z comes from the
// cycle): without rvec this is its launch, with rvec the kernel's r.p branch is taken for the read-out alone
// (diagnostic only; q and p.q do not depend on it, tested).  The batch's scalars are put back on both sides; b_az, b_r
// and b_q are rewritten by every pcg_batch before it reads them.
int Engine::operator_apply_batch(int32_t nrhs, const double* lambda, const double* p, const double* rvec, double* q,
                                 double* pq, double* rp, std::string& err) {
  int rc = batch_alloc(err);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(stream));
  DevScalars saved_d[KB], saved_h[KB], s[KB];
  HIPCHK(hipMemcpy(saved_d, d_bsc, sizeof(saved_d), hipMemcpyDeviceToHost));
  std::memcpy(saved_h, h_bsc, sizeof(saved_h));
  auto body = [&]() -> int {
    std::memset(s, 0, sizeof(s));
    for (int k = 0; k < KB; ++k) {
      s[k].lambda = lambda[std::min<int>(k, nrhs - 1)];
      s[k].done = k < nrhs ? 0 : 1;
    }
    HIPCHK(hipMemcpy(d_bsc, s, sizeof(s), hipMemcpyHostToDevice));
    const size_t bytes = sizeof(double) * (size_t)n;
    for (int k = 0; k < nrhs; ++k) {
      HIPCHK(hipMemcpyAsync(b_az + (size_t)k * b_vs, p + (size_t)k * n, bytes, hipMemcpyHostToDevice, stream));
      if (rvec) HIPCHK(hipMemcpyAsync(b_r + (size_t)k * b_vs, rvec + (size_t)k * n, bytes, hipMemcpyHostToDevice, stream));
    }
    const int gs = span_grid;
    BatchStrides bs0{b_vs, cv_batch.lv[0].ms, 0, 0, SPAN_GRID_MAX};
    BATCH_DISPATCH(nrhs, hipLaunchKernelGGL((k_spmv_span<8, true, 0, double, KS, false>), dim3(gs), dim3(WG), 0, stream,
                       nb, d_wrow, d_rowptr, d_colidx, (const double*)d_vals, (const double*)b_az, b_q, 0.0, b_part_a,
                       rvec ? (const double*)b_r : (const double*)nullptr, b_part_b, d_bsc, (const double*)nullptr, 1,
                       (const int32_t*)nullptr, 1.0, bs0, (const float*)nullptr));
    BATCH_DISPATCH(nrhs, hipLaunchKernelGGL((k_final_sum2_k<KS>), dim3(1), dim3(WG), 0, stream, (const double*)b_part_a,
                       (const double*)b_part_b, gs, SPAN_GRID_MAX, d_bsc));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipMemcpy(s, d_bsc, sizeof(s), hipMemcpyDeviceToHost));
    for (int k = 0; k < nrhs; ++k) {
      HIPCHK(hipMemcpy(q + (size_t)k * n, b_q + (size_t)k * b_vs, bytes, hipMemcpyDeviceToHost));
      pq[k] = s[k].tmp_pq;
      if (rp) rp[k] = s[k].tmp_rz;
    }
    return SIM3OPT_OK;
  };
  rc = body();
  if (hipStreamSynchronize(stream) != hipSuccess || hipMemcpy(d_bsc, saved_d, sizeof(saved_d), hipMemcpyHostToDevice) != hipSuccess) {
    if (rc == SIM3OPT_OK) {
      err = "operator_apply: restoring the batch's scalars failed";
      rc = SIM3OPT_ERR_HIP;
    }
  }
  std::memcpy(h_bsc, saved_h, sizeof(saved_h));
  return rc;
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

}  // namespace sim3opt
