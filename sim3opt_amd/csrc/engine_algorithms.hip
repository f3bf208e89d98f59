// engine_algorithms.hip -- the nonlinear algorithms besides Levenberg-Marquardt (g2o: OptimizationAlgorithmGaussNewton
// and OptimizationAlgorithmDogleg behind SparseOptimizer::setAlgorithm), on the engine's linearisation, solvers and
// chi2.  Engine::optimize hands options.algorithm = 1 / 2 here.  The rules are written out in DESIGN.md 5h.
#include "engine_impl.hpp"

namespace sim3opt {

#include "algo_kernels.hpp"

int Engine::fail_iteration(int it, sim3opt_iter_stats& T, double chi, std::vector<sim3opt_iter_stats>& stats,
                           const char* why, std::string& err) {
  iter_end(T, chi, stats);
  err = why;
  if (opt.verbose) std::fprintf(stderr, "iteration= %d\t %s\n", it, err.c_str());
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

// ------------------------------------------------------------------------------------------
// Gauss-Newton: linearise, solve H x = b (lambda = 0), S <- exp(x) S, chi2.  No acceptance test; a failed solve
// (CG breakdown, a non-positive pivot of the exact factorisation) is g2o's Fail: optimize() returns 0.
// ------------------------------------------------------------------------------------------
int Engine::optimize_gauss_newton(int32_t max_iters, std::vector<sim3opt_iter_stats>& stats, std::string& err) {
  int iters = 0;
  for (int it = 0; it < max_iters; ++it) {
    sim3opt_iter_stats T{};
    double currentChi = 0.0;
    int rc = iter_begin(T, currentChi, err);
    if (rc) return rc;
    if (phase_timing) HIPCHK(hipEventRecord(ev_ph[1], stream));
    int32_t pit = 0;
    double rres = 0.0;
    bool ok = true;
    rc = pcg(0.0, &pit, &rres, &ok, err);
    if (rc) return rc;
    if (phase_timing) HIPCHK(hipEventRecord(ev_ph[2], stream));
    T.pcg_iters = pit;
    T.pcg_rel_res = rres;
    if (last_capped) T.pcg_capped = 1;
    T.trials = 1;
    double newChi = DBL_MAX;
    if (ok) {  // (exact path: the verdict comes back with chi2; k_oplus leaves the estimates alone on a failure)
      apply_step(d_x, false);
      HIPCHK(hipGetLastError());
      rc = chi2(&newChi, err, phase_timing ? ev_ph[3] : nullptr);
      if (rc) return rc;
      kt.n_update += 1;
      if (direct_rejected()) ok = false;
      else if ((rc = phase_ms(2, 3, T.ms_update, err))) return rc;
    } else if (phase_timing) {
      HIPCHK(hipStreamSynchronize(stream));  // (ev_ph[2] was recorded after the solve's last fetch)
    }
    if ((rc = phase_ms(0, 1, T.ms_linearize, err)) || (rc = phase_ms(1, 2, T.ms_solve, err))) return rc;
    if (!ok)
      return fail_iteration(it, T, currentChi, stats,
                            "optimize: Gauss-Newton: the linear solve failed (H not positive definite)", err);
    iter_end(T, newChi, stats);
    ++iters;
    if (opt.verbose)
      std::fprintf(stderr, "iteration= %d\t chi2= %.9g\t pcg= %d (rel %.2e)\t ms lin/solve/upd= %.3f/%.3f/%.3f\n", it,
                   newChi, pit, rres, T.ms_linearize, T.ms_solve, T.ms_update);
  }
  HIPCHK(hipStreamSynchronize(stream));
  return iters;
}

// ------------------------------------------------------------------------------------------
// Powell's dogleg
// ------------------------------------------------------------------------------------------
// d_dl[DL_OUT + DL_*] <- b.b, b^T H b, g.g, b.g, (Hb).g, g^T H g for b = d_b, g = h_gn = d_x.  Both vectors are whole on
// every rank here (b all-gathered after the linearisation, h_gn by the PCG), so the SpMVs of this rank's rows need
// no further exchange; the scalars of the ranks' rows are summed by one all-reduce.
int Engine::dogleg_dots(std::string& err) {
  const int gs = spmv_grid();
  double* out = d_dl + 4 * MAX_GRID + DL_OUT;
  // q = H b (lambda = 0): its v.q partials are b^T H b
  spmv_raw(0.0, d_b, d_q, nullptr, nullptr);
  hipLaunchKernelGGL(k_dl_sum, dim3(1), dim3(WG), 0, stream, (const double*)d_part_a, gs, out + DL_BHB);
  // H h_gn into the PCG's (now unused) direction vector: its v.q partials are h_gn^T H h_gn
  spmv_raw(0.0, d_x, d_p, nullptr, nullptr);
  const int gd = grid_for(7 * (int64_t)(r1 - r0), WG);
  hipLaunchKernelGGL(k_dl_dots, dim3(gd), dim3(WG), 0, stream, 7 * r0, 7 * r1, (const double*)d_b,
                     (const double*)d_x, (const double*)d_q, d_dl);
  hipLaunchKernelGGL(k_dl_final, dim3(1), dim3(WG), 0, stream, (const double*)d_dl, gd, (const double*)d_part_a, gs,
                     out);
  HIPCHK(hipGetLastError());
  if (comm.active()) return comm.allreduce(out, 6, 0, stream, err);
  return SIM3OPT_OK;
}

int Engine::optimize_dogleg(int32_t max_iters, std::vector<sim3opt_iter_stats>& stats, std::string& err) {
  if (!d_dl) {
    HIPCHK(mem.alloc(d_dl, 4 * MAX_GRID + DL_OUT + 8, nullptr));
  }
  if (!h_dl) HIPCHK(host_malloc((void**)&h_dl, sizeof(double) * 8));
  // (the span SpMV's launch state -- row spans d_wrow, partial buffers -- is built by init() for every linear
  // solver; with the exact factorisation it is otherwise unused)
  if (!d_wrow || spmv_grid() <= 0 || !d_part_a) {
    err = "dogleg: the SpMV's launch state is missing";
    return SIM3OPT_ERR_STATE;
  }
  const double* d_out = d_dl + 4 * MAX_GRID + DL_OUT;
  // g2o's state at iteration 0 of a (non-online) optimize()
  double delta = opt.dl_delta_init, lam_c = opt.dl_lambda_init;
  bool was_pd = true;
  const double factor = opt.dl_lambda_factor;
  int iters = 0;
  bool ok_all = true;
  for (int it = 0; it < max_iters && ok_all; ++it) {
    sim3opt_iter_stats T{};
    sim3opt_tr_stats R{};
    R.delta_before = delta;
    double currentChi = 0.0;
    int rc = iter_begin(T, currentChi, err);
    if (rc) return rc;
    if (comm.active()) {  // every replica forms the whole step from b
      rc = comm.allgatherv(d_b, offs, stream, err);
      if (rc) return rc;
    }
    if (phase_timing) HIPCHK(hipEventRecord(ev_ph[1], stream));
    // h_gn, once per iteration; damped (lambda_c) from the first failure on, lambda_c adapted as g2o does
    bool solved = false;
    while (!solved) {
      const double lam = was_pd ? 0.0 : lam_c;
      int32_t pit = 0;
      double rres = 0.0;
      bool ok = true;
      rc = pcg(lam, &pit, &rres, &ok, err);
      if (rc) return rc;
      T.pcg_iters += pit;
      T.pcg_rel_res = rres;
      if (last_capped) T.pcg_capped += 1;
      rc = dogleg_dots(err);
      if (rc) return rc;
      if (phase_timing) HIPCHK(hipEventRecord(ev_ph[2], stream));
      // one round trip: the six scalars and (exact path) the factorisation's verdict
      HIPCHK(hipMemcpyAsync(h_dl, d_out, sizeof(double) * 6, hipMemcpyDeviceToHost, stream));
      rc = fetch_scalars(err);
      if (rc) return rc;
      if (direct_rejected()) ok = false;
      was_pd = was_pd && ok;
      if (!was_pd) {
        if (ok) {
          T.lambda = lam;
          lam_c = std::max(1e-12, lam_c / (0.5 * factor));
        } else {
          lam_c *= factor;
          if (lam_c > 1e3) {  // g2o: Fail
            lam_c = 1e3;
            break;
          }
        }
      }
      solved = ok;
      if (opt.verbose >= 2)
        std::fprintf(stderr, "  GN solve: lambda %.6g, %s, %d PCG iterations (rel %.2e)\n", lam,
                     ok ? "ok" : "failed", pit, rres);
    }
    if ((rc = phase_ms(0, 1, T.ms_linearize, err)) || (rc = phase_ms(1, 2, T.ms_solve, err))) return rc;
    R.was_pd = was_pd ? 1 : 0;
    if (!solved) {
      T.lambda = lam_c;
      R.delta_after = delta;
      tr_stats.push_back(R);
      return fail_iteration(it, T, currentChi, stats,
                            "optimize: dogleg: the damped linear solve still failed at lambda 1e3", err);
    }
    const double bb = h_dl[DL_BB], bHb = h_dl[DL_BHB], gg = h_dl[DL_GG], bg = h_dl[DL_BG], hbg = h_dl[DL_HBG],
                 gHg = h_dl[DL_GHG];
    const double alpha = bb / bHb;  // h_sd = alpha b
    const double hsd_norm = std::fabs(alpha) * std::sqrt(bb), hgn_norm = std::sqrt(gg);
    R.alpha = alpha;
    R.norm_sd = hsd_norm;
    R.norm_gn = hgn_norm;
    int tries = 0;
    bool good = false;
    double rho = 0.0;
    do {
      ++tries;
      if (phase_timing) HIPCHK(hipEventRecord(ev_ph[1], stream));
      double ca = 0.0, cg = 0.0;  // h_dl = ca b + cg h_gn
      if (hgn_norm < delta) {
        cg = 1.0;
        R.step = SIM3OPT_STEP_GN;
      } else if (hsd_norm > delta) {
        ca = delta / hsd_norm * alpha;
        R.step = SIM3OPT_STEP_SD;
      } else {
        // h_sd + beta (h_gn - h_sd), ||.|| = delta; g2o's two numerically stable forms of the root
        const double hsd2 = alpha * alpha * bb;
        const double c = alpha * bg - hsd2;                  // h_sd . (h_gn - h_sd)
        const double bma2 = gg - 2.0 * alpha * bg + hsd2;    // ||h_gn - h_sd||^2
        const double d2 = delta * delta - hsd2;
        double beta;
        if (c <= 0.0) beta = (-c + std::sqrt(c * c + bma2 * d2)) / bma2;
        else beta = d2 / (c + std::sqrt(c * c + bma2 * d2));
        ca = (1.0 - beta) * alpha;
        cg = beta;
        R.step = SIM3OPT_STEP_DL;
      }
      // ||h_dl||^2, b.h_dl and h_dl^T H h_dl as quadratic forms in (ca, cg)
      const double dl2 = ca * ca * bb + 2.0 * ca * cg * bg + cg * cg * gg;
      const double bh = ca * bb + cg * bg;
      const double hHh = ca * ca * bHb + 2.0 * ca * cg * hbg + cg * cg * gHg;
      double linearGain = 2.0 * bh - hHh;
      R.norm_dl = std::sqrt(std::max(0.0, dl2));
      hipLaunchKernelGGL(k_dogleg_oplus, dim3((nv + WG - 1) / WG), dim3(WG), 0, stream, nv, (const int32_t*)d_hidx,
                         (const double*)d_b, (const double*)d_x, ca, cg, d_states, mopts(),
                         use_direct ? (const DevScalars*)d_sc : nullptr, d_backup, fail_token);
      HIPCHK(hipGetLastError());
      double newChi = 0.0;
      rc = chi2(&newChi, err, phase_timing ? ev_ph[3] : nullptr);
      if (rc) return rc;
      kt.n_update += 1;
      rc = phase_ms(1, 3, T.ms_update, err);
      if (rc) return rc;
      if (std::fabs(linearGain) < 1e-12) linearGain = 1e-12;
      rho = (currentChi - newChi) / linearGain;
      if (rho > 0) {  // discardTop
        currentChi = newChi;
        good = true;
      } else {
        pop_states();
      }
      if (rho > 0.75) delta = std::max(delta, 3.0 * R.norm_dl);
      else if (rho < 0.25) delta *= 0.5;
      if (opt.verbose >= 2)
        std::fprintf(stderr, "  trial %d: step %d, ||h_dl|| %.6g, rho %.6g, delta %.6g\n", tries, R.step, R.norm_dl,
                     rho, delta);
    } while (!good && tries < opt.dl_max_trials);
    R.delta_after = delta;
    tr_stats.push_back(R);
    T.rho = rho;
    T.trials = tries;
    iter_end(T, currentChi, stats);
    ++iters;
    if (opt.verbose)
      std::fprintf(stderr,
                   "iteration= %d\t chi2= %.9g\t delta= %.6g\t step= %d\t numTries= %d\t lambda= %.6g\t pcg= %d "
                   "(rel %.2e)\t ms lin/solve/upd= %.3f/%.3f/%.3f\n",
                   it, currentChi, delta, R.step, tries, T.lambda, T.pcg_iters, T.pcg_rel_res, T.ms_linearize,
                   T.ms_solve, T.ms_update);
    if (!good) ok_all = false;  // Terminate
  }
  HIPCHK(hipStreamSynchronize(stream));
  return iters;
}

}  // namespace sim3opt
