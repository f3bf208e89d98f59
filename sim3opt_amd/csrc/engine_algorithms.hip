// engine_algorithms.hip -- the nonlinear algorithms besides Levenberg-Marquardt (g2o: OptimizationAlgorithmGaussNewton
// and OptimizationAlgorithmDogleg behind SparseOptimizer::setAlgorithm), on the engine's linearisation, solvers and
// chi2.  Engine::optimize hands options.algorithm = 1 / 2 here.  The rules are written out in DESIGN.md 5h.
#include "engine_impl.hpp"
#include "dogleg_rule.hpp"

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
int Engine::dogleg_dots(std::string& err, int grid, int64_t j0, int64_t j1) {
  const int gs = spmv_grid();
  double* out = d_dl + 4 * MAX_GRID + DL_OUT;
  // q = H b (lambda = 0): its v.q partials are b^T H b
  spmv_raw(0.0, d_b, d_q, nullptr, nullptr);
  hipLaunchKernelGGL(k_dl_sum, dim3(1), dim3(WG), 0, stream, (const double*)d_part_a, gs, out + DL_BHB);
  // H h_gn into the PCG's (now unused) direction vector: its v.q partials are h_gn^T H h_gn
  spmv_raw(0.0, d_x, d_p, nullptr, nullptr);
  if (j1 < 0) {  // this rank's rows
    j0 = 7 * (int64_t)r0;
    j1 = 7 * (int64_t)r1;
  }
  const int gd = grid > 0 ? grid : grid_for(7 * (int64_t)(r1 - r0), WG);
  hipLaunchKernelGGL(k_dl_dots, dim3(gd), dim3(WG), 0, stream, (int)j0, (int)j1, (const double*)d_b,
                     (const double*)d_x, (const double*)d_q, d_dl);
  hipLaunchKernelGGL(k_dl_final, dim3(1), dim3(WG), 0, stream, (const double*)d_dl, gd, (const double*)d_part_a, gs,
                     out);
  HIPCHK(hipGetLastError());
  if (comm.active()) return comm.allreduce(out, 6, 0, stream, err);
  return SIM3OPT_OK;
}

// the dogleg's buffers, allocated at their first use (an optimize() with options.algorithm = 2, or the read-out)
int Engine::dogleg_alloc(std::string& err) {
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
  return SIM3OPT_OK;
}

// one trial's update: backup <- S, S <- exp(ca b + cg h_gn) S on the free vertices (k_dogleg_oplus)
void Engine::dogleg_step(double ca, double cg) {
  hipLaunchKernelGGL(k_dogleg_oplus, dim3((nv + WG - 1) / WG), dim3(WG), 0, stream, nv, (const int32_t*)d_hidx,
                     (const double*)d_b, (const double*)d_x, ca, cg, d_states, mopts(),
                     use_direct ? (const DevScalars*)d_sc : nullptr, d_backup, fail_token);
}

// ---- diagnostic read-out of the dogleg's launches (include/sim3opt.h, "Diagnostic."; tests/test_gpu_dogleg_operators.py)
int Engine::debug_dogleg(const double* h_gn, double ca, double cg, bool with_fail, int32_t grid, int64_t j0, int64_t j1,
                         double* scalars, double* states_out, double* backup_out, std::string& err) {
  if (comm.active()) {
    err = "debug_dogleg: a partitioned graph holds this rank's share only (one GPU, please)";
    return SIM3OPT_ERR_STATE;
  }
  if (!linearized) {
    err = "debug_dogleg: call sim3opt_linearize (or optimize) first: the model needs H and b";
    return SIM3OPT_ERR_STATE;
  }
  if (with_fail && !use_direct) {
    err = "debug_dogleg: with_fail needs the exact solver (only its failure token reaches k_dogleg_oplus)";
    return SIM3OPT_ERR_STATE;
  }
  if (grid < 0 || grid > MAX_GRID) {
    err = "debug_dogleg: grid out of range";
    return SIM3OPT_ERR_ARG;
  }
  if (j0 < 0 || j0 > j1 || j1 > (int64_t)n) {
    err = "debug_dogleg: entry range out of bounds (0 <= j0 <= j1 <= 7 x block rows)";
    return SIM3OPT_ERR_ARG;
  }
  int rc = dogleg_alloc(err);
  if (rc) return rc;
  // everything these launches overwrite that a later call could see
  SolverSnapshot snap;
  rc = snap.take(*this, err, true);
  if (rc) return rc;
  const bool whole = j0 == 0 && j1 == 0;
  bool pushed = false;
  double six[6] = {0, 0, 0, 0, 0, 0};
  auto body = [&]() -> int {
    // h_gn where the solve leaves its solution
    HIPCHK(hipMemcpy(d_x, h_gn, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    if (with_fail) {
      const int32_t token = fail_token;  // what the factorisation of the current solve stores on a bad pivot
      HIPCHK(hipMemcpy(&d_sc->fail, &token, sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (scalars) {  // the launches and the read of an iteration after its solve (optimize_dogleg)
      const int rc2 = whole ? dogleg_dots(err, grid) : dogleg_dots(err, grid, j0, j1);
      if (rc2) return rc2;
      HIPCHK(hipMemcpyAsync(h_dl, d_dl + 4 * MAX_GRID + DL_OUT, sizeof(double) * 6, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      for (int k = 0; k < 6; ++k) six[k] = h_dl[k];
    }
    if (states_out || backup_out) {  // ... and of a trial
      pushed = true;
      dogleg_step(ca, cg);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(stream));
      if (states_out) HIPCHK(hipMemcpy(states_out, d_states, sizeof(Sim3) * (size_t)nv, hipMemcpyDeviceToHost));
      if (backup_out) HIPCHK(hipMemcpy(backup_out, d_backup, sizeof(Sim3) * (size_t)nv, hipMemcpyDeviceToHost));
    }
    return SIM3OPT_OK;
  };
  rc = body();
  if (pushed) pop_states();  // (the backup was taken whatever followed it)
  rc = snap.put_back(rc, err);
  if (rc) return rc;
  if (scalars)
    for (int k = 0; k < 6; ++k) scalars[k] = six[k];
  return SIM3OPT_OK;
}

int engine_debug_dogleg(Engine* e, const double* h_gn, double ca, double cg, bool with_fail, int32_t grid, int64_t j0,
                        int64_t j1, double* scalars, double* states_out, double* backup_out, std::string& err) {
  return e->debug_dogleg(h_gn, ca, cg, with_fail, grid, j0, j1, scalars, states_out, backup_out, err);
}

// the step rule on the host (sim3opt_dogleg_rule): the functions optimize_dogleg calls, in this translation unit
void engine_dogleg_rule(const double scalars[6], double delta, double model[3], double trial[4], int32_t* step) {
  const DoglegScalars S{scalars[DL_BB], scalars[DL_BHB], scalars[DL_GG], scalars[DL_BG], scalars[DL_HBG], scalars[DL_GHG]};
  const DoglegModel M = dogleg_model(S);
  const DoglegTrial D = dogleg_trial(S, M, delta);
  model[0] = M.alpha;
  model[1] = M.norm_sd;
  model[2] = M.norm_gn;
  trial[0] = D.ca;
  trial[1] = D.cg;
  trial[2] = D.norm_dl;
  trial[3] = D.linear_gain;
  *step = D.step;
}

int Engine::optimize_dogleg(int32_t max_iters, std::vector<sim3opt_iter_stats>& stats, std::string& err) {
  const int rc0 = dogleg_alloc(err);
  if (rc0) return rc0;
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
    const DoglegScalars S{h_dl[DL_BB], h_dl[DL_BHB], h_dl[DL_GG], h_dl[DL_BG], h_dl[DL_HBG], h_dl[DL_GHG]};
    const DoglegModel M = dogleg_model(S);  // h_sd = alpha b
    R.alpha = M.alpha;
    R.norm_sd = M.norm_sd;
    R.norm_gn = M.norm_gn;
    int tries = 0;
    bool good = false;
    double rho = 0.0;
    do {
      ++tries;
      if (phase_timing) HIPCHK(hipEventRecord(ev_ph[1], stream));
      const DoglegTrial D = dogleg_trial(S, M, delta);  // h_dl = ca b + cg h_gn (dogleg_rule.hpp)
      double linearGain = D.linear_gain;
      R.step = D.step;
      R.norm_dl = D.norm_dl;
      dogleg_step(D.ca, D.cg);
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
