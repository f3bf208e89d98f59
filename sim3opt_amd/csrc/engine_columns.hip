// engine_columns.hip -- blocks of (H + lambda I)^-1 by columns of the inverse: SparseOptimizer::computeMarginals and the
// gate of candidate edges on the graphs the PCG was built for, where the exact block Cholesky behind
// Engine::cov_blocks (engine_direct.hip) is refused.  Block (a, b) is rows a of the seven solutions of
// (H + lambda I) y = e_{7 b + c}: the request is covered by vertices (col_plan.hpp), their columns are solved by the
// PCG the graph was initialised with -- on a multigrid graph up to KB columns per pass over the blocks, through
// pcg_batch with per-system right-hand sides and one set-up for all of them (they share lambda) -- and every column is
// accepted on its TRUE residual g - (H + lambda I) y, formed by the SpMV, in the 2-norm against options.cov_rel_tol;
// a column above it is refined at most twice (solve for the residual, add).  Per column the arithmetic does not depend
// on the columns that share its batch (the batch's guarantee), so a block's bits depend on the endpoint the cover chose
// and on nothing else of the request.  What the solves write of the solver's state is put back.
#include "engine_impl.hpp"
#include "col_plan.hpp"

namespace sim3opt {

#include "col_kernels.hpp"

int Engine::cols_alloc(std::string& err) {
  if (c_g) return SIM3OPT_OK;
  c_vs = pad64(n);
  double** v0[] = {&c_g, &c_y, &c_r, &c_d};
  for (double** v : v0) HIPCHK(cols_mem.alloc(*v, (size_t)KB * c_vs, stream));
  HIPCHK(cols_mem.raw(c_nrm, 2 * KB));
  return SIM3OPT_OK;
}

void Engine::cols_release() {
  cols_mem.release();
  c_g = c_y = c_r = c_d = c_nrm = nullptr;
}

int Engine::cols_solve(double lambda, int nsys, const double* g, const double* tol, bool setup, const double** x,
                       int32_t* iters, bool* failed, std::string& err) {
  const int width = cols_batch_width();
  for (int s = 0; s < nsys; ++s) iters[s] = 0;
  if (width > 0) {
    double lams[KB], rel[KB];
    bool capped[KB], usable = false;
    for (int s = 0; s < KB; ++s) lams[s] = lambda;
    const BatchRhs rhs{g, c_vs, tol, setup};
    int rc = pcg_batch(lams, nsys, iters, rel, capped, &usable, err, &rhs);
    if (rc) return rc;
    for (int s = 0; s < nsys; ++s) {
      // (a failed pivot of the shared set-up is raised on system 0 and ends the batch before its first step)
      failed[s] = h_bsc[s].fail != 0 || h_bsc[0].fail != 0;
      x[s] = b_x + (size_t)s * b_vs;
    }
    return SIM3OPT_OK;
  }
  // one column at a time through the one-system view, with its right-hand side and tolerance
  int rc = SIM3OPT_OK;
  for (int s = 0; s < nsys && rc == SIM3OPT_OK; ++s) {  // (nsys = 1 here)
    bool ok = true, broke = false;
    double rr = 0.0;
    rc = pcg_attempt(lambda, use_amg ? 2 : (use_chain ? 1 : 0), &iters[s], &rr, &ok, &broke, err, 0, nullptr,
                     g + (size_t)s * c_vs, tol[s]);
    failed[s] = !ok || broke;
    x[s] = d_x;
  }
  return rc;
}

int Engine::cols_true_residuals(double lambda, int cnt, const int* sys, double* rel, std::string& err) {
  const int ge = grid_for(n / 2, WG);
  for (int j = 0; j < cnt; ++j) {
    const size_t o = (size_t)sys[j] * c_vs;
    spmv_raw(lambda, c_y + o, d_q, nullptr, nullptr);
    hipLaunchKernelGGL(k_cols_residual, dim3(ge), dim3(WG), 0, stream, (int64_t)n, (const double*)(c_g + o),
                       (const double*)d_q, c_r + o);
    norms2(c_r + o, c_g + o, d_part_a, d_part_b, c_nrm + 2 * sys[j]);
  }
  HIPCHK(hipGetLastError());
  double h[2 * KB];
  HIPCHK(hipMemcpyAsync(h, c_nrm, sizeof(h), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (int j = 0; j < cnt; ++j) {
    const double rr = h[2 * sys[j]], gg = h[2 * sys[j] + 1];
    rel[j] = gg > 0.0 && rr == rr ? std::sqrt(rr / gg) : (rr == 0.0 ? 0.0 : INFINITY);
  }
  return SIM3OPT_OK;
}

int Engine::inverse_columns(double lambda, int32_t nvert, const int32_t* vertices, const int32_t* first,
                            const int32_t* blk_row, double* blocks, std::string& err) {
  const std::string pre = "columns of the inverse: ";
  for (int64_t& v : col_counts) v = 0;
  col_res[0] = 0.0;
  col_res[1] = opt.cov_rel_tol;
  col_fail_vertex = -1;
  if (comm.world > 1) {
    err = pre + "one GPU only (the graph is partitioned over ranks)";
    return SIM3OPT_ERR_STATE;
  }
  if (use_direct) {
    err = pre + "options.cov_solver needs a graph initialised on the PCG path (linear_solver = 0); this one factorises "
          "exactly -- cov_solver = 0 is the path for it";
    return SIM3OPT_ERR_STATE;
  }
  const sim3opt_kernel_times kt0 = kt;  // (not one of the optimiser's linearisations: the counters stay)
  int rc = linearize(err);  // H at the current estimates (b is rewritten with the values it has)
  kt = kt0;
  if (rc) return rc;
  if (nvert == 0) return SIM3OPT_OK;
  rc = cols_alloc(err);
  if (rc) return rc;
  const int width = cols_batch_width();
  if (width > 0 && (rc = batch_alloc(err))) return rc;
  SolverSnapshot snap;  // (after batch_alloc: the batch's scalars are in it)
  if ((rc = snap.take(*this, err))) return rc;
  // one set-up for all systems of a batch: slot 0 of the smoother inverses, the FP32 diagonals and the dense inverse --
  // a mode of this call, not solver state: the strides go to zero here and come back below
  std::vector<int64_t> ms_saved;
  const int64_t as_saved = cv_batch.as;
  if (width > 0) {
    for (CycleLevel& B : cv_batch.lv) {
      ms_saved.push_back(B.ms);
      B.ms = 0;
    }
    cv_batch.as = 0;
    pv_batch.ms = 0;
  }

  const int32_t nblk = first[nvert];
  DevBuf<int32_t> d_rows;  // (they go after the put-back's synchronisation)
  DevBuf<double> d_blocks;
  std::vector<double> out((size_t)49 * std::max(nblk, 1));
  auto body = [&]() -> int {
    HIPCHK(d_rows.alloc((size_t)std::max(nblk, 1)));
    HIPCHK(d_blocks.alloc(49 * (size_t)std::max(nblk, 1)));
    HIPCHK(hipMemcpyAsync(d_rows, blk_row, sizeof(int32_t) * (size_t)nblk, hipMemcpyHostToDevice, stream));
    const double ctol = opt.cov_rel_tol;
    double first_pass = 0.01;
    // (tuning, and the test of the refinement: 1 leaves the true residual above the bound on most graphs)
    if (const char* ev = std::getenv("SIM3OPT_COLS_FIRST_PASS"))
      if (std::atof(ev) > 0.0 && std::atof(ev) <= 1.0) first_pass = std::atof(ev);
    const int64_t total = (int64_t)7 * nvert;
    const int per = width > 0 ? width : 1;
    const int ge = grid_for(n / 2, WG);
    const size_t vbytes = sizeof(double) * (size_t)n;
    bool setup = true;
    for (int64_t c0 = 0; c0 < total; c0 += per) {
      const int nsys = (int)std::min<int64_t>(per, total - c0);
      ColUnits u;
      for (int s = 0; s < KB; ++s) u.at[s] = s < nsys ? (int64_t)7 * vertices[(c0 + s) / 7] + (c0 + s) % 7 : -1;
      BATCH_DISPATCH(nsys, hipLaunchKernelGGL((k_cols_rhs<KS>), dim3(ge), dim3(WG), 0, stream, (int64_t)n, c_vs, c_g, u));
      HIPCHK(hipGetLastError());
      // the PCG stops on ||r||_Minv, which the square root of the preconditioner's condition number separates from
      // the 2-norm: two digits below the bound (each costs a few iterations; a refinement costs a solve with its
      // set-up), and what they do not cover the refinement does
      double tol[KB], rel[KB];
      const double* x[KB];
      int32_t its[KB] = {0, 0, 0, 0};
      bool failed[KB];
      int sys[KB];
      for (int s = 0; s < KB; ++s) tol[s] = first_pass * ctol;
      int rc2 = cols_solve(lambda, nsys, c_g, tol, setup, x, its, failed, err);
      if (rc2) return rc2;
      setup = false;
      col_counts[4] += 1;
      for (int s = 0; s < nsys; ++s) {
        col_counts[2] += its[s];
        if (failed[s]) {
          col_fail_vertex = st.row2vertex[vertices[(c0 + s) / 7]];
          err = pre + "the PCG broke down or its set-up met a non-positive pivot (column " + std::to_string((c0 + s) % 7) +
                " of vertex #" + std::to_string(col_fail_vertex) + "): H + lambda I is not positive definite";
          return SIM3OPT_ERR_STATE;
        }
        HIPCHK(hipMemcpyAsync(c_y + (size_t)s * c_vs, x[s], vbytes, hipMemcpyDeviceToDevice, stream));
        sys[s] = s;
      }
      rc2 = cols_true_residuals(lambda, nsys, sys, rel, err);
      if (rc2) return rc2;
      double relc[KB];  // per system of the batch
      for (int s = 0; s < nsys; ++s) relc[s] = rel[s];
      for (int round = 0; round < 2; ++round) {
        int bad[KB], nbad = 0;
        for (int s = 0; s < nsys; ++s)
          if (!(relc[s] <= ctol)) bad[nbad++] = s;
        if (nbad == 0) break;
        col_counts[3] += 1;
        // solve for the residuals (to what is still missing, relative to them), add, look again
        for (int j0 = 0; j0 < nbad; j0 += per) {
          const int m = std::min(per, nbad - j0);
          for (int j = 0; j < m; ++j) {
            const int s = bad[j0 + j];
            HIPCHK(hipMemcpyAsync(c_d + (size_t)j * c_vs, c_r + (size_t)s * c_vs, vbytes, hipMemcpyDeviceToDevice, stream));
            tol[j] = std::isfinite(relc[s]) ? std::min(0.1, 0.1 * ctol / relc[s]) : 0.1;
          }
          rc2 = cols_solve(lambda, m, c_d, tol, false, x, its, failed, err);
          if (rc2) return rc2;
          for (int j = 0; j < m; ++j) {
            const int s = bad[j0 + j];
            col_counts[2] += its[j];
            if (failed[j]) continue;  // (the column keeps its residual and is reported below)
            hipLaunchKernelGGL(k_cols_axpy, dim3(ge), dim3(WG), 0, stream, (int64_t)n, x[j], c_y + (size_t)s * c_vs);
            if (width == 0) {  // (one system: d_x is the next solve's too)
              rc2 = cols_true_residuals(lambda, 1, &s, &relc[s], err);
              if (rc2) return rc2;
            }
          }
          HIPCHK(hipGetLastError());
        }
        if (width > 0) {
          rc2 = cols_true_residuals(lambda, nbad, bad, rel, err);
          if (rc2) return rc2;
          for (int j = 0; j < nbad; ++j) relc[bad[j]] = rel[j];
        }
      }
      for (int s = 0; s < nsys; ++s) {
        if (relc[s] == relc[s]) col_res[0] = std::max(col_res[0], relc[s]);
        if (!(relc[s] <= ctol)) {
          col_fail_vertex = st.row2vertex[vertices[(c0 + s) / 7]];
          char buf[96];
          std::snprintf(buf, sizeof(buf), "%.3e, above cov_rel_tol = %.3e", relc[s], ctol);
          err = pre + "column " + std::to_string((c0 + s) % 7) + " of vertex #" + std::to_string(col_fail_vertex) +
                " reached ||g - (H + lambda I) y|| / ||g|| = " + buf +
                " after two rounds of refinement: pass a lambda > 0 (cond x eps is the floor), a larger cov_rel_tol "
                "or more pcg_max_iters";
          return SIM3OPT_ERR_STATE;
        }
        const int32_t v = (int32_t)((c0 + s) / 7), cnt = first[v + 1] - first[v];
        if (cnt > 0)
          hipLaunchKernelGGL(k_cols_gather, dim3(grid_for(7 * (int64_t)cnt, WG)), dim3(WG), 0, stream, first[v], cnt,
                             (int32_t)((c0 + s) % 7), (const int32_t*)d_rows, (const double*)(c_y + (size_t)s * c_vs),
                             d_blocks.get());
      }
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out.data(), d_blocks, sizeof(double) * 49 * (size_t)nblk, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return SIM3OPT_OK;
  };
  rc = snap.put_back(body(), err);
  if (width > 0) {
    for (size_t l = 0; l < cv_batch.lv.size(); ++l) cv_batch.lv[l].ms = ms_saved[l];
    cv_batch.as = as_saved;
    pv_batch.ms = ms_saved[0];
  }
  if (rc) return rc;
  col_counts[0] = nvert;
  col_counts[1] = (int64_t)7 * nvert;
  std::memcpy(blocks, out.data(), sizeof(double) * 49 * (size_t)nblk);
  return SIM3OPT_OK;
}

// The request of Engine::cov_blocks by columns: cover, solve, lay out.  Each unordered pair is computed once, from the
// endpoint the cover chose; the reversed pair is its exact transpose, a diagonal block is symmetrised as (B + B^T) / 2.
int Engine::cov_blocks_columns(const std::string& pre, bool fixed_zero, double lambda, int32_t n, const int32_t* row_a,
                               const int32_t* row_b, double* cov, std::string& err) {
  for (int64_t& v : cov_stats) v = 0;  // (the exact path's counters)
  for (int32_t q = 0; q < n; ++q) {
    if (fixed_zero && (row_a[q] < 0 || row_b[q] < 0)) continue;
    if (row_a[q] < 0 || row_b[q] < 0 || row_a[q] >= nb || row_b[q] >= nb) {
      err = pre + "fixed vertex in a pair";
      return SIM3OPT_ERR_ARG;
    }
  }
  ColumnCover C;
  covariance_columns_cover(nb, n, row_a, row_b, C);
  const int32_t nvert = (int32_t)C.chosen.size(), np = (int32_t)C.pairs.size();
  // the blocks of a chosen vertex b: (a, b) for every pair {a, b} it covers
  std::vector<int32_t> first(nvert + 1, 0), blk_of(np), blk_row(std::max(np, 1));
  for (int32_t k = 0; k < np; ++k) ++first[C.owner[k] + 1];
  for (int32_t v = 0; v < nvert; ++v) first[v + 1] += first[v];
  {
    std::vector<int32_t> fill(first.begin(), first.end() - 1);
    for (int32_t k = 0; k < np; ++k) {
      const int32_t b = C.chosen[C.owner[k]];
      blk_of[k] = fill[C.owner[k]]++;
      blk_row[blk_of[k]] = C.pairs[k].first == b ? C.pairs[k].second : C.pairs[k].first;
    }
  }
  std::vector<double> blocks((size_t)49 * std::max(np, 1));
  int rc = inverse_columns(lambda, nvert, C.chosen.data(), first.data(), blk_row.data(), blocks.data(), err);
  if (rc) {
    if (rc == SIM3OPT_ERR_STATE) err = pre + err;
    return rc;
  }
  for (size_t k = 0; k < (size_t)49 * np; ++k)
    if (!std::isfinite(blocks[k])) {
      err = pre + "non-finite result";
      return SIM3OPT_ERR_STATE;
    }
  for (int32_t q = 0; q < n; ++q) {
    double* dst = cov + (size_t)49 * q;
    const int32_t k = C.pair_of[q];
    if (k < 0) {
      for (int e = 0; e < 49; ++e) dst[e] = 0.0;
      continue;
    }
    const double* src = blocks.data() + (size_t)49 * blk_of[k];
    const int32_t b = C.chosen[C.owner[k]];
    if (row_a[q] == row_b[q]) {
      for (int c = 0; c < 7; ++c)
        for (int r = 0; r < 7; ++r) dst[r + 7 * c] = 0.5 * (src[r + 7 * c] + src[c + 7 * r]);
    } else if (row_b[q] == b) {  // stored as (a, b): rows a, columns b
      std::memcpy(dst, src, sizeof(double) * 49);
    } else {
      for (int c = 0; c < 7; ++c)
        for (int r = 0; r < 7; ++r) dst[r + 7 * c] = src[c + 7 * r];
    }
  }
  return SIM3OPT_OK;
}

// ---- diagnostic read-out of the four kernels above (include/sim3opt.h, "Diagnostic."; tests/test_gpu_column_vectors.py) ----
// One kernel per call, on the caller's data staged in the c_* buffers a column solve uses, at a length nvec <= 7 nb of
// the caller's choice (the kernels take any length; a solve passes 7 nb).  `out` is read and written: what it holds on
// entry is what the kernel's output buffer holds before the launch.  Every index the kernels dereference is checked
// here first.
int Engine::debug_column_vectors(int32_t op, int32_t grid, int64_t nvec, int32_t K, const int64_t* at, int32_t sys,
                                 const double* a, const double* b, int32_t first, int32_t count, int32_t col,
                                 const int32_t* rows, int32_t n_blocks, double* out, std::string& err) {
  const std::string pre = "debug_column_vectors: ";
  if (comm.world > 1) {
    err = pre + "one GPU only (the graph is partitioned over ranks)";
    return SIM3OPT_ERR_STATE;
  }
  if (use_direct) {
    err = pre + "the column kernels belong to a graph initialised on the PCG path (linear_solver = 0); this one "
          "factorises exactly";
    return SIM3OPT_ERR_STATE;
  }
  if (!linearized) {
    err = pre + "call sim3opt_linearize (or optimize) first";
    return SIM3OPT_ERR_STATE;
  }
  if (grid < 0 || grid > MAX_GRID) {
    err = pre + "grid out of range";
    return SIM3OPT_ERR_ARG;
  }
  if (op < 0 || op > 3 || !out) {
    err = pre + "unknown kernel or null output";
    return SIM3OPT_ERR_ARG;
  }
  if (nvec < 1 || nvec > (int64_t)n) {
    err = pre + "vector length out of range (1 .. 7 x block rows)";
    return SIM3OPT_ERR_ARG;
  }
  if (op == 0) {
    if (K < 1 || K > KB || !at) {
      err = pre + "k_cols_rhs takes 1 .. 4 systems and their unit entries";
      return SIM3OPT_ERR_ARG;
    }
    for (int s = 0; s < K; ++s)
      if (at[s] >= nvec) {
        err = pre + "unit entry past the end of the vector";
        return SIM3OPT_ERR_ARG;
      }
  } else if (sys < 0 || sys >= KB || !a || (op == 1 && !b)) {
    err = pre + "system index out of range or null input";
    return SIM3OPT_ERR_ARG;
  }
  if (op == 3) {
    if (first < 0 || count < 0 || n_blocks < 1 || (int64_t)first + count > n_blocks || col < 0 || col > 6 || !rows) {
      err = pre + "k_cols_gather: blocks [first, first + count) must lie in the output, col in 0 .. 6";
      return SIM3OPT_ERR_ARG;
    }
    for (int32_t k = first; k < first + count; ++k)
      if (rows[k] < 0 || (int64_t)7 * rows[k] + 7 > nvec) {
        err = pre + "k_cols_gather: a row past the end of the vector";
        return SIM3OPT_ERR_ARG;
      }
  }
  int rc = cols_alloc(err);
  if (rc) return rc;
  SolverSnapshot snap;
  if ((rc = snap.take(*this, err))) return rc;
  DevBuf<int32_t> d_rows;  // (they go after the put-back's synchronisation)
  DevBuf<double> d_blocks;
  auto body = [&]() -> int {
    const int ge = grid > 0 ? grid : grid_for(nvec / 2, WG);
    const size_t vb = sizeof(double) * (size_t)nvec, sb = sizeof(double) * (size_t)c_vs, o = (size_t)sys * c_vs;
    if (op == 0) {
      HIPCHK(hipMemcpy(c_g, out, sb * K, hipMemcpyHostToDevice));
      ColUnits u;
      for (int s = 0; s < KB; ++s) u.at[s] = s < K ? at[s] : -1;
      BATCH_DISPATCH(K, hipLaunchKernelGGL((k_cols_rhs<KS>), dim3(ge), dim3(WG), 0, stream, nvec, c_vs, c_g, u));
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(stream));
      HIPCHK(hipMemcpy(out, c_g, sb * K, hipMemcpyDeviceToHost));
    } else if (op == 1) {  // (q staged in c_d, which no kernel of this call reads otherwise; a column solve passes d_q)
      HIPCHK(hipMemcpy(c_g + o, a, vb, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(c_d + o, b, vb, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(c_r + o, out, sb, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_cols_residual, dim3(ge), dim3(WG), 0, stream, nvec, (const double*)(c_g + o),
                         (const double*)(c_d + o), c_r + o);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(stream));
      HIPCHK(hipMemcpy(out, c_r + o, sb, hipMemcpyDeviceToHost));
    } else if (op == 2) {
      HIPCHK(hipMemcpy(c_d + o, a, vb, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(c_y + o, out, sb, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_cols_axpy, dim3(ge), dim3(WG), 0, stream, nvec, (const double*)(c_d + o), c_y + o);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(stream));
      HIPCHK(hipMemcpy(out, c_y + o, sb, hipMemcpyDeviceToHost));
    } else {
      HIPCHK(d_rows.alloc((size_t)n_blocks));
      HIPCHK(d_blocks.alloc(49 * (size_t)n_blocks));
      HIPCHK(hipMemcpy(d_rows, rows, sizeof(int32_t) * (size_t)(first + count), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_blocks, out, sizeof(double) * 49 * (size_t)n_blocks, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(c_y + o, a, vb, hipMemcpyHostToDevice));
      if (count > 0)
        hipLaunchKernelGGL(k_cols_gather, dim3(grid > 0 ? grid : grid_for(7 * (int64_t)count, WG)), dim3(WG), 0, stream,
                           first, count, col, (const int32_t*)d_rows, (const double*)(c_y + o), d_blocks.get());
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(stream));
      HIPCHK(hipMemcpy(out, d_blocks, sizeof(double) * 49 * (size_t)n_blocks, hipMemcpyDeviceToHost));
    }
    return SIM3OPT_OK;
  };
  return snap.put_back(body(), err);
}

int engine_debug_column_vectors(Engine* e, int32_t op, int32_t grid, int64_t n, int32_t K, const int64_t* at,
                                int32_t sys, const double* a, const double* b, int32_t first, int32_t count,
                                int32_t col, const int32_t* rows, int32_t n_blocks, double* out, std::string& err) {
  return e->debug_column_vectors(op, grid, n, K, at, sys, a, b, first, count, col, rows, n_blocks, out, err);
}

void engine_covariance_columns_stats(const Engine* e, int64_t counts[5], double res[2], int32_t* failed_vertex) {
  for (int k = 0; k < 5; ++k) counts[k] = e->col_counts[k];
  res[0] = e->col_res[0];
  res[1] = e->col_res[1];
  if (failed_vertex) *failed_vertex = e->col_fail_vertex;
}

}  // namespace sim3opt
