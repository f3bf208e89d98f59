// batch_kernels.hpp -- the vector kernels of the PCG loop for K right-hand sides at once (included by
// engine_batch.hip only, inside namespace sim3opt): the rejected trials of one LM iteration solve
// (H + lambda_k I) x_k = b for a KNOWN sequence lambda_k (g2o's OptimizationAlgorithmLevenberg: lambda *= nu,
// nu *= 2 after every rejection), so after the first rejection the next K systems are solved together and the
// trials are then evaluated in g2o's order.  What LinearSolverEigen does K times in a row (kitti_surf.cpp:553-554,
// 675).  Every kernel here performs, per system, the operations of its one-system counterpart (pcg_kernels.hpp) in
// the same order: the K solutions are bit for bit those of K sequential solves (asserted in
// tests/test_gpu_parity.py).  Vectors of system s live at base + s * stride (BatchStrides, spmv_kernel.hpp).
// Everything else of a batched iteration has no twin: the SpMV (spmv_kernel.hpp) and the multigrid cycle's
// transfer kernels (amg_kernels.hpp) are templates on K whose one-system kernel is the K = 1 instantiation.
#pragma once

// ------------------------------------------------------------------------------------------
// PCG vector kernels for K systems (k_pcg_init / k_pcg_step / k_final_sum2 per system; b is shared -- or, OWNB: the
// columns of the inverse, engine_columns.hip -- system s has its own right-hand side b + s * bstride)
// ------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(WG) void k_final_sum2_k(const double* __restrict__ pa, const double* __restrict__ pb,
                                                     int n, int pstride, DevScalars* __restrict__ sc) {
  __shared__ double sh[4];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const double a = sum_partials(pa + (size_t)s * pstride, n, sh);
    const double b = sum_partials(pb + (size_t)s * pstride, n, sh);
    if (threadIdx.x == 0) {
      sc[s].tmp_pq = a;
      sc[s].tmp_rz = b;
    }
  }
}

template <int K, bool OWNB = false>
__global__ __launch_bounds__(WG) void k_pcg_init_k(int r0, int r1, const double* __restrict__ b,
                                                   const double* __restrict__ Minv, double* __restrict__ x,
                                                   double* __restrict__ r, double* __restrict__ z,
                                                   double* __restrict__ p, double* __restrict__ sv,
                                                   BatchStrides bs, int64_t bstride = 0) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sub = lane / 7, rr = lane % 7, base = lane - rr;
  for (int row0 = r0 + (blockIdx.x * 4 + wave) * 9; row0 < r1; row0 += gridDim.x * 36) {
    const int row = row0 + sub;
    const bool act = lane < 63 && row < r1;
    const size_t j = (size_t)7 * row + rr;
    double rv = act ? b[j] : 0.0;
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const size_t o = (size_t)s * bs.vec;
      if (OWNB && s > 0) rv = act ? b[(size_t)s * bstride + j] : 0.0;
      if (act) {
        x[o + j] = 0.0;
        r[o + j] = rv;
        p[o + j] = 0.0;
        sv[o + j] = 0.0;
      }
      double zv = 0.0;
#pragma unroll
      for (int cc = 0; cc < 7; ++cc) {
        const double rc = __shfl(rv, base + cc);
        if (act) zv += Minv[(size_t)s * bs.minv + (size_t)49 * row + 7 * rr + cc] * rc;
      }
      if (act) z[o + j] = zv;
    }
  }
}

// k_pcg_step for K systems: every system has its own scalars (sc[s]); a finished system is left alone.
// it >= 0: the launch number (0 = first iteration of every system); the systems run in lock-step, a system
// that converges earlier just stops being updated.
template <int K>
__global__ __launch_bounds__(WG) void k_pcg_step_k(int r0, int r1, int par, int it,
                                                   const double* __restrict__ Minv, const double* zin,
                                                   double* zout, const double* __restrict__ w,
                                                   double* __restrict__ p, double* __restrict__ sv,
                                                   double* __restrict__ x, double* __restrict__ r,
                                                   DevScalars* sc, BatchStrides bs) {
  double alpha[K], beta[K];
  bool live[K];
  const bool commit = blockIdx.x == 0 && threadIdx.x == 0;
  const bool first = it == 0;
  bool any = false;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    live[s] = false;
    alpha[s] = beta[s] = 0.0;
    if (sc[s].done) continue;
    const double delta = sc[s].tmp_pq, gamma = sc[s].tmp_rz;
    const double gamma0 = first ? gamma : sc[s].rz0;
    if (!(gamma == gamma) || gamma < 0.0 || gamma <= sc[s].tol2 * gamma0 || (first && gamma == 0.0)) {
      if (commit) {
        if (!(gamma == gamma) || gamma < 0.0) sc[s].fail = 1;
        if (first) sc[s].rz0 = gamma;
        sc[s].rz[par ^ 1] = gamma;
        sc[s].gam_last = gamma;
        sc[s].done = 1;
      }
      continue;
    }
    beta[s] = first ? 0.0 : gamma / sc[s].rz[par];
    const double denom = first ? delta : delta - beta[s] * gamma / sc[s].alpha[par];
    if (!(denom > 0.0) || !(denom < DBL_MAX)) {
      if (commit) {
        sc[s].fail = 1;
        sc[s].done = 1;
      }
      continue;
    }
    alpha[s] = gamma / denom;
    live[s] = true;
    any = true;
  }
  if (!any) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sub = lane / 7, rr = lane % 7, base = lane - rr;
  for (int row0 = r0 + (blockIdx.x * 4 + wave) * 9; row0 < r1; row0 += gridDim.x * 36) {
    const int row = row0 + sub;
    const bool act = lane < 63 && row < r1;
    const size_t j = (size_t)7 * row + rr;
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if (!live[s]) continue;  // (uniform over the grid)
      const size_t o = (size_t)s * bs.vec;
      double rv = 0.0;
      if (act) {
        const double pn = zin[o + j] + beta[s] * p[o + j];
        const double sn = w[o + j] + beta[s] * sv[o + j];
        p[o + j] = pn;
        sv[o + j] = sn;
        x[o + j] += alpha[s] * pn;
        rv = r[o + j] - alpha[s] * sn;
        r[o + j] = rv;
      }
      double zv = 0.0;
#pragma unroll
      for (int cc = 0; cc < 7; ++cc) {
        const double rc = __shfl(rv, base + cc);
        if (act) zv += Minv[(size_t)s * bs.minv + (size_t)49 * row + 7 * rr + cc] * rc;
      }
      if (act) zout[o + j] = zv;
    }
  }
  if (commit) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if (!live[s]) continue;
      const double gamma = sc[s].tmp_rz;
      if (first) sc[s].rz0 = gamma;
      sc[s].rz[par ^ 1] = gamma;
      sc[s].gam_last = gamma;
      sc[s].alpha[par ^ 1] = alpha[s];
      const int itn = it + 1;
      sc[s].iter = itn;
      if (itn >= sc[s].max_iter) sc[s].stop = 1;
    }
  }
}
