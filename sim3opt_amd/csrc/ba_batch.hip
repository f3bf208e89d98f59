// ba_batch.hip -- the loop detector's two-view refinement (BAOptimize, kittiDetector.h:845-954, helpers :712-788,
// called once per accepted loop candidate at :1325) for a whole batch of candidates in ONE launch.
//
// One problem = two g2o::VertexSE3Expmap cameras, the first fixed (:861-870), n g2o::VertexSBAPointXYZ points
// (marginalised), two g2o::EdgeProjectXYZ2UV observations per point (:892-902), RobustKernelHuber, Levenberg-
// Marquardt with setUserLambdaInit(50) (:779-782) and setMaxTrialsAfterFailure(5) (:730).  It is the model of
// ba.hip in another configuration; what differs is the shape of the workload: many small independent problems
// whose reduced camera system is one 6x6 block.  ba.hip spends a dozen launches and a host synchronisation per LM
// trial of one problem; here a workgroup owns a problem and runs its whole LM loop, the damping rule included,
// without the host.
//
// k_ba_two_view: workgroup = problem, thread t owns the points t, t + 256, ... of its problem from the first pass to
// the last, so per-point data (the global scratch, the estimates) is only ever read by the thread that wrote it and
// needs no barrier.  What crosses threads are sums: a butterfly over the wavefront, then the four wavefronts'
// partials through LDS, added in a fixed order; every thread ends with the same bits, does the 6x6 Cholesky and
// the damping rule redundantly in registers, and so takes the same branches.  Nothing crosses workgroups; there are
// no atomics and no waits; every loop is bounded by max_iters x max_trials.  A problem's result depends on nothing
// but its own data: not on its position in the batch, nor on the batch.
//
//   per iteration   pass L: residuals, analytic Jacobians, Huber weights of both observations of a point ->
//                   H_pp (undamped), b_p, A_1, B_1, es_1 to the scratch; sums: robust chi2, sum A_1^T A_1, b_c
//   per trial       pass S: H_pp^-1 (damped), Z = (A_1^T B_1) H_pp^-1 -> scratch; sums: - sum Z (A_1^T B_1)^T, - sum Z b_p
//                   6x6 Cholesky of S = lambda I + sum A_1^T A_1 - sum Z Y^T, dx_c; exp-map update of camera 1
//                   pass U: dx_p = H_pp^-1 b_p - Z^T dx_c, trial points; sums: robust chi2 of the trial, x.(lambda x + b)
//                   LmDamping::update (lm_damping.hpp) accepts (the thread copies its trial points) or rejects
//   at the end      pass F: e->chi2() of every observation, activeChi2, the count above outlier_chi2 (:947-953)
//
// The passes are device functions (two_view_pass_L / _S / _U, two_view_reduced_solve, two_view_maxdiag), inlined into
// k_ba_two_view and into k_ba_two_view_trial, the read-out of ONE trial at a caller's lambda
// (sim3opt_ba_batch_debug_trial): what a test reads is what the LM loop runs.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "ba_math.hpp"
#include "handle_device.hpp"
#include "lm_damping.hpp"

namespace sim3opt_bundle {

constexpr int WGB = 256;                    // threads of a workgroup (four wavefronts)
constexpr int NWAVE = WGB / 64;
constexpr int SCR_PER_POINT = SIM3OPT_BA_BATCH_TRIAL_POINT_ROWS;  // doubles of scratch per point, see the S_* offsets
constexpr int STAT_DOUBLES = 5;             // chi2_before, chi2_after, lambda, rho, trials
constexpr int SUMMARY_DOUBLES = 5;          // iterations run, activeChi2 before / after, outlier edges, lambda_0
// scratch rows (row r of point g at scr[r * total + g]: consecutive threads, consecutive addresses)
constexpr int S_HPP = 0, S_BP = 6, S_A1 = 9, S_B1 = 21, S_ES1 = 27, S_HINV = 29, S_Z = 35, S_TRIAL = 53;
static_assert(S_TRIAL + 3 == SCR_PER_POINT && SCR_PER_POINT == 56, "scratch layout");
// the read-out's row of a problem (sim3opt.h, sim3opt_ba_batch_debug_trial)
constexpr int T_ATA = 0, T_BC = 21, T_CHI = 27, T_ACTIVE = 28, T_MAXDIAG = 29, T_ZY = 30, T_ZB = 51, T_S = 57, T_G = 78,
              T_DXC = 84, T_FAIL = 90, T_CAM = 91, T_CHI_NEW = 98, T_SCALE = 99;
constexpr int TRIAL_DOUBLES = SIM3OPT_BA_BATCH_TRIAL_PROBLEM_DOUBLES;
static_assert(T_SCALE + 1 == TRIAL_DOUBLES && TRIAL_DOUBLES == 100, "read-out layout");

struct TwoViewArgs {
  const int32_t* ptr;     // n_problems + 1
  const double* cam0;     // n x 7, fixed
  const double* cam1;     // n x 7, start
  const double* pts_in;   // total x 3
  const double* uv0;      // total x 2
  const double* uv1;
  double* scr;            // SCR_PER_POINT x total
  double* pts;            // total x 3: the estimate, then the result
  double* cam_out;        // n x 7
  double* stats;          // n x max_iters x STAT_DOUBLES
  double* summary;        // n x SUMMARY_DOUBLES
  double* edge_chi2;      // total x 2
  int64_t total;
  double f, cx, cy, omega, huber, tau, user_lambda_init, outlier_chi2;
  int32_t max_iters, max_trials;
};

// e, e2 = e^T Omega e, the Huber rho of one observation
__device__ __forceinline__ double two_view_rho(const TwoViewArgs& A, const double q[4], const double t[3],
                                               const double* p, const double* uv, double& e2) {
  double R[9], X[3], e[2], rho, w;
  ba_project_residual(q, t, p, uv[0], uv[1], A.f, A.cx, A.cy, R, X, e);
  e2 = A.omega * (e[0] * e[0] + e[1] * e[1]);
  ba_huber(e2, A.huber, rho, w);
  return rho;
}

// ---- pass L: linearise at the estimate A.pts, (c1q, c1t).  The thread's points are p0 + tid, p0 + tid + 256, ...
// below p0 + n.  acc, summed over the workgroup: 0..20 sum A1^T A1 (upper), 21..26 b_c, 27 robust chi2, 28 activeChi2;
// dmax: the largest diagonal entry of H_pp among THIS thread's points ----
__device__ __forceinline__ void two_view_pass_L(const TwoViewArgs& A, int tid, int64_t p0, int n, const double c0q[4],
                                                const double c0t[3], const double c1q[4], const double c1t[3],
                                                double (&acc)[29], double& dmax, double* red) {
  const int64_t T = A.total;
  double* const scr = A.scr;
  const double* const pts = A.pts;
#pragma unroll
  for (int q = 0; q < 29; ++q) acc[q] = 0.0;
  dmax = 0.0;
  for (int i = tid; i < n; i += WGB) {
    const int64_t g = p0 + i;
    const double p[3] = {pts[3 * g], pts[3 * g + 1], pts[3 * g + 2]};
    double R[9], X[3], e[2], rho, w, Jc[12], Jp[6];
    // camera 0 is fixed: its observation reaches H_pp and b_p only
    ba_project_residual(c0q, c0t, p, A.uv0[2 * g], A.uv0[2 * g + 1], A.f, A.cx, A.cy, R, X, e);
    double e2 = A.omega * (e[0] * e[0] + e[1] * e[1]);
    ba_huber(e2, A.huber, rho, w);
    acc[27] += rho;
    acc[28] += e2;
    double sw = sqrt(w * A.omega);
    ba_jacobians(R, X, A.f, Jc, Jp);
    double B[6], es[2] = {sw * e[0], sw * e[1]};
#pragma unroll
    for (int q = 0; q < 6; ++q) B[q] = sw * Jp[q];
    double H[6], b[3];
    H[0] = B[0] * B[0] + B[3] * B[3];
    H[1] = B[0] * B[1] + B[3] * B[4];
    H[2] = B[0] * B[2] + B[3] * B[5];
    H[3] = B[1] * B[1] + B[4] * B[4];
    H[4] = B[1] * B[2] + B[4] * B[5];
    H[5] = B[2] * B[2] + B[5] * B[5];
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = -(B[c] * es[0] + B[3 + c] * es[1]);
    // camera 1
    ba_project_residual(c1q, c1t, p, A.uv1[2 * g], A.uv1[2 * g + 1], A.f, A.cx, A.cy, R, X, e);
    e2 = A.omega * (e[0] * e[0] + e[1] * e[1]);
    ba_huber(e2, A.huber, rho, w);
    acc[27] += rho;
    acc[28] += e2;
    sw = sqrt(w * A.omega);
    ba_jacobians(R, X, A.f, Jc, Jp);
    double A1[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) A1[q] = sw * Jc[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) B[q] = sw * Jp[q];
    es[0] = sw * e[0];
    es[1] = sw * e[1];
    H[0] += B[0] * B[0] + B[3] * B[3];
    H[1] += B[0] * B[1] + B[3] * B[4];
    H[2] += B[0] * B[2] + B[3] * B[5];
    H[3] += B[1] * B[1] + B[4] * B[4];
    H[4] += B[1] * B[2] + B[4] * B[5];
    H[5] += B[2] * B[2] + B[5] * B[5];
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] -= B[c] * es[0] + B[3 + c] * es[1];
    dmax = fmax(dmax, fmax(H[0], fmax(H[3], H[5])));
#pragma unroll
    for (int q = 0; q < 6; ++q) scr[(S_HPP + q) * T + g] = H[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) scr[(S_BP + q) * T + g] = b[q];
#pragma unroll
    for (int q = 0; q < 12; ++q) scr[(S_A1 + q) * T + g] = A1[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) scr[(S_B1 + q) * T + g] = B[q];
    scr[(S_ES1 + 0) * T + g] = es[0];
    scr[(S_ES1 + 1) * T + g] = es[1];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int c = r; c < 6; ++c) acc[tri6(r, c)] += A1[r] * A1[c] + A1[6 + r] * A1[6 + c];
      acc[21 + r] -= A1[r] * es[0] + A1[6 + r] * es[1];
    }
  }
  wg_sum(acc, red);
}

// computeLambdaInit's maximum: the largest diagonal entry of the (undamped) Hessian over the free vertices
__device__ __forceinline__ double two_view_maxdiag(double dmax, const double (&acc)[29], double* red) {
  double maxdiag = wg_max(dmax, red);
#pragma unroll
  for (int r = 0; r < 6; ++r) maxdiag = fmax(maxdiag, acc[tri6(r, r)]);
  return maxdiag;
}

// ---- pass S: eliminate the points at damping lambda, sum the reduced camera system.  sg, summed over the
// workgroup: 0..20 - sum Z Y^T (upper), 21..26 - sum Z b_p ----
__device__ __forceinline__ void two_view_pass_S(const TwoViewArgs& A, int tid, int64_t p0, int n, double lambda,
                                                double (&sg)[27], double* red) {
  const int64_t T = A.total;
  double* const scr = A.scr;
#pragma unroll
  for (int q = 0; q < 27; ++q) sg[q] = 0.0;
  for (int i = tid; i < n; i += WGB) {
    const int64_t g = p0 + i;
    double H[6], b[3], A1[12], B[6], Hi[9];
#pragma unroll
    for (int q = 0; q < 6; ++q) H[q] = scr[(S_HPP + q) * T + g];
#pragma unroll
    for (int q = 0; q < 3; ++q) b[q] = scr[(S_BP + q) * T + g];
#pragma unroll
    for (int q = 0; q < 12; ++q) A1[q] = scr[(S_A1 + q) * T + g];
#pragma unroll
    for (int q = 0; q < 6; ++q) B[q] = scr[(S_B1 + q) * T + g];
    ba_sym3_inverse(H[0] + lambda, H[1], H[2], H[3] + lambda, H[4], H[5] + lambda, Hi);
    scr[(S_HINV + 0) * T + g] = Hi[0]; scr[(S_HINV + 1) * T + g] = Hi[1]; scr[(S_HINV + 2) * T + g] = Hi[2];
    scr[(S_HINV + 3) * T + g] = Hi[4]; scr[(S_HINV + 4) * T + g] = Hi[5]; scr[(S_HINV + 5) * T + g] = Hi[8];
    double Y[18], Z[18];  // Y = A1^T B1, Z = Y H_pp^-1, 6x3 row-major
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      Y[3 * r] = A1[r] * B[0] + A1[6 + r] * B[3];
      Y[3 * r + 1] = A1[r] * B[1] + A1[6 + r] * B[4];
      Y[3 * r + 2] = A1[r] * B[2] + A1[6 + r] * B[5];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Z[3 * r + c] = Y[3 * r] * Hi[c] + Y[3 * r + 1] * Hi[3 + c] + Y[3 * r + 2] * Hi[6 + c];
        scr[(S_Z + 3 * r + c) * T + g] = Z[3 * r + c];
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int c = r; c < 6; ++c)
        sg[tri6(r, c)] -= Z[3 * r] * Y[3 * c] + Z[3 * r + 1] * Y[3 * c + 1] + Z[3 * r + 2] * Y[3 * c + 2];
      sg[21 + r] -= Z[3 * r] * b[0] + Z[3 * r + 1] * b[1] + Z[3 * r + 2] * b[2];
    }
  }
  wg_sum(sg, red);
}

// S = lambda I + sum A_1^T A_1 - sum Z Y^T, g = b_c - sum Z b_p, dx_c = S^-1 g by the 6x6 Cholesky; returns `fail`:
// a non-positive pivot, the trial is rejected
__device__ __forceinline__ bool two_view_reduced_solve(const double (&acc)[29], const double (&sg)[27], double lambda,
                                                       double (&Su)[21], double (&gv)[6], double (&dxc)[6]) {
#pragma unroll
  for (int q = 0; q < 21; ++q) Su[q] = acc[q] + sg[q];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    Su[tri6(r, r)] += lambda;
    gv[r] = acc[21 + r] + sg[21 + r];
  }
  return !chol6_solve(Su, gv, dxc);
}

// ---- pass U: back-substitute the camera step dxc, the trial points to the scratch; the trial's robust chi2 with
// camera 1 at (nq, nt), and scale = x.(lambda x + b) over the points and the camera (b_c = acc[21..26]) ----
__device__ __forceinline__ void two_view_pass_U(const TwoViewArgs& A, int tid, int64_t p0, int n, double lambda,
                                                const double (&dxc)[6], const double (&acc)[29], const double c0q[4],
                                                const double c0t[3], const double nq[4], const double nt[3],
                                                double& tempChi, double& scale, double* red) {
  const int64_t T = A.total;
  double* const scr = A.scr;
  const double* const pts = A.pts;
  double tr[2] = {0.0, 0.0};
  for (int i = tid; i < n; i += WGB) {
    const int64_t g = p0 + i;
    double b[3], h[6], d[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) b[q] = scr[(S_BP + q) * T + g];
#pragma unroll
    for (int q = 0; q < 6; ++q) h[q] = scr[(S_HINV + q) * T + g];
    d[0] = h[0] * b[0] + h[1] * b[1] + h[2] * b[2];
    d[1] = h[1] * b[0] + h[3] * b[1] + h[4] * b[2];
    d[2] = h[2] * b[0] + h[4] * b[1] + h[5] * b[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) s += scr[(S_Z + 3 * r + c) * T + g] * dxc[r];
      d[c] -= s;
    }
    double pn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      tr[1] += d[c] * (lambda * d[c] + b[c]);
      pn[c] = pts[3 * g + c] + d[c];
      scr[(S_TRIAL + c) * T + g] = pn[c];
    }
    double e2;
    tr[0] += two_view_rho(A, c0q, c0t, pn, A.uv0 + 2 * g, e2);
    tr[0] += two_view_rho(A, nq, nt, pn, A.uv1 + 2 * g, e2);
  }
  wg_sum(tr, red);
  tempChi = tr[0];
  scale = tr[1];
#pragma unroll
  for (int r = 0; r < 6; ++r) scale += dxc[r] * (lambda * dxc[r] + acc[21 + r]);
}

__global__ __launch_bounds__(WGB) void k_ba_two_view(TwoViewArgs A) {
  __shared__ double red[NWAVE * 32];
  const int tid = threadIdx.x;
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const int64_t T = A.total;
  double* const scr = A.scr;
  double* const pts = A.pts;

  double c0q[4], c0t[3], c1q[4], c1t[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) { c0q[i] = A.cam0[7 * (size_t)prob + i]; c1q[i] = A.cam1[7 * (size_t)prob + i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) { c0t[i] = A.cam0[7 * (size_t)prob + 4 + i]; c1t[i] = A.cam1[7 * (size_t)prob + 4 + i]; }
  for (int i = tid; i < n; i += WGB) {
    const int64_t g = p0 + i;
#pragma unroll
    for (int c = 0; c < 3; ++c) pts[3 * g + c] = A.pts_in[3 * g + c];
  }

  sim3opt::LmDamping damp;
  bool go = true;
  int iters = 0;
  double active_before = 0.0, lambda0 = 0.0;
  for (int it = 0; it < A.max_iters && go; ++it) {
    double acc[29], dmax;
    two_view_pass_L(A, tid, p0, n, c0q, c0t, c1q, c1t, acc, dmax, red);
    double currentChi = acc[27];
    const double chi2_before = currentChi;
    if (it == 0) {
      active_before = acc[28];
      double maxdiag = 0.0;
      // computeLambdaInit: tau * max diagonal entry of the (undamped) Hessian over the free vertices
      if (!(A.user_lambda_init > 0)) maxdiag = two_view_maxdiag(dmax, acc, red);
      damp.start(A.user_lambda_init, A.tau, maxdiag);
      lambda0 = damp.lambda;
    }

    double rho = 0.0;
    int qmax = 0;
    do {
      const double lambda = damp.lambda;
      double sg[27], Su[21], gv[6], dxc[6];
      two_view_pass_S(A, tid, p0, n, lambda, sg, red);
      const bool fail = two_view_reduced_solve(acc, sg, lambda, Su, gv, dxc);

      double tempChi = DBL_MAX, scale = 0.0;
      double nq[4] = {c1q[0], c1q[1], c1q[2], c1q[3]}, nt[3] = {c1t[0], c1t[1], c1t[2]};
      if (!fail) {
        ba_se3_oplus(dxc, nq, nt);
        two_view_pass_U(A, tid, p0, n, lambda, dxc, acc, c0q, c0t, nq, nt, tempChi, scale, red);
      }
      if (damp.update(currentChi, tempChi, scale, 1.0 / 3.0, 2.0 / 3.0, rho)) {
        currentChi = tempChi;
#pragma unroll
        for (int i = 0; i < 4; ++i) c1q[i] = nq[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) c1t[i] = nt[i];
        // A failed trial skipped pass U and has no trial points: the estimate stays.  (The rule does accept one when
        // the current chi2 is not finite, DBL_MAX being less than +inf; the rows would be whatever the scratch held.)
        for (int i = tid; i < n && !fail; i += WGB) {
          const int64_t g = p0 + i;
#pragma unroll
          for (int c = 0; c < 3; ++c) pts[3 * g + c] = scr[(S_TRIAL + c) * T + g];
        }
      }
      ++qmax;
    } while (rho < 0 && qmax < A.max_trials);

    if (tid == 0) {
      double* s = A.stats + ((size_t)prob * A.max_iters + it) * STAT_DOUBLES;
      s[0] = chi2_before; s[1] = currentChi; s[2] = damp.lambda; s[3] = rho; s[4] = (double)qmax;
    }
    ++iters;
    if (damp.terminate(qmax, A.max_trials, rho)) go = false;
  }

  // ---- pass F: e->chi2() of every observation at the final estimate ----
  double fin[2] = {0.0, 0.0};  // activeChi2, observations above outlier_chi2
  for (int i = tid; i < n; i += WGB) {
    const int64_t g = p0 + i;
    const double p[3] = {pts[3 * g], pts[3 * g + 1], pts[3 * g + 2]};
    double e0, e1;
    two_view_rho(A, c0q, c0t, p, A.uv0 + 2 * g, e0);
    two_view_rho(A, c1q, c1t, p, A.uv1 + 2 * g, e1);
    A.edge_chi2[2 * g] = e0;
    A.edge_chi2[2 * g + 1] = e1;
    fin[0] += e0;
    fin[0] += e1;
    fin[1] += (e0 > A.outlier_chi2 ? 1.0 : 0.0) + (e1 > A.outlier_chi2 ? 1.0 : 0.0);
  }
  wg_sum(fin, red);
  if (tid == 0) {
    double* s = A.summary + (size_t)prob * SUMMARY_DOUBLES;
    s[0] = (double)iters; s[1] = active_before; s[2] = fin[0]; s[3] = fin[1]; s[4] = lambda0;
    double* c = A.cam_out + 7 * (size_t)prob;
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = c1q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[4 + i] = c1t[i];
  }
}

// The read-out of one trial (sim3opt_ba_batch_debug_trial): passes L, S, the Cholesky and U of k_ba_two_view, once,
// at the estimate A.pts (read only) and A.cam1, at the caller's lam[problem]; pass U with the caller's camera step
// when dx_c is given.  The scratch is the per-point half of the read-out, `out` the per-problem half (T_* offsets).
// Of A it reads ptr, cam0, cam1, pts, uv0, uv1, scr, total and the camera / kernel constants.
__global__ __launch_bounds__(WGB) void k_ba_two_view_trial(TwoViewArgs A, const double* lam, const double* dx_c,
                                                           double* out) {
  __shared__ double red[NWAVE * 32];
  const int tid = threadIdx.x;
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);

  double c0q[4], c0t[3], c1q[4], c1t[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) { c0q[i] = A.cam0[7 * (size_t)prob + i]; c1q[i] = A.cam1[7 * (size_t)prob + i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) { c0t[i] = A.cam0[7 * (size_t)prob + 4 + i]; c1t[i] = A.cam1[7 * (size_t)prob + 4 + i]; }

  double acc[29], dmax;
  two_view_pass_L(A, tid, p0, n, c0q, c0t, c1q, c1t, acc, dmax, red);
  const double maxdiag = two_view_maxdiag(dmax, acc, red);
  const double lambda = lam[prob];
  double sg[27], Su[21], gv[6], dxc[6], step[6];
  two_view_pass_S(A, tid, p0, n, lambda, sg, red);
  const bool fail = two_view_reduced_solve(acc, sg, lambda, Su, gv, dxc);
#pragma unroll
  for (int r = 0; r < 6; ++r) step[r] = dx_c ? dx_c[6 * (size_t)prob + r] : dxc[r];
  double tempChi = DBL_MAX, scale = 0.0;
  double nq[4] = {c1q[0], c1q[1], c1q[2], c1q[3]}, nt[3] = {c1t[0], c1t[1], c1t[2]};
  if (!fail) {
    ba_se3_oplus(step, nq, nt);
    two_view_pass_U(A, tid, p0, n, lambda, step, acc, c0q, c0t, nq, nt, tempChi, scale, red);
  }
  if (tid == 0) {
    double* o = out + (size_t)prob * TRIAL_DOUBLES;
#pragma unroll
    for (int q = 0; q < 21; ++q) { o[T_ATA + q] = acc[q]; o[T_ZY + q] = sg[q]; o[T_S + q] = Su[q]; }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      o[T_BC + r] = acc[21 + r]; o[T_ZB + r] = sg[21 + r]; o[T_G + r] = gv[r]; o[T_DXC + r] = dxc[r];
    }
    o[T_CHI] = acc[27]; o[T_ACTIVE] = acc[28]; o[T_MAXDIAG] = maxdiag;
    o[T_FAIL] = fail ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[T_CAM + i] = nq[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[T_CAM + 4 + i] = nt[i];
    o[T_CHI_NEW] = tempChi; o[T_SCALE] = scale;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Batch : sim3opt::BatchHandle {
  sim3opt_ba_batch_options opt;
  // the problems, as set; cam1 and pts hold the current estimate
  std::vector<int32_t> ptr;
  std::vector<double> cam0_given, cam0, cam1, pts, uv0, uv1;
  double f = 0, cx = 0, cy = 0;
  // the last run
  std::vector<double> stats, summary, edge_chi2;
  int32_t stats_stride = 0;  // max_iters of the last run
  // device
  sim3opt::DevArena mem;  // the four blocks of dev
  struct Dev {
    int32_t* ptr;
    double *in, *scr, *out;
    int64_t cap_n, cap_total, cap_iters;  // what the blocks were sized for
    bool static_uploaded;
  } dev{};

  ~Batch() { release(); }
  int32_t n() const { return ptr.empty() ? 0 : (int32_t)ptr.size() - 1; }
  int64_t total() const { return ptr.empty() ? 0 : ptr.back(); }

  void release() {
    close_stream(mem);
    dev = Dev{};
  }

  size_t in_doubles() const { return 14 * (size_t)n() + 7 * (size_t)total(); }
  size_t out_doubles() const {
    return (7 + SUMMARY_DOUBLES + (size_t)STAT_DOUBLES * opt.max_iters) * n() + 5 * (size_t)total();
  }

  // the camera and kernel constants of a launch
  void constants(TwoViewArgs& A) const {
    A.total = total();
    A.f = f; A.cx = cx; A.cy = cy;
    A.omega = 1.0 / (opt.pixel_noise * opt.pixel_noise);
    A.huber = opt.huber_delta; A.tau = opt.tau; A.user_lambda_init = opt.user_lambda_init;
    A.outlier_chi2 = opt.outlier_chi2;
    A.max_iters = opt.max_iters; A.max_trials = opt.max_trials;
  }

  int optimize() {
    err.clear();
    if (n() < 1) { err = "ba_batch_optimize: no problems set"; return SIM3OPT_ERR_STATE; }
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    const int32_t N = n();
    const size_t T = (size_t)total();
    if (N != dev.cap_n || (int64_t)T != dev.cap_total || opt.max_iters != dev.cap_iters) {
      release();
      if (int rc = open_stream()) return rc;
      HIPCHK(mem.raw(dev.ptr, (size_t)N + 1));
      HIPCHK(mem.raw(dev.in, in_doubles()));
      HIPCHK(mem.raw(dev.scr, SCR_PER_POINT * T));
      HIPCHK(mem.raw(dev.out, out_doubles()));
      dev.cap_n = N; dev.cap_total = (int64_t)T; dev.cap_iters = opt.max_iters;
    }
    // device layout of dev.in: cam0 | cam1 | points | uv0 | uv1; of dev.out: points | cam1 | stats | summary | edge chi2
    double* d_cam0 = dev.in;
    double* d_cam1 = d_cam0 + 7 * (size_t)N;
    double* d_pin = d_cam1 + 7 * (size_t)N;
    double* d_uv0 = d_pin + 3 * T;
    double* d_uv1 = d_uv0 + 2 * T;
    if (!dev.static_uploaded) {
      HIPCHK(hipMemcpyAsync(dev.ptr, ptr.data(), sizeof(int32_t) * ((size_t)N + 1), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_cam0, cam0.data(), sizeof(double) * 7 * N, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_uv0, uv0.data(), sizeof(double) * 2 * T, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_uv1, uv1.data(), sizeof(double) * 2 * T, hipMemcpyHostToDevice, stream));
    }
    HIPCHK(hipMemcpyAsync(d_cam1, cam1.data(), sizeof(double) * 7 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_pin, pts.data(), sizeof(double) * 3 * T, hipMemcpyHostToDevice, stream));
    // (the copies read pageable memory: each has left the host buffer when its call returns)
    dev.static_uploaded = true;

    TwoViewArgs A;
    A.ptr = dev.ptr; A.cam0 = d_cam0; A.cam1 = d_cam1; A.pts_in = d_pin; A.uv0 = d_uv0; A.uv1 = d_uv1;
    A.scr = dev.scr;
    A.pts = dev.out;
    A.cam_out = A.pts + 3 * T;
    A.stats = A.cam_out + 7 * (size_t)N;
    A.summary = A.stats + (size_t)STAT_DOUBLES * opt.max_iters * N;
    A.edge_chi2 = A.summary + (size_t)SUMMARY_DOUBLES * N;
    constants(A);
    // the statistics of iterations a problem does not reach read as zeros
    HIPCHK(hipMemsetAsync(A.stats, 0, sizeof(double) * STAT_DOUBLES * opt.max_iters * N, stream));
    hipLaunchKernelGGL(k_ba_two_view, dim3(N), dim3(WGB), 0, stream, A);  // the one launch of the batch
    HIPCHK(hipGetLastError());
    std::vector<double> out;
    HIPCHK(sim3opt::read_back(out, dev.out, out_doubles(), stream));
    HIPCHK(hipStreamSynchronize(stream));
    const double* o = out.data();
    pts.assign(o, o + 3 * T); o += 3 * T;
    cam1.assign(o, o + 7 * (size_t)N); o += 7 * (size_t)N;
    stats.assign(o, o + (size_t)STAT_DOUBLES * opt.max_iters * N); o += (size_t)STAT_DOUBLES * opt.max_iters * N;
    summary.assign(o, o + (size_t)SUMMARY_DOUBLES * N); o += (size_t)SUMMARY_DOUBLES * N;
    edge_chi2.assign(o, o + 2 * T);
    stats_stride = opt.max_iters;
    have_run = true;
    return N;
  }

  // sim3opt_ba_batch_debug_trial: one trial of every problem at the current estimate, in blocks of its own that are
  // gone when it returns.  Nothing of the handle is written: not the estimate, not the last run, not `dev`.
  int debug_trial(const double* lam, const double* dx_c, double* point_rows, double* problem_rows) {
    err.clear();
    if (n() < 1) { err = "ba_batch_debug_trial: no problems set"; return SIM3OPT_ERR_STATE; }
    const size_t N = (size_t)n(), T = (size_t)total();
    if (!sim3opt::all_finite(lam, N)) { err = "ba_batch_debug_trial: non-finite lambda"; return SIM3OPT_ERR_ARG; }
    if (dx_c && !sim3opt::all_finite(dx_c, 6 * N)) {
      err = "ba_batch_debug_trial: non-finite camera step";
      return SIM3OPT_ERR_ARG;
    }
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    // d_in: cam0 | cam1 | points | uv0 | uv1 | lam | dx_c.  (Declared before the stream's lease: on every path the
    // lease's synchronisation comes first, then the blocks go.)
    sim3opt::DevBuf<int32_t> d_ptr;
    sim3opt::DevBuf<double> d_in, d_scr, d_out;
    hipStream_t s = nullptr;  // (the handle's own may not exist yet, and is not this call's to create)
    HIPCHK(sim3opt::stream_acquire(&s));
    struct Lease {
      hipStream_t s;
      ~Lease() { (void)hipStreamSynchronize(s); sim3opt::stream_release(s); }
    } lease{s};
    HIPCHK(d_ptr.alloc(N + 1));
    HIPCHK(d_in.alloc(in_doubles() + 7 * N));
    HIPCHK(d_scr.alloc(SCR_PER_POINT * T));
    HIPCHK(d_out.alloc(TRIAL_DOUBLES * N));
    double* d_cam0 = d_in.get();
    double* d_cam1 = d_cam0 + 7 * N;
    double* d_pts = d_cam1 + 7 * N;
    double* d_uv0 = d_pts + 3 * T;
    double* d_uv1 = d_uv0 + 2 * T;
    double* d_lam = d_uv1 + 2 * T;
    double* d_dxc = d_lam + N;
    HIPCHK(hipMemcpyAsync(d_ptr.get(), ptr.data(), sizeof(int32_t) * (N + 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_cam0, cam0.data(), sizeof(double) * 7 * N, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_cam1, cam1.data(), sizeof(double) * 7 * N, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_pts, pts.data(), sizeof(double) * 3 * T, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_uv0, uv0.data(), sizeof(double) * 2 * T, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_uv1, uv1.data(), sizeof(double) * 2 * T, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_lam, lam, sizeof(double) * N, hipMemcpyHostToDevice, s));
    if (dx_c) HIPCHK(hipMemcpyAsync(d_dxc, dx_c, sizeof(double) * 6 * N, hipMemcpyHostToDevice, s));
    // a failed trial skips pass U: its trial rows read as zeros
    HIPCHK(hipMemsetAsync(d_scr.get(), 0, sizeof(double) * SCR_PER_POINT * T, s));
    TwoViewArgs A{};
    A.ptr = d_ptr.get(); A.cam0 = d_cam0; A.cam1 = d_cam1; A.pts_in = d_pts; A.uv0 = d_uv0; A.uv1 = d_uv1;
    A.scr = d_scr.get();
    A.pts = d_pts;
    constants(A);
    hipLaunchKernelGGL(k_ba_two_view_trial, dim3((unsigned)N), dim3(WGB), 0, s, A, (const double*)d_lam,
                       dx_c ? (const double*)d_dxc : (const double*)nullptr, d_out.get());
    HIPCHK(hipGetLastError());
    std::vector<double> h_scr, h_out;
    if (point_rows) HIPCHK(sim3opt::read_back(h_scr, (const double*)d_scr.get(), SCR_PER_POINT * T, s));
    if (problem_rows) HIPCHK(sim3opt::read_back(h_out, (const double*)d_out.get(), TRIAL_DOUBLES * N, s));
    HIPCHK(hipStreamSynchronize(s));
    if (point_rows) std::memcpy(point_rows, h_scr.data(), sizeof(double) * h_scr.size());
    if (problem_rows) std::memcpy(problem_rows, h_out.data(), sizeof(double) * h_out.size());
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_bundle

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched two-view bundle adjustment")
// ------------------------------------------------------------------------------------------
struct sim3opt_ba_batch : sim3opt_bundle::Batch {};

extern "C" {

void sim3opt_ba_batch_options_default(sim3opt_ba_batch_options* o) {
  if (!o) return;
  o->huber_delta = 3.0;        // OptParams(10, true, 3), kittiDetector.h:1325
  o->pixel_noise = 1.0;        // information = weight * I, weight = 1, :758-764
  o->tau = 1e-5;
  o->user_lambda_init = 50.0;  // :779-782
  o->outlier_chi2 = 5.995;     // :847
  o->max_iters = 10;           // :1325
  o->max_trials = 5;           // :730
  o->device = -1;
}

sim3opt_ba_batch* sim3opt_ba_batch_create(void) {
  return sim3opt::handle_create<sim3opt_ba_batch>(sim3opt_ba_batch_options_default);
}

void sim3opt_ba_batch_destroy(sim3opt_ba_batch* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_ba_batch_last_error(const sim3opt_ba_batch* b) { return b ? b->err.c_str() : "null batch"; }

int sim3opt_ba_batch_set_options(sim3opt_ba_batch* b, const sim3opt_ba_batch_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  if (o->max_iters < 1 || o->max_trials < 1 || !(o->pixel_noise > 0) || !std::isfinite(o->pixel_noise) ||
      !(o->tau > 0) || !std::isfinite(o->tau) || !(o->huber_delta >= 0) || !std::isfinite(o->huber_delta) ||
      !std::isfinite(o->user_lambda_init) || !std::isfinite(o->outlier_chi2)) {
    b->err = "ba_batch_set_options: value out of range";
    return SIM3OPT_ERR_ARG;
  }
  if (o->device != b->opt.device) b->release();  // the device is chosen at the next optimize
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_ba_batch_set_problems(sim3opt_ba_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                  const double* cam0, const double* cam1, const double* points, const double* uv0,
                                  const double* uv1, double focal, double cx, double cy) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (n_problems < 1 || !point_ptr || !cam0 || !cam1 || !points || !uv0 || !uv1 || !(focal > 0) ||
      !std::isfinite(focal) || !std::isfinite(cx) || !std::isfinite(cy)) {
    b->err = "ba_batch_set_problems: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "ba_batch_set_problems", sim3opt::NO_MEMORY, [&]() -> int {
  using sim3opt::all_finite;
  const std::string e = sim3opt::check_point_ptr(n_problems, point_ptr);
  if (!e.empty()) { b->err = "ba_batch_set_problems: " + e; return SIM3OPT_ERR_ARG; }
  const size_t T = (size_t)point_ptr[n_problems];
  if (!all_finite(cam0, 7 * (size_t)n_problems) || !all_finite(cam1, 7 * (size_t)n_problems)) {
    b->err = "ba_batch_set_problems: non-finite camera";
    return SIM3OPT_ERR_ARG;
  }
  if (!all_finite(points, 3 * T)) { b->err = "ba_batch_set_problems: non-finite point"; return SIM3OPT_ERR_ARG; }
  if (!all_finite(uv0, 2 * T) || !all_finite(uv1, 2 * T)) {
    b->err = "ba_batch_set_problems: non-finite observation";
    return SIM3OPT_ERR_ARG;
  }
  // unit quaternions, as sim3opt_ba_set_problem makes them
  std::vector<double> c0(cam0, cam0 + 7 * (size_t)n_problems), c1(cam1, cam1 + 7 * (size_t)n_problems);
  for (std::vector<double>* c : {&c0, &c1})
    for (int32_t k = 0; k < n_problems; ++k) {
      double* s = c->data() + 7 * (size_t)k;
      const double nq = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3]);
      if (!(nq > 0) || !std::isfinite(nq)) { b->err = "ba_batch_set_problems: zero quaternion"; return SIM3OPT_ERR_ARG; }
      for (int i = 0; i < 4; ++i) s[i] /= nq;
    }
  std::vector<int32_t> ptr(point_ptr, point_ptr + n_problems + 1);
  std::vector<double> given(cam0, cam0 + 7 * (size_t)n_problems), p(points, points + 3 * T), a(uv0, uv0 + 2 * T),
      c(uv1, uv1 + 2 * T);
  // nothing failed: the handle changes now
  b->ptr.swap(ptr);
  b->cam0_given.swap(given); b->cam0.swap(c0); b->cam1.swap(c1);
  b->pts.swap(p); b->uv0.swap(a); b->uv1.swap(c);
  b->f = focal; b->cx = cx; b->cy = cy;
  b->stats.clear(); b->summary.clear(); b->edge_chi2.clear();
  b->have_run = false;
  b->dev.static_uploaded = false;
  return SIM3OPT_OK;
  });
}

int sim3opt_ba_batch_dims(const sim3opt_ba_batch* b, int32_t* n_problems, int32_t* total_points) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (n_problems) *n_problems = b->n();
  if (total_points) *total_points = (int32_t)b->total();
  return SIM3OPT_OK;
}

int sim3opt_ba_batch_optimize(sim3opt_ba_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_batch_optimize", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->optimize(); });
}

int sim3opt_ba_batch_debug_trial(sim3opt_ba_batch* b, const double* lambda, const double* dx_c, double* point_rows,
                                 double* problem_rows) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!lambda || (!point_rows && !problem_rows)) {
    b->err = "ba_batch_debug_trial: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "ba_batch_debug_trial", sim3opt::NO_MEMORY_OR_INTERNAL,
                          [&] { return b->debug_trial(lambda, dx_c, point_rows, problem_rows); });
}

int sim3opt_ba_batch_get_cameras(const sim3opt_ba_batch* b, double* cam0, double* cam1) {
  if (!b || (!cam0 && !cam1)) return SIM3OPT_ERR_ARG;
  if (cam0 && !b->cam0_given.empty()) std::memcpy(cam0, b->cam0_given.data(), sizeof(double) * b->cam0_given.size());
  if (cam1 && !b->cam1.empty()) std::memcpy(cam1, b->cam1.data(), sizeof(double) * b->cam1.size());
  return SIM3OPT_OK;
}

int sim3opt_ba_batch_get_points(const sim3opt_ba_batch* b, double* points) {
  if (!b || !points) return SIM3OPT_ERR_ARG;
  if (!b->pts.empty()) std::memcpy(points, b->pts.data(), sizeof(double) * b->pts.size());
  return SIM3OPT_OK;
}

int32_t sim3opt_ba_batch_num_iterations(const sim3opt_ba_batch* b, int32_t problem) {
  if (!b || !b->have_run || problem < 0 || problem >= b->n()) return 0;
  return (int32_t)b->summary[(size_t)sim3opt_bundle::SUMMARY_DOUBLES * problem];
}

int sim3opt_ba_batch_get_stats(const sim3opt_ba_batch* b, int32_t problem, int32_t iter, sim3opt_iter_stats* out) {
  if (!b || !out || iter < 0 || iter >= sim3opt_ba_batch_num_iterations(b, problem)) return SIM3OPT_ERR_ARG;
  const double* s = b->stats.data() + ((size_t)problem * b->stats_stride + iter) * sim3opt_bundle::STAT_DOUBLES;
  sim3opt_iter_stats T{};
  T.chi2_before = s[0]; T.chi2_after = s[1]; T.lambda = s[2]; T.rho = s[3]; T.trials = (int32_t)s[4];
  *out = T;
  return SIM3OPT_OK;
}

int sim3opt_ba_batch_get_lambda_init(const sim3opt_ba_batch* b, double* lambda_init) {
  if (!b || !lambda_init) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k) lambda_init[k] = b->summary[(size_t)sim3opt_bundle::SUMMARY_DOUBLES * k + 4];
  return SIM3OPT_OK;
}

int sim3opt_ba_batch_get_chi2(const sim3opt_ba_batch* b, double* active_before, double* active_after,
                              double* edge_chi2, int32_t* n_outlier_edges) {
  if (!b || (!active_before && !active_after && !edge_chi2 && !n_outlier_edges)) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k) {
    const double* s = b->summary.data() + (size_t)sim3opt_bundle::SUMMARY_DOUBLES * k;
    if (active_before) active_before[k] = s[1];
    if (active_after) active_after[k] = s[2];
    if (n_outlier_edges) n_outlier_edges[k] = (int32_t)s[3];
  }
  if (edge_chi2) std::memcpy(edge_chi2, b->edge_chi2.data(), sizeof(double) * b->edge_chi2.size());
  return SIM3OPT_OK;
}

}  // extern "C"
