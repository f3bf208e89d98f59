// pnp_batch.hip -- the loop detector's start pose (cv::solvePnPRansac, kittiDetector.h:1300-1301: camera 1 from
// camera 0's 3-D points and camera 1's pixels, 100 hypotheses, 3 px, called once per accepted loop candidate) for a
// whole batch of candidates in ONE launch.  Its result is the cam1 start sim3opt_ba_batch_set_problems asks for.
//
// PARITY UNPINNED: loopConstraints.txt stores what the reference's PnP runs returned, not what they were given, and
// OpenCV's sampling is not reproducible.  This is not OpenCV's algorithm restated: hypotheses come from a
// closed-form P3P on three points, disambiguated by a fourth (OpenCV: EPnP on its minimal sets), every one of
// `iterations` hypotheses is evaluated (OpenCV leaves early on its confidence estimate), the sampler is counter
// based and reproducible, and the final refit is a Levenberg-Marquardt of the project's own (OpenCV: CV_ITERATIVE).
// What is OpenCV's: the inlier criterion (squared reprojection error <= reproj_error^2) and the order of the steps.
// tests/pnp_ref.py restates the whole pipeline independently (another P3P); planted truth checks both.
//
// k_pnp_ransac: workgroup = problem, 256 threads, as ba_batch.hip.  Nothing crosses workgroups, there are no atomics
// and no waits on other workgroups; every loop is bounded by the options; a problem's result depends on its own data
// and the options only.
//   hypotheses   in chunks of 256: thread t makes hypothesis base + t (pnp_math.hpp) and leaves its pose in LDS
//   scoring,     ransac_frame.hpp (score_chunk, best_of_waves) with PnpScore: the squared reprojection error of the
//   best         points in front of the camera, staged in LDS when the problem has at most LDS_POINTS of them
//   refit        LM on camera 1 over the best hypothesis's inliers: thread t owns the points t, t + 256, ...; sums by
//                wg_sum, 6x6 Cholesky and the damping rule (lm_damping.hpp) redundantly per thread, as ba_batch.hip
//   final count  inlier mask, count and RMS at the refitted pose
// One launch per batch: no step needs anything from another problem, so there is no reason for a second.
// k_ransac_score<PnpScore> and k_pnp_refine run the same scoring and refit code on supplied poses
// (sim3opt_pnp_batch_debug_*).  The handle is the frame's RansacBatch; this file adds args() and the refit's debug
// entry.
#include <hip/hip_runtime.h>

#include <algorithm>
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
#include "pnp_math.hpp"
#include "ransac_frame.hpp"

namespace sim3opt_pnp {

using sim3opt_bundle::ba_jacobians;
using sim3opt_bundle::ba_project_residual;
using sim3opt_bundle::ba_se3_oplus;
using sim3opt_bundle::chol6_solve;
using sim3opt_bundle::R_to_quat;
using sim3opt_bundle::tri6;
using sim3opt_bundle::wg_sum;
using sim3opt_ransac::NWAVE;
using sim3opt_ransac::WG;

// Points of a problem staged in LDS for the scoring: 5 doubles each, 45 KiB at the cap; with the chunk's poses
// (14 KiB) and the reduction slots the workgroup stays below the 64 KiB a workgroup may declare statically, so two
// workgroups share a CU's 160 KiB.  KITTI-00's candidates have 219-1047 points: all of them are staged.
constexpr int LDS_POINTS = 1152;
constexpr double REFIT_GAIN_TOL = 1e-9;  // the refit has converged when a step promises less of chi2 than this
constexpr int HYP_INTS = 7;         // per hypothesis: sample (4), solutions, valid, inlier count
constexpr int OUT_DOUBLES = 9;      // per problem: pose (7), cost of the best hypothesis, RMS of the final inliers
constexpr int OUT_INTS = 5;         // status, best hypothesis, its inlier count, final inlier count, refit iterations

struct PnpArgs {
  const int32_t* ptr;   // n_problems + 1
  const double* pts;    // total x 3
  const double* uv;     // total x 2
  double* hyp_pose;     // n x H x 7
  double* hyp_cost;     // n x H
  int32_t* hyp_int;     // n x H x HYP_INTS
  double* out_d;        // n x OUT_DOUBLES
  int32_t* out_i;       // n x OUT_INTS
  uint8_t* mask;        // total
  double f, cx, cy, thr2, tau;
  uint64_t seed;
  int32_t H, min_points, min_inliers, refine_iters, max_trials;
};

struct PtsGlobal {  // the points of a problem where the caller's arrays lie
  const double* p;
  const double* uv;
  __device__ __forceinline__ void get(int i, double X[3], double& u, double& v) const {
    X[0] = p[3 * (size_t)i]; X[1] = p[3 * (size_t)i + 1]; X[2] = p[3 * (size_t)i + 2];
    u = uv[2 * (size_t)i]; v = uv[2 * (size_t)i + 1];
  }
};

struct PtsLds {  // ... and staged: five rows of LDS_POINTS (consecutive lanes, consecutive addresses)
  const double* s;
  __device__ __forceinline__ void get(int i, double X[3], double& u, double& v) const {
    X[0] = s[i]; X[1] = s[LDS_POINTS + i]; X[2] = s[2 * LDS_POINTS + i];
    u = s[3 * LDS_POINTS + i]; v = s[4 * LDS_POINTS + i];
  }
};

__device__ __forceinline__ void stage_points(const PtsGlobal& G, int n, double* s) {
  const double* const p = G.p;
  const double* const uv = G.uv;
  for (int i = threadIdx.x; i < n; i += WG) {
    s[i] = p[3 * (size_t)i]; s[LDS_POINTS + i] = p[3 * (size_t)i + 1]; s[2 * LDS_POINTS + i] = p[3 * (size_t)i + 2];
    s[3 * LDS_POINTS + i] = uv[2 * (size_t)i]; s[4 * LDS_POINTS + i] = uv[2 * (size_t)i + 1];
  }
}

// point i counts for the pose iff it lies in front of the camera and its squared error is within thr2
__device__ __forceinline__ bool pnp_inlier(const double R[9], const double t[3], const double X[3], double u, double v,
                                           double f, double cx, double cy, double thr2, double& e2) {
  double z;
  e2 = pnp_sqerr(R, t, X, u, v, f, cx, cy, z);
  return z > 0.0 && e2 <= thr2;
}

struct PnpScore {  // the frame's scoring policy: a pose [q t] counts the points pnp_inlier admits
  static constexpr int DOUBLES = 7, CHUNK = WG, LDS_POINTS = sim3opt_pnp::LDS_POINTS, POINT_DOUBLES = 5;
  using Args = PnpArgs;
  using Lds = PtsLds;
  struct Prepared { double R[9], t[3]; };
  const PnpArgs& A;
  static __device__ __forceinline__ PtsGlobal global(const PnpArgs& A, int64_t p0) {
    return PtsGlobal{A.pts + 3 * p0, A.uv + 2 * p0};
  }
  static __device__ __forceinline__ void stage(const PtsGlobal& G, int n, double* s) { stage_points(G, n, s); }
  __device__ __forceinline__ void prepare(const double* pose, Prepared& p) const {
    const double q[4] = {pose[0], pose[1], pose[2], pose[3]};
    pnp_quat_to_R(q, p.R);
    p.t[0] = pose[4]; p.t[1] = pose[5]; p.t[2] = pose[6];
  }
  template <class Pts>
  __device__ __forceinline__ bool inlier(const Prepared& p, const Pts& P, int i, double& e2) const {
    double X[3], u, v;
    P.get(i, X, u, v);
    return pnp_inlier(p.R, p.t, X, u, v, A.f, A.cx, A.cy, A.thr2, e2);
  }
};

// The inliers of (q, t) among the points a thread owns -> mask; count and sum of squared errors over the workgroup
__device__ __forceinline__ void mark_inliers(const PnpArgs& A, int64_t p0, int n, const double q[4], const double t[3],
                                             uint8_t* mask, double* red, int& count, double& cost) {
  double R[9];
  pnp_quat_to_R(q, R);
  double acc[2] = {0.0, 0.0};  // (the count is an integer below 2^31: a double carries it exactly)
  for (int i = threadIdx.x; i < n; i += WG) {
    const int64_t g = p0 + i;
    const double X[3] = {A.pts[3 * g], A.pts[3 * g + 1], A.pts[3 * g + 2]};
    double e2;
    const bool in = pnp_inlier(R, t, X, A.uv[2 * g], A.uv[2 * g + 1], A.f, A.cx, A.cy, A.thr2, e2);
    mask[g] = in ? 1 : 0;
    if (in) { acc[0] += 1.0; acc[1] += e2; }
  }
  wg_sum(acc, red);
  count = (int)acc[0];
  cost = acc[1];
}

// sum of squared errors of the masked points under (q, t)
__device__ __forceinline__ double masked_chi2(const PnpArgs& A, int64_t p0, int n, const uint8_t* mask,
                                              const double q[4], const double t[3], double* red) {
  double acc[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += WG) {
    const int64_t g = p0 + i;
    if (!mask[g]) continue;
    double R[9], X[3], e[2];
    ba_project_residual(q, t, A.pts + 3 * g, A.uv[2 * g], A.uv[2 * g + 1], A.f, A.cx, A.cy, R, X, e);
    acc[0] += e[0] * e[0] + e[1] * e[1];
  }
  wg_sum(acc, red);
  return acc[0];
}

// The refit: LM on the six degrees of freedom of (q, t) over the masked points (fixed, information I, no robust
// kernel), lambda_0 = tau max diag(H), at most refine_iters iterations of at most max_trials trials.  It also ends
// when a step promises nothing: its predicted decrease of chi2, x.(lambda x + b), is at most REFIT_GAIN_TOL of chi2.
// With lambda_0 this small the LM converges in three or four iterations; whether the steps after that are accepted
// is decided by rounding, so they are not taken.  Thread t reads the mask entries of the points it owns only.
// trials (refine_iters entries, or NULL) gets the trial count of every iteration run.
__device__ __forceinline__ void pnp_refit(const PnpArgs& A, int64_t p0, int n, const uint8_t* mask, double q[4],
                                          double t[3], double* red, int32_t* trials, int& iters, double& chi_before,
                                          double& chi_after) {
  sim3opt::LmDamping damp;
  bool go = true;
  iters = 0;
  double currentChi = 0.0;
  for (int it = 0; it < A.refine_iters && go; ++it) {
    double acc[28];  // 0..20 sum J^T J (upper), 21..26 b = - sum J^T e, 27 chi2
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += WG) {
      const int64_t g = p0 + i;
      if (!mask[g]) continue;
      double R[9], X[3], e[2], Jc[12], Jp[6];
      ba_project_residual(q, t, A.pts + 3 * g, A.uv[2 * g], A.uv[2 * g + 1], A.f, A.cx, A.cy, R, X, e);
      ba_jacobians(R, X, A.f, Jc, Jp);
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = r; c < 6; ++c) acc[tri6(r, c)] += Jc[r] * Jc[c] + Jc[6 + r] * Jc[6 + c];
        acc[21 + r] -= Jc[r] * e[0] + Jc[6 + r] * e[1];
      }
      acc[27] += e[0] * e[0] + e[1] * e[1];
    }
    wg_sum(acc, red);
    currentChi = acc[27];
    if (it == 0) {
      chi_before = currentChi;
      double maxdiag = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) maxdiag = fmax(maxdiag, acc[tri6(r, r)]);
      damp.start(0.0, A.tau, maxdiag);
    }
    double rho = 0.0;
    int qmax = 0;
    bool converged = false;
    do {
      const double lambda = damp.lambda;
      double Su[21], gv[6], dx[6];
#pragma unroll
      for (int k = 0; k < 21; ++k) Su[k] = acc[k];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        Su[tri6(r, r)] += lambda;
        gv[r] = acc[21 + r];
      }
      const bool fail = !chol6_solve(Su, gv, dx);  // a non-positive pivot: the trial is rejected
      double tempChi = DBL_MAX, scale = 0.0;
      double nq[4] = {q[0], q[1], q[2], q[3]}, nt[3] = {t[0], t[1], t[2]};
      if (!fail) {
#pragma unroll
        for (int r = 0; r < 6; ++r) scale += dx[r] * (lambda * dx[r] + gv[r]);
        if (scale <= REFIT_GAIN_TOL * currentChi) {  // (the same bits in every thread: the workgroup leaves together)
          converged = true;
          break;
        }
        ba_se3_oplus(dx, nq, nt);
        tempChi = masked_chi2(A, p0, n, mask, nq, nt, red);
      }
      if (damp.update(currentChi, tempChi, scale, 1.0 / 3.0, 2.0 / 3.0, rho)) {
        currentChi = tempChi;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = nq[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = nt[i];
      }
      ++qmax;
    } while (rho < 0 && qmax < A.max_trials);
    if (converged && qmax == 0) break;  // nothing was tried: not an iteration
    if (trials && threadIdx.x == 0) trials[it] = qmax;
    ++iters;
    if (converged || damp.terminate(qmax, A.max_trials, rho)) go = false;
  }
  if (iters == 0) chi_before = currentChi = masked_chi2(A, p0, n, mask, q, t, red);
  chi_after = currentChi;
}

__device__ __forceinline__ void write_result(const PnpArgs& A, int prob, int status, int best_h, int n_hyp,
                                             double cost_hyp, int n_final, double rms, int iters, const double q[4],
                                             const double t[3]) {
  if (threadIdx.x != 0) return;
  double* d = A.out_d + (size_t)OUT_DOUBLES * prob;
  int32_t* o = A.out_i + (size_t)OUT_INTS * prob;
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = q[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) d[4 + i] = t[i];
  d[7] = cost_hyp; d[8] = rms;
  o[0] = status; o[1] = best_h; o[2] = n_hyp; o[3] = n_final; o[4] = iters;
}

__global__ __launch_bounds__(WG) void k_pnp_ransac(PnpArgs A) {
  __shared__ double s_pts[5 * LDS_POINTS];
  __shared__ double s_pose[7 * WG];
  __shared__ int s_valid[WG];
  __shared__ double red[NWAVE * 32];
  __shared__ double s_best[NWAVE * 10];
  const int tid = threadIdx.x;
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const PtsGlobal G = PnpScore::global(A, p0);
  const double* const P = G.p;
  const double* const UV = G.uv;
  double q[4] = {0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};

  if (n < A.min_points) {  // (the whole workgroup: n is the problem's)
    sim3opt_ransac::clear_mask(A.mask, p0, n);
    write_result(A, prob, 1, -1, 0, 0.0, 0, 0.0, 0, q, t);
    return;
  }
  const bool staged = n <= LDS_POINTS;
  if (staged) stage_points(G, n, s_pts);

  const PnpScore score{A};
  sim3opt_ransac::Best<7> best;
  double* const hp = A.hyp_pose + (size_t)prob * A.H * 7;
  double* const hc = A.hyp_cost + (size_t)prob * A.H;
  int32_t* const hi = A.hyp_int + (size_t)prob * A.H * HYP_INTS;
  for (int first = 0; first < A.H; first += WG) {
    const int h = first + tid;
    if (h < A.H) {
      int idx[4], nsol = 0;
      sim3opt_ransac::ransac_sample<4>(A.seed, (uint32_t)h, n, idx);
      double X[4][3], uv[4][2], R[9], tt[3], pose[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) X[k][c] = P[3 * (size_t)idx[k] + c];
        uv[k][0] = UV[2 * (size_t)idx[k]];
        uv[k][1] = UV[2 * (size_t)idx[k] + 1];
      }
      bool valid = p3p_hypothesis(X, uv, A.f, A.cx, A.cy, R, tt, nsol);
      if (valid) {
        double qq[4];
        R_to_quat(R, qq);
        const double nq = sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
        valid = nq > 0.0 && std::isfinite(nq);
        if (valid) {
#pragma unroll
          for (int i = 0; i < 4; ++i) pose[i] = qq[i] / nq;
#pragma unroll
          for (int i = 0; i < 3; ++i) pose[4 + i] = tt[i];
        }
      }
#pragma unroll
      for (int i = 0; i < 7; ++i) { s_pose[7 * tid + i] = pose[i]; hp[7 * (size_t)h + i] = pose[i]; }
      s_valid[tid] = valid ? 1 : 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) hi[HYP_INTS * (size_t)h + k] = idx[k];
      hi[HYP_INTS * (size_t)h + 4] = nsol;
      hi[HYP_INTS * (size_t)h + 5] = valid ? 1 : 0;
    }
    __syncthreads();  // the chunk's poses (and, the first time, the staged points) are in LDS
    const int m = min(WG, A.H - first);
    if (staged) score_chunk(score, PtsLds{s_pts}, n, s_pose, 7, s_valid, m, first, hi + 6, HYP_INTS, hc, best);
    else score_chunk(score, G, n, s_pose, 7, s_valid, m, first, hi + 6, HYP_INTS, hc, best);
    __syncthreads();  // ... before the next chunk overwrites them
  }

  int n_hyp, best_h;
  double cost_hyp, pose[7];
  sim3opt_ransac::best_of_waves(best, s_best, n_hyp, best_h, cost_hyp, pose);
  if (best_h < 0) {  // no valid hypothesis
    sim3opt_ransac::clear_mask(A.mask, p0, n);
    write_result(A, prob, 2, -1, 0, 0.0, 0, 0.0, 0, q, t);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = pose[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = pose[4 + i];

  int count, iters = 0;
  double cost, chi0, chi1;
  mark_inliers(A, p0, n, q, t, A.mask, red, count, cost);
  if (A.refine_iters > 0) {
    pnp_refit(A, p0, n, A.mask, q, t, red, nullptr, iters, chi0, chi1);
    mark_inliers(A, p0, n, q, t, A.mask, red, count, cost);
  }
  const double rms = count > 0 ? sqrt(cost / (double)count) : 0.0;
  write_result(A, prob, count < A.min_inliers ? 3 : 0, best_h, n_hyp, cost_hyp, count, rms, iters, q, t);
}

// sim3opt_pnp_batch_debug_refine: pnp_refit from a supplied pose on a supplied mask
__global__ __launch_bounds__(WG) void k_pnp_refine(PnpArgs A, const double* poses, const uint8_t* mask,
                                                   double* pose_out, int32_t* iterations, double* chi2,
                                                   int32_t* trials) {
  __shared__ double red[NWAVE * 32];
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  double q[4], t[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = poses[7 * (size_t)prob + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = poses[7 * (size_t)prob + 4 + i];
  int iters;
  double chi0, chi1;
  pnp_refit(A, p0, n, mask, q, t, red, trials + (size_t)prob * A.refine_iters, iters, chi0, chi1);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) pose_out[7 * (size_t)prob + i] = q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pose_out[7 * (size_t)prob + 4 + i] = t[i];
    iterations[prob] = iters;
    chi2[2 * (size_t)prob] = chi0;
    chi2[2 * (size_t)prob + 1] = chi1;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Batch;
struct PnpTraits {  // what the frame's handle needs to know of this stage
  using Options = sim3opt_pnp_batch_options;
  using Args = PnpArgs;
  using Score = PnpScore;
  static constexpr int IN0 = 3, IN1 = 2;  // points, uv1
  static constexpr int SAMPLE = 4, MODEL = 7, HYP_INTS = sim3opt_pnp::HYP_INTS, OUT_DOUBLES = sim3opt_pnp::OUT_DOUBLES,
                       OUT_INTS = sim3opt_pnp::OUT_INTS;
  static constexpr auto KERNEL = &k_pnp_ransac;
  static constexpr const char* PREFIX = "pnp_batch";
  static constexpr const char* IN0_NAME = "point";
  static int32_t n_inliers(const int32_t* o) { return o[3]; }
};

struct Batch : sim3opt_ransac::RansacBatch<PnpTraits, Batch> {
  PnpArgs args() const {
    PnpArgs A{};
    A.ptr = dev.ptr; A.pts = dev.in; A.uv = dev.in + 3 * (size_t)total();
    A.hyp_pose = dev.hyp_model; A.hyp_cost = dev.hyp_cost; A.hyp_int = dev.hyp_int;
    A.out_d = dev.out_d; A.out_i = dev.out_i; A.mask = dev.mask;
    A.f = f; A.cx = cx; A.cy = cy;
    A.thr2 = opt.reproj_error * opt.reproj_error;
    A.tau = opt.tau; A.seed = opt.seed;
    A.H = opt.iterations; A.min_points = opt.min_points; A.min_inliers = opt.min_inliers;
    A.refine_iters = opt.refine_iters; A.max_trials = opt.max_trials;
    return A;
  }

  int debug_refine(const double* poses, const uint8_t* msk, double* pose_out, int32_t* iterations, double* chi2,
                   int32_t* trials) {
    err.clear();
    const int rc = ensure_device("pnp_batch_debug_refine");
    if (rc != SIM3OPT_OK) return rc;
    const size_t N = (size_t)n(), T = (size_t)total(), I = (size_t)opt.refine_iters;
    sim3opt::DevBuf<double> dp, dq, dchi;
    sim3opt::DevBuf<int32_t> dit, dtr;
    sim3opt::DevBuf<uint8_t> dm;
    HIPCHK(dp.alloc(7 * N));
    HIPCHK(dq.alloc(7 * N));
    HIPCHK(dchi.alloc(2 * N));
    HIPCHK(dit.alloc(N));
    HIPCHK(dtr.alloc(std::max<size_t>(N * I, 1)));
    HIPCHK(dm.alloc(T));
    HIPCHK(hipMemcpyAsync(dp.get(), poses, sizeof(double) * 7 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dm.get(), msk, T, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(dtr.get(), 0, sizeof(int32_t) * std::max<size_t>(N * I, 1), stream));
    hipLaunchKernelGGL(k_pnp_refine, dim3((unsigned)N), dim3(WG), 0, stream, args(), dp.get(), dm.get(), dq.get(),
                       dit.get(), dchi.get(), dtr.get());
    HIPCHK(hipGetLastError());
    std::vector<double> hq, hchi;
    std::vector<int32_t> hit, htr;
    HIPCHK(sim3opt::read_back(hq, dq.get(), 7 * N, stream));
    HIPCHK(sim3opt::read_back(hchi, dchi.get(), 2 * N, stream));
    HIPCHK(sim3opt::read_back(hit, dit.get(), N, stream));
    HIPCHK(sim3opt::read_back(htr, dtr.get(), N * I, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (pose_out) std::memcpy(pose_out, hq.data(), sizeof(double) * 7 * N);
    if (chi2) std::memcpy(chi2, hchi.data(), sizeof(double) * 2 * N);
    if (iterations) std::memcpy(iterations, hit.data(), sizeof(int32_t) * N);
    if (trials && N * I) std::memcpy(trials, htr.data(), sizeof(int32_t) * N * I);
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_pnp

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched PnP RANSAC")
// ------------------------------------------------------------------------------------------
struct sim3opt_pnp_batch : sim3opt_pnp::Batch {};

extern "C" {

void sim3opt_pnp_batch_options_default(sim3opt_pnp_batch_options* o) {
  if (!o) return;
  o->reproj_error = 3.0;  // kittiDetector.h:1301
  o->tau = 1e-5;
  o->seed = 0;
  o->iterations = 100;    // :1301
  o->min_inliers = 10;    // :1301
  o->min_points = 9;      // point_count > 8, :1282
  o->refine_iters = 10;
  o->max_trials = 5;
  o->device = -1;
}

sim3opt_pnp_batch* sim3opt_pnp_batch_create(void) {
  return sim3opt::handle_create<sim3opt_pnp_batch>(sim3opt_pnp_batch_options_default);
}

void sim3opt_pnp_batch_destroy(sim3opt_pnp_batch* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_pnp_batch_last_error(const sim3opt_pnp_batch* b) { return b ? b->err.c_str() : "null batch"; }

int sim3opt_pnp_batch_set_options(sim3opt_pnp_batch* b, const sim3opt_pnp_batch_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  if (o->iterations < 1 || o->iterations > 4096 || !(o->reproj_error > 0) || !std::isfinite(o->reproj_error) ||
      o->min_inliers < 0 || o->min_points < 4 || o->refine_iters < 0 || o->max_trials < 1 || !(o->tau > 0) ||
      !std::isfinite(o->tau)) {
    b->err = "pnp_batch_set_options: value out of range";
    return SIM3OPT_ERR_ARG;
  }
  if (o->device != b->opt.device) b->release();  // the device is chosen at the next solve
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_pnp_batch_set_problems(sim3opt_pnp_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                   const double* points, const double* uv1, double focal, double cx, double cy) {
  return b ? b->set_problems(n_problems, point_ptr, points, uv1, focal, cx, cy) : SIM3OPT_ERR_ARG;
}

int sim3opt_pnp_batch_dims(const sim3opt_pnp_batch* b, int32_t* n_problems, int32_t* total_points) {
  return b ? b->dims(n_problems, total_points) : SIM3OPT_ERR_ARG;
}

int sim3opt_pnp_batch_solve(sim3opt_pnp_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "pnp_batch_solve", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve(); });
}

int sim3opt_pnp_batch_get_poses(const sim3opt_pnp_batch* b, double* cam1) {
  return b ? b->get_poses(cam1) : SIM3OPT_ERR_ARG;
}

int sim3opt_pnp_batch_get_inliers(const sim3opt_pnp_batch* b, uint8_t* mask, int32_t* n_inliers) {
  return b ? b->get_inliers(mask, n_inliers) : SIM3OPT_ERR_ARG;
}

int sim3opt_pnp_batch_get_summary(const sim3opt_pnp_batch* b, int32_t* status, int32_t* best_hypothesis,
                                  int32_t* n_inliers_hypothesis, double* cost_hypothesis, double* rms_px,
                                  int32_t* refine_iterations) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k) {
    const int32_t* o = b->out_i.data() + (size_t)sim3opt_pnp::OUT_INTS * k;
    const double* d = b->out_d.data() + (size_t)sim3opt_pnp::OUT_DOUBLES * k;
    if (status) status[k] = o[0];
    if (best_hypothesis) best_hypothesis[k] = o[1];
    if (n_inliers_hypothesis) n_inliers_hypothesis[k] = o[2];
    if (cost_hypothesis) cost_hypothesis[k] = d[7];
    if (rms_px) rms_px[k] = d[8];
    if (refine_iterations) refine_iterations[k] = o[4];
  }
  return SIM3OPT_OK;
}

int sim3opt_pnp_batch_debug_hypotheses(sim3opt_pnp_batch* b, int32_t problem, int32_t* sample, int32_t* n_solutions,
                                       int32_t* valid, double* pose, int32_t* count, double* cost) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "pnp_batch_debug_hypotheses", sim3opt::NO_MEMORY,
                          [&] { return b->debug_hypotheses(problem, sample, n_solutions, valid, pose, count, cost); });
}

int sim3opt_pnp_batch_debug_score(sim3opt_pnp_batch* b, int32_t P, const double* poses, int32_t* count, double* cost) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (P < 1 || P > 4096 || !poses || (!count && !cost)) { b->err = "pnp_batch_debug_score: bad argument"; return SIM3OPT_ERR_ARG; }
  return sim3opt::guarded(b, "pnp_batch_debug_score", sim3opt::NO_MEMORY,
                          [&] { return b->debug_score(P, poses, count, cost); });
}

int sim3opt_pnp_batch_debug_refine(sim3opt_pnp_batch* b, const double* poses, const uint8_t* mask, double* pose_out,
                                   int32_t* iterations, double* chi2, int32_t* trials) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!poses || !mask) { b->err = "pnp_batch_debug_refine: bad argument"; return SIM3OPT_ERR_ARG; }
  if (b->n() >= 1 && !sim3opt::all_finite(poses, 7 * (size_t)b->n())) {
    b->err = "pnp_batch_debug_refine: non-finite pose"; return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "pnp_batch_debug_refine", sim3opt::NO_MEMORY,
                          [&] { return b->debug_refine(poses, mask, pose_out, iterations, chi2, trials); });
}

int sim3opt_median_depth_ratio(int32_t n_problems, const int32_t* point_ptr, const double* depth0,
                               const double* depth1, double* ratio) {
  if (n_problems < 1 || !point_ptr || !depth0 || !depth1 || !ratio) return SIM3OPT_ERR_ARG;
  try {
    if (!sim3opt::check_point_ptr(n_problems, point_ptr).empty()) return SIM3OPT_ERR_ARG;
    const size_t T = (size_t)point_ptr[n_problems];
    if (!sim3opt::all_finite(depth0, T) || !sim3opt::all_finite(depth1, T)) return SIM3OPT_ERR_ARG;
    std::vector<double> a, c;
    for (int32_t k = 0; k < n_problems; ++k) {
      const size_t lo = (size_t)point_ptr[k], n = (size_t)point_ptr[k + 1] - lo;
      const size_t mid = (size_t)(0.5 * (double)n);  // depths.begin() + 0.5 * depths.size(), :1306
      a.assign(depth0 + lo, depth0 + lo + n);
      c.assign(depth1 + lo, depth1 + lo + n);
      std::nth_element(a.begin(), a.begin() + mid, a.end());
      std::nth_element(c.begin(), c.begin() + mid, c.end());
      ratio[k] = c[mid] / a[mid];
    }
  } catch (...) {
    return SIM3OPT_ERR_ARG;
  }
  return SIM3OPT_OK;
}

}  // extern "C"
