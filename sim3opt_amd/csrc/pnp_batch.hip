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
//   scoring      one wavefront per hypothesis of the chunk, lanes over the points (staged in LDS when the problem has
//                at most LDS_POINTS of them, else read from global memory), butterfly sums: inlier count (integer),
//                sum of the inliers' squared errors; every wavefront keeps the best of the hypotheses it scored
//   best         largest count, then smallest cost, then smallest index, over the four wavefronts
//   refit        LM on camera 1 over the best hypothesis's inliers: thread t owns the points t, t + 256, ...; sums by
//                wg_sum, 6x6 Cholesky and the damping rule (lm_damping.hpp) redundantly per thread, as ba_batch.hip
//   final count  inlier mask, count and RMS at the refitted pose
// One launch per batch: no step needs anything from another problem, so there is no reason for a second.
// k_pnp_score and k_pnp_refine run the same scoring and refit code on supplied poses (sim3opt_pnp_batch_debug_*).
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

namespace sim3opt_pnp {

using sim3opt_bundle::ba_jacobians;
using sim3opt_bundle::ba_project_residual;
using sim3opt_bundle::ba_se3_oplus;
using sim3opt_bundle::chol6_solve;
using sim3opt_bundle::R_to_quat;
using sim3opt_bundle::tri6;
using sim3opt_bundle::wg_sum;

constexpr int WG = 256;             // threads of a workgroup (four wavefronts)
constexpr int NWAVE = WG / 64;
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

__device__ __forceinline__ void stage_points(const double* p, const double* uv, int n, double* s) {
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

// One wavefront scores one pose: lane l takes the points l, l + 64, ... in ascending order, then a butterfly; every
// lane ends with the same count and the same bits of cost.
template <class Pts>
__device__ __forceinline__ void score_pose(const Pts& P, int n, const double* pose, double f, double cx, double cy,
                                           double thr2, int& count, double& cost) {
  const int lane = threadIdx.x & 63;
  double R[9];
  const double q[4] = {pose[0], pose[1], pose[2], pose[3]}, t[3] = {pose[4], pose[5], pose[6]};
  pnp_quat_to_R(q, R);
  int c = 0;
  double s = 0.0;
  for (int i = lane; i < n; i += 64) {
    double X[3], u, v, e2;
    P.get(i, X, u, v);
    if (pnp_inlier(R, t, X, u, v, f, cx, cy, thr2, e2)) { ++c; s += e2; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { c += __shfl_xor(c, off); s += __shfl_xor(s, off); }
  count = c;
  cost = s;
}

struct Best {  // of the hypotheses a wavefront has scored: the same in all its lanes
  int count = -1, h = -1;
  double cost = 0.0;
  double pose[7] = {0, 0, 0, 1, 0, 0, 0};
};

// The poses s_pose[7 k], k < m, of a chunk (s_valid[k] says which count): wavefront w scores k = w, w + 4, ...,
// writes count and cost of pose `first + k` and updates its best (larger count, then smaller cost; it goes through
// its hypotheses in ascending order, so of equals the smallest index stays).
template <class Pts>
__device__ __forceinline__ void score_chunk(const Pts& P, int n, const double* s_pose, const int* s_valid, int m,
                                            int first, const PnpArgs& A, int32_t* count_out, int count_stride,
                                            double* cost_out, Best& best) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < m; k += NWAVE) {
    int c = 0;
    double s = 0.0;
    const bool valid = s_valid[k] != 0;
    if (valid) {
      score_pose(P, n, s_pose + 7 * k, A.f, A.cx, A.cy, A.thr2, c, s);
      if (c > best.count || (c == best.count && s < best.cost)) {
        best.count = c; best.cost = s; best.h = first + k;
#pragma unroll
        for (int i = 0; i < 7; ++i) best.pose[i] = s_pose[7 * k + i];
      }
    }
    if (lane == 0) {
      count_out[(size_t)(first + k) * count_stride] = c;
      cost_out[first + k] = s;
    }
  }
}

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
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const double* const P = A.pts + 3 * p0;
  const double* const UV = A.uv + 2 * p0;
  double q[4] = {0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};

  if (n < A.min_points) {  // (the whole workgroup: n is the problem's)
    for (int i = tid; i < n; i += WG) A.mask[p0 + i] = 0;
    write_result(A, prob, 1, -1, 0, 0.0, 0, 0.0, 0, q, t);
    return;
  }
  const bool staged = n <= LDS_POINTS;
  if (staged) stage_points(P, UV, n, s_pts);

  Best best;
  double* const hp = A.hyp_pose + (size_t)prob * A.H * 7;
  double* const hc = A.hyp_cost + (size_t)prob * A.H;
  int32_t* const hi = A.hyp_int + (size_t)prob * A.H * HYP_INTS;
  for (int first = 0; first < A.H; first += WG) {
    const int h = first + tid;
    if (h < A.H) {
      int idx[4], nsol = 0;
      pnp_sample(A.seed, (uint32_t)h, n, idx);
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
    if (staged) score_chunk(PtsLds{s_pts}, n, s_pose, s_valid, m, first, A, hi + 6, HYP_INTS, hc, best);
    else score_chunk(PtsGlobal{P, UV}, n, s_pose, s_valid, m, first, A, hi + 6, HYP_INTS, hc, best);
    __syncthreads();  // ... before the next chunk overwrites them
  }

  // ---- the best of the four wavefronts: count, then cost, then index ----
  if (lane == 0) {
    double* b = s_best + 10 * wave;
    b[0] = (double)best.count; b[1] = best.cost; b[2] = (double)best.h;
#pragma unroll
    for (int i = 0; i < 7; ++i) b[3 + i] = best.pose[i];
  }
  __syncthreads();
  int bw = 0;
  for (int w = 1; w < NWAVE; ++w) {
    const double* a = s_best + 10 * w;
    const double* b = s_best + 10 * bw;
    if (a[2] < 0.0) continue;
    if (b[2] < 0.0 || a[0] > b[0] || (a[0] == b[0] && (a[1] < b[1] || (a[1] == b[1] && a[2] < b[2])))) bw = w;
  }
  const int n_hyp = (int)s_best[10 * bw], best_h = (int)s_best[10 * bw + 2];
  const double cost_hyp = s_best[10 * bw + 1];
  if (best_h < 0) {  // no valid hypothesis
    for (int i = tid; i < n; i += WG) A.mask[p0 + i] = 0;
    write_result(A, prob, 2, -1, 0, 0.0, 0, 0.0, 0, q, t);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = s_best[10 * bw + 3 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = s_best[10 * bw + 7 + i];

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

// sim3opt_pnp_batch_debug_score: P supplied poses per problem through score_chunk
__global__ __launch_bounds__(WG) void k_pnp_score(PnpArgs A, const double* poses, int32_t* count, double* cost) {
  __shared__ double s_pts[5 * LDS_POINTS];
  __shared__ double s_pose[7 * WG];
  __shared__ int s_valid[WG];
  const int tid = threadIdx.x, prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const double* const P = A.pts + 3 * p0;
  const double* const UV = A.uv + 2 * p0;
  const bool staged = n <= LDS_POINTS;
  if (staged) stage_points(P, UV, n, s_pts);
  Best best;
  for (int first = 0; first < A.H; first += WG) {
    if (first + tid < A.H) {
#pragma unroll
      for (int i = 0; i < 7; ++i) s_pose[7 * tid + i] = poses[((size_t)prob * A.H + first + tid) * 7 + i];
      s_valid[tid] = 1;
    }
    __syncthreads();
    const int m = min(WG, A.H - first);
    int32_t* const co = count + (size_t)prob * A.H;
    double* const cs = cost + (size_t)prob * A.H;
    if (staged) score_chunk(PtsLds{s_pts}, n, s_pose, s_valid, m, first, A, co, 1, cs, best);
    else score_chunk(PtsGlobal{P, UV}, n, s_pose, s_valid, m, first, A, co, 1, cs, best);
    __syncthreads();
  }
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
struct Batch : sim3opt::BatchHandle {
  sim3opt_pnp_batch_options opt;
  // the problems, as set
  std::vector<int32_t> ptr;
  std::vector<double> pts, uv;
  double f = 0, cx = 0, cy = 0;
  // the last solve
  std::vector<double> out_d;
  std::vector<int32_t> out_i;
  std::vector<uint8_t> mask;
  int32_t solved_H = 0;
  // device
  sim3opt::DevArena mem;  // the eight blocks of dev
  struct Dev {
    int32_t* ptr;
    double *in, *hyp_pose, *hyp_cost, *out_d;
    int32_t *hyp_int, *out_i;
    uint8_t* mask;
    int64_t cap_n, cap_total, cap_H;  // what the blocks were sized for
    bool uploaded;
  } dev{};

  ~Batch() { release(); }
  int32_t n() const { return ptr.empty() ? 0 : (int32_t)ptr.size() - 1; }
  int64_t total() const { return ptr.empty() ? 0 : ptr.back(); }

  void release() {
    close_stream(mem);
    dev = Dev{};
  }

  // the device, the handle's blocks (sized by the problems and options.iterations) and the problems on the device
  int ensure_device(const char* who) {
    if (n() < 1) { err = std::string(who) + ": no problems set"; return SIM3OPT_ERR_STATE; }
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    const size_t N = (size_t)n(), T = (size_t)total(), H = (size_t)opt.iterations;
    if ((int64_t)N != dev.cap_n || (int64_t)T != dev.cap_total || (int64_t)H != dev.cap_H) {
      release();
      if (int rc = open_stream()) return rc;
      HIPCHK(mem.raw(dev.ptr, N + 1));
      HIPCHK(mem.raw(dev.in, 5 * T));
      HIPCHK(mem.raw(dev.hyp_pose, 7 * N * H));
      HIPCHK(mem.raw(dev.hyp_cost, N * H));
      HIPCHK(mem.raw(dev.hyp_int, HYP_INTS * N * H));
      HIPCHK(mem.raw(dev.out_d, OUT_DOUBLES * N));
      HIPCHK(mem.raw(dev.out_i, OUT_INTS * N));
      HIPCHK(mem.raw(dev.mask, T));
      dev.cap_n = (int64_t)N; dev.cap_total = (int64_t)T; dev.cap_H = (int64_t)H;
    }
    if (!dev.uploaded) {
      HIPCHK(hipMemcpyAsync(dev.ptr, ptr.data(), sizeof(int32_t) * (N + 1), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(dev.in, pts.data(), sizeof(double) * 3 * T, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(dev.in + 3 * T, uv.data(), sizeof(double) * 2 * T, hipMemcpyHostToDevice, stream));
      dev.uploaded = true;
    }
    return SIM3OPT_OK;
  }

  PnpArgs args() const {
    PnpArgs A{};
    A.ptr = dev.ptr; A.pts = dev.in; A.uv = dev.in + 3 * (size_t)total();
    A.hyp_pose = dev.hyp_pose; A.hyp_cost = dev.hyp_cost; A.hyp_int = dev.hyp_int;
    A.out_d = dev.out_d; A.out_i = dev.out_i; A.mask = dev.mask;
    A.f = f; A.cx = cx; A.cy = cy;
    A.thr2 = opt.reproj_error * opt.reproj_error;
    A.tau = opt.tau; A.seed = opt.seed;
    A.H = opt.iterations; A.min_points = opt.min_points; A.min_inliers = opt.min_inliers;
    A.refine_iters = opt.refine_iters; A.max_trials = opt.max_trials;
    return A;
  }

  int solve() {
    err.clear();
    const int rc = ensure_device("pnp_batch_solve");
    if (rc != SIM3OPT_OK) return rc;
    const size_t N = (size_t)n(), T = (size_t)total(), H = (size_t)opt.iterations;
    // hypotheses of a problem that runs none (status 1) read as zeros
    HIPCHK(hipMemsetAsync(dev.hyp_pose, 0, sizeof(double) * 7 * N * H, stream));
    HIPCHK(hipMemsetAsync(dev.hyp_cost, 0, sizeof(double) * N * H, stream));
    HIPCHK(hipMemsetAsync(dev.hyp_int, 0, sizeof(int32_t) * HYP_INTS * N * H, stream));
    hipLaunchKernelGGL(k_pnp_ransac, dim3((unsigned)N), dim3(WG), 0, stream, args());  // the one launch of the batch
    HIPCHK(hipGetLastError());
    std::vector<double> od;
    std::vector<int32_t> oi;
    std::vector<uint8_t> m;
    HIPCHK(sim3opt::read_back(od, dev.out_d, OUT_DOUBLES * N, stream));
    HIPCHK(sim3opt::read_back(oi, dev.out_i, OUT_INTS * N, stream));
    HIPCHK(sim3opt::read_back(m, dev.mask, T, stream));
    HIPCHK(hipStreamSynchronize(stream));
    out_d.swap(od); out_i.swap(oi); mask.swap(m);
    solved_H = opt.iterations;
    have_run = true;
    int ok = 0;
    for (size_t k = 0; k < N; ++k) ok += out_i[OUT_INTS * k] == 0;
    return ok;
  }

  int debug_hypotheses(int32_t problem, int32_t* sample, int32_t* n_solutions, int32_t* valid, double* pose,
                       int32_t* count, double* cost) {
    err.clear();
    if (!have_run) { err = "pnp_batch_debug_hypotheses: no solve yet"; return SIM3OPT_ERR_STATE; }
    if (problem < 0 || problem >= n()) { err = "pnp_batch_debug_hypotheses: no such problem"; return SIM3OPT_ERR_ARG; }
    if (solved_H != opt.iterations || dev.cap_H != solved_H) {
      err = "pnp_batch_debug_hypotheses: options.iterations changed since the solve";
      return SIM3OPT_ERR_STATE;
    }
    const size_t H = (size_t)solved_H;
    std::vector<int32_t> hi;
    std::vector<double> hp, hc;
    HIPCHK(sim3opt::read_back(hi, dev.hyp_int + HYP_INTS * H * problem, HYP_INTS * H, stream));
    HIPCHK(sim3opt::read_back(hp, dev.hyp_pose + 7 * H * problem, 7 * H, stream));
    HIPCHK(sim3opt::read_back(hc, dev.hyp_cost + H * problem, H, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (size_t h = 0; h < H; ++h) {
      if (sample)
        for (int k = 0; k < 4; ++k) sample[4 * h + k] = hi[HYP_INTS * h + k];
      if (n_solutions) n_solutions[h] = hi[HYP_INTS * h + 4];
      if (valid) valid[h] = hi[HYP_INTS * h + 5];
      if (count) count[h] = hi[HYP_INTS * h + 6];
    }
    if (pose) std::memcpy(pose, hp.data(), sizeof(double) * hp.size());
    if (cost) std::memcpy(cost, hc.data(), sizeof(double) * H);
    return SIM3OPT_OK;
  }

  int debug_score(int32_t P, const double* poses, int32_t* count, double* cost) {
    err.clear();
    const int rc = ensure_device("pnp_batch_debug_score");
    if (rc != SIM3OPT_OK) return rc;
    const size_t N = (size_t)n(), M = N * (size_t)P;
    sim3opt::DevBuf<double> dp, dc;
    sim3opt::DevBuf<int32_t> dn;
    HIPCHK(dp.alloc(7 * M));
    HIPCHK(dc.alloc(M));
    HIPCHK(dn.alloc(M));
    HIPCHK(hipMemcpyAsync(dp.get(), poses, sizeof(double) * 7 * M, hipMemcpyHostToDevice, stream));
    PnpArgs A = args();
    A.H = P;
    hipLaunchKernelGGL(k_pnp_score, dim3((unsigned)N), dim3(WG), 0, stream, A, dp.get(), dn.get(), dc.get());
    HIPCHK(hipGetLastError());
    std::vector<int32_t> hn;
    std::vector<double> hc;
    HIPCHK(sim3opt::read_back(hn, dn.get(), M, stream));
    HIPCHK(sim3opt::read_back(hc, dc.get(), M, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (count) std::memcpy(count, hn.data(), sizeof(int32_t) * M);
    if (cost) std::memcpy(cost, hc.data(), sizeof(double) * M);
    return SIM3OPT_OK;
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
  if (!b) return SIM3OPT_ERR_ARG;
  if (n_problems < 1 || !point_ptr || !points || !uv1 || !(focal > 0) || !std::isfinite(focal) ||
      !std::isfinite(cx) || !std::isfinite(cy)) {
    b->err = "pnp_batch_set_problems: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "pnp_batch_set_problems", sim3opt::NO_MEMORY, [&]() -> int {
    const std::string e = sim3opt::check_point_ptr(n_problems, point_ptr);
    if (!e.empty()) { b->err = "pnp_batch_set_problems: " + e; return SIM3OPT_ERR_ARG; }
    const size_t T = (size_t)point_ptr[n_problems];
    if (!sim3opt::all_finite(points, 3 * T)) { b->err = "pnp_batch_set_problems: non-finite point"; return SIM3OPT_ERR_ARG; }
    if (!sim3opt::all_finite(uv1, 2 * T)) { b->err = "pnp_batch_set_problems: non-finite observation"; return SIM3OPT_ERR_ARG; }
    std::vector<int32_t> ptr(point_ptr, point_ptr + n_problems + 1);
    std::vector<double> p(points, points + 3 * T), a(uv1, uv1 + 2 * T);
    // nothing failed: the handle changes now
    b->ptr.swap(ptr); b->pts.swap(p); b->uv.swap(a);
    b->f = focal; b->cx = cx; b->cy = cy;
    b->out_d.clear(); b->out_i.clear(); b->mask.clear();
    b->have_run = false;
    b->dev.uploaded = false;
    return SIM3OPT_OK;
  });
}

int sim3opt_pnp_batch_dims(const sim3opt_pnp_batch* b, int32_t* n_problems, int32_t* total_points) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (n_problems) *n_problems = b->n();
  if (total_points) *total_points = (int32_t)b->total();
  return SIM3OPT_OK;
}

int sim3opt_pnp_batch_solve(sim3opt_pnp_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "pnp_batch_solve", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve(); });
}

int sim3opt_pnp_batch_get_poses(const sim3opt_pnp_batch* b, double* cam1) {
  if (!b || !cam1) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k)
    std::memcpy(cam1 + 7 * (size_t)k, b->out_d.data() + (size_t)sim3opt_pnp::OUT_DOUBLES * k, sizeof(double) * 7);
  return SIM3OPT_OK;
}

int sim3opt_pnp_batch_get_inliers(const sim3opt_pnp_batch* b, uint8_t* mask, int32_t* n_inliers) {
  if (!b || (!mask && !n_inliers)) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  if (mask && !b->mask.empty()) std::memcpy(mask, b->mask.data(), b->mask.size());
  if (n_inliers)
    for (int32_t k = 0; k < b->n(); ++k) n_inliers[k] = b->out_i[(size_t)sim3opt_pnp::OUT_INTS * k + 3];
  return SIM3OPT_OK;
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
