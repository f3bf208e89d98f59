// sim3_batch.hip -- the Sim(3) measurement of a loop candidate with its information matrix, for a whole batch of
// candidates in ONE launch: `iterations` hypotheses by Horn's closed form on three 3-D -- 3-D matches, every one scored
// on the reprojection errors in both images, a Levenberg-Marquardt refinement of the best one on its inliers over the
// seven parameters of C <- exp(delta) C, the final inlier set re-derived with the scoring rule, and
// Omega = sum w J^T J / pixel_noise^2 over it: the `meas` and `info` of sim3opt_add_edge / sim3opt_gate_edges.
//
// PARITY UNPINNED: the reference has no such step -- its scale is a ratio of median depths (kittiDetector.h:1305-1311),
// its rotation and translation come from a rigid two-view BA, every loop edge gets Identity(7) (kitti_surf.cpp:167,
// 202) and Constraint::fisher_information (kittiDetector.h:404-422) is never filled.  The method is ORB-SLAM's
// Sim3Solver / OptimizeSim3; the deviations are listed in sim3_batch_math.hpp and DESIGN.md 5c (the sampler, Horn's
// eigenproblem by Jacobi sweeps, the errors on the camera plane, LM under lm_damping.hpp instead of g2o's fixed five
// iterations, the fixed inlier set during refinement, exp with the exact small-angle B).  tests/sim3_batch_ref.py
// restates the whole pipeline independently (Umeyama by numpy's SVD, Jacobians by central differences).
//
// k_sim3_ransac: workgroup = problem, 256 threads, on ransac_frame.hpp as its three siblings.  Nothing crosses
// workgroups, there are no atomics; every loop is bounded by an option or a constant; a problem's result depends on
// its own data and the options only.
//   hypotheses   in chunks of CHUNK = 128: thread t < 128 makes hypothesis first + t (ransac_sample<3>, s3b_horn: about
//                1500 operations, most of them the Jacobi sweeps).  Scoring one is 60 operations a match, so at the
//                219-1047 matches of KITTI-00's candidates making them is a tenth of the work; half the threads idle
//                through it.  128 rather than 256 leaves LDS for every candidate's matches.
//   scoring      the frame's score_chunk / best_of_waves with Sim3Score (s3b_inlier): count, then cost e0 + e1.
//   inliers      thread t owns the matches t, t + 256, ...: the scoring rule under the best C, into the mask.
//   refinement   LM on that fixed set (s3b_refit): the 28 + 7 + 1 sums by wg_sum -- a thread's matches ascending, a
//                butterfly, the wavefronts in order -- and the 7 x 7 Cholesky by every thread from the same bits, as
//                the 6-DoF refit of k_pnp_ransac.
//   result       the mask re-derived under the refined C, its count and RMS, Omega over it, Omega's Cholesky.
// What this mapping leaves idle: nothing while scoring; 128 threads while hypotheses are made; the 7 x 7 solve is done
// 256 times over instead of once and broadcast (it is short, and a broadcast would cost the barrier it saves).
// Static LDS of k_sim3_ransac: matches 6 x 1072 x 8 = 51456, the chunk's models 128 x 8 x 8 = 8192, validity 512,
// reduction 4 x 36 x 8 = 1152, best 4 x 11 x 8 = 352: 61664 bytes, below the 64 KiB a workgroup may declare statically.
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
#include "ransac_frame.hpp"
#include "sim3_batch_math.hpp"

namespace sim3opt_sim3b {

using sim3opt_bundle::wg_sum;
using sim3opt_ransac::NWAVE;
using sim3opt_ransac::WG;

constexpr int CHUNK = 128;        // hypotheses made, then scored, at a time
constexpr int LDS_POINTS = 1072;  // KITTI-00's candidates have 219-1047 matches: all of them are staged
constexpr double REFIT_GAIN_TOL = 1e-9;  // converged when a step promises less of chi2 than this (as pnp_batch.hip)
constexpr int HYP_INTS = 6;       // per hypothesis: sample (3), solutions (0 / 1), valid, inlier count
// per problem: sim3 (8), Omega (49), the best hypothesis's cost, RMS, chi2 before and after the refinement
constexpr int OUT_DOUBLES = 8 + 49 + 4;
constexpr int OUT_INTS = 5;  // status, best hypothesis, its inlier count, final inlier count, LM iterations
constexpr int D_INFO = 8, D_COST = 57, D_RMS = 58, D_CHI = 59;

struct S3bArgs {
  const int32_t* ptr;  // n_problems + 1
  const double* m0;    // total x 3: u0 v0 depth0
  const double* m1;    // total x 3: u1 v1 depth1
  double* hyp_model;   // n x H x 8
  double* hyp_cost;    // n x H
  int32_t* hyp_int;    // n x H x HYP_INTS
  double* out_d;       // n x OUT_DOUBLES
  int32_t* out_i;      // n x OUT_INTS
  uint8_t* mask;       // total
  double f, cx, cy, max2, huber, pixel_noise, min_sin2, tau;
  uint64_t seed;
  int32_t H, min_points, min_inliers, refine_iters, max_trials;
};

struct PtsGlobal {  // the matches of a problem where the caller's arrays lie
  const double* a;
  const double* b;
  double f, cx, cy;
  __device__ __forceinline__ void get(int i, double p[6]) const {
    const double* x = a + 3 * (size_t)i;
    const double* y = b + 3 * (size_t)i;
    s3b_match(x[0], x[1], x[2], y[0], y[1], y[2], f, cx, cy, p);
  }
};

struct PtsLds {  // ... and staged: six rows of LDS_POINTS (consecutive lanes, consecutive addresses)
  const double* s;
  __device__ __forceinline__ void get(int i, double p[6]) const {
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = s[k * LDS_POINTS + i];
  }
};

__device__ __forceinline__ void stage_points(const PtsGlobal& G, int n, double* s) {
  for (int i = threadIdx.x; i < n; i += WG) {
    double p[6];
    G.get(i, p);
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k * LDS_POINTS + i] = p[k];
  }
}

struct Sim3Score {  // the frame's scoring policy: C counts the matches s3b_inlier admits, at the cost e0 + e1
  static constexpr int DOUBLES = 8, CHUNK = sim3opt_sim3b::CHUNK, LDS_POINTS = sim3opt_sim3b::LDS_POINTS,
                       POINT_DOUBLES = 6;
  using Args = S3bArgs;
  using Lds = PtsLds;
  using Prepared = S3bPrep;
  const S3bArgs& A;
  static __device__ __forceinline__ PtsGlobal global(const S3bArgs& A, int64_t p0) {
    return PtsGlobal{A.m0 + 3 * p0, A.m1 + 3 * p0, A.f, A.cx, A.cy};
  }
  static __device__ __forceinline__ void stage(const PtsGlobal& G, int n, double* s) { stage_points(G, n, s); }
  __device__ __forceinline__ void prepare(const double* m, Prepared& p) const {
    double mm[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) mm[i] = m[i];
    s3b_prepare(mm, p);
  }
  template <class Pts>
  __device__ __forceinline__ bool inlier(const Prepared& p, const Pts& P, int i, double& e2) const {
    double m[6];
    P.get(i, m);
    return s3b_inlier(p, m, A.f, A.max2, e2);
  }
};

// The inliers of C among the matches a thread owns -> mask; their count and the sum of e0 + e1 over the workgroup
template <class Pts>
__device__ __forceinline__ void mark_inliers(const S3bArgs& A, const Pts& P, int n, const double C[8], uint8_t* mask,
                                             double* red, int& count, double& cost) {
  S3bPrep prep;
  s3b_prepare(C, prep);
  double acc[2] = {0.0, 0.0};  // (the count is an integer below 2^31: a double carries it exactly)
  for (int i = threadIdx.x; i < n; i += WG) {
    double p[6], e2;
    P.get(i, p);
    const bool in = s3b_inlier(prep, p, A.f, A.max2, e2);
    mask[i] = in ? 1 : 0;
    if (in) { acc[0] += 1.0; acc[1] += e2; }
  }
  wg_sum(acc, red);
  count = (int)acc[0];
  cost = acc[1];
}

// the sums of an LM iteration at C over the masked matches (S3B_ACC, the same bits in every thread); weights
// (n x 2, or null) gets the Huber weights of every match (0 where the mask is)
template <class Pts>
__device__ __forceinline__ void linearize(const S3bArgs& A, const Pts& P, int n, const uint8_t* in, const double C[8],
                                          double (&acc)[S3B_ACC], double* red, double* weights) {
  S3bPrep prep;
  s3b_prepare(C, prep);
#pragma unroll
  for (int k = 0; k < S3B_ACC; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < n; i += WG) {
    double w[2] = {0.0, 0.0};
    if (in[i] != 0) {
      double p[6];
      P.get(i, p);
      s3b_accumulate(prep, p, A.f, A.huber, acc, w);
    }
    if (weights) { weights[2 * (size_t)i] = w[0]; weights[2 * (size_t)i + 1] = w[1]; }
  }
  wg_sum(acc, red);
}

template <class Pts>
__device__ __forceinline__ double masked_chi2(const S3bArgs& A, const Pts& P, int n, const uint8_t* in,
                                              const double C[8], double* red) {
  S3bPrep prep;
  s3b_prepare(C, prep);
  double acc[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += WG) {
    if (in[i] == 0) continue;
    double p[6];
    P.get(i, p);
    acc[0] += s3b_chi2(prep, p, A.f, A.huber);
  }
  wg_sum(acc, red);
  return acc[0];
}

// The refinement: LM on the seven parameters of C <- exp(delta) C over the masked matches (fixed), Huber of width
// A.huber per reprojection, lambda_0 = tau max diag(H), at most refine_iters iterations of at most max_trials trials
// under lm_damping.hpp's rule.  As pnp_refit it also ends when a step promises nothing: x.(lambda x + b) at most
// REFIT_GAIN_TOL of chi2.  trials (refine_iters entries, or null) gets the trial count of every iteration run.
template <class Pts>
__device__ __forceinline__ void s3b_refit(const S3bArgs& A, const Pts& P, int n, const uint8_t* in, double C[8],
                                          double* red, int32_t* trials, int& iters, double& chi_before,
                                          double& chi_after) {
  sim3opt::LmDamping damp;
  bool go = true;
  iters = 0;
  double currentChi = 0.0;
  for (int it = 0; it < A.refine_iters && go; ++it) {
    double acc[S3B_ACC];
    linearize(A, P, n, in, C, acc, red, nullptr);
    currentChi = acc[35];
    if (it == 0) {
      chi_before = currentChi;
      double maxdiag = 0.0;
#pragma unroll
      for (int r = 0; r < 7; ++r) maxdiag = fmax(maxdiag, acc[tri7(r, r)]);
      damp.start(0.0, A.tau, maxdiag);
    }
    double rho = 0.0;
    int qmax = 0;
    bool converged = false;
    do {
      const double lambda = damp.lambda;
      double Su[28], gv[7], dx[7];
#pragma unroll
      for (int k = 0; k < 28; ++k) Su[k] = acc[k];
#pragma unroll
      for (int r = 0; r < 7; ++r) {
        Su[tri7(r, r)] += lambda;
        gv[r] = acc[28 + r];
      }
      const bool fail = !s3b_chol7_solve(Su, gv, dx);  // a non-positive pivot: the trial is rejected
      double tempChi = DBL_MAX, scale = 0.0;
      double nC[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) nC[i] = C[i];
      if (!fail) {
#pragma unroll
        for (int r = 0; r < 7; ++r) scale += dx[r] * (lambda * dx[r] + gv[r]);
        if (scale <= REFIT_GAIN_TOL * currentChi) {  // (the same bits in every thread: the workgroup leaves together)
          converged = true;
          break;
        }
        s3b_oplus(dx, nC);
        tempChi = masked_chi2(A, P, n, in, nC, red);
      }
      if (damp.update(currentChi, tempChi, scale, 1.0 / 3.0, 2.0 / 3.0, rho)) {
        currentChi = tempChi;
#pragma unroll
        for (int i = 0; i < 8; ++i) C[i] = nC[i];
      }
      ++qmax;
    } while (rho < 0 && qmax < A.max_trials);
    if (converged && qmax == 0) break;  // nothing was tried: not an iteration
    if (trials && threadIdx.x == 0) trials[it] = qmax;
    ++iters;
    if (converged || damp.terminate(qmax, A.max_trials, rho)) go = false;
  }
  if (iters == 0) chi_before = currentChi = masked_chi2(A, P, n, in, C, red);
  chi_after = currentChi;
}

// Omega at C over the masked matches -> info (49, written by thread 0; may be null); whether its Cholesky succeeds
template <class Pts>
__device__ __forceinline__ bool information(const S3bArgs& A, const Pts& P, int n, const uint8_t* in, const double C[8],
                                            double* red, double* info, double* weights) {
  double acc[S3B_ACC], om[49];
  linearize(A, P, n, in, C, acc, red, weights);
  s3b_information(acc, A.pixel_noise, om);
  double Su[28], z[7], x[7];
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    z[r] = 0.0;
#pragma unroll
    for (int c = r; c < 7; ++c) Su[tri7(r, c)] = om[7 * c + r];
  }
  const bool ok = s3b_chol7_solve(Su, z, x);
  if (info && threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 49; ++i) info[i] = om[i];
  }
  return ok;
}

// a problem that ends before the refinement: the identity, Omega zero
__device__ __forceinline__ void write_early(const S3bArgs& A, int prob, int status) {
  if (threadIdx.x != 0) return;
  double* d = A.out_d + (size_t)OUT_DOUBLES * prob;
  int32_t* o = A.out_i + (size_t)OUT_INTS * prob;
  for (int i = 0; i < OUT_DOUBLES; ++i) d[i] = 0.0;
  d[3] = 1.0; d[7] = 1.0;
  o[0] = status; o[1] = -1; o[2] = 0; o[3] = 0; o[4] = 0;
}

// from the best hypothesis on: inliers, refinement, final mask, Omega, the problem's outputs
template <class Pts>
__device__ __forceinline__ void finish(const S3bArgs& A, const Pts& P, int n, int prob, uint8_t* mask, double* red,
                                       int best_h, int n_hyp, double cost_hyp, double C[8]) {
  int count, iters = 0;
  double cost, chi0 = 0.0, chi1 = 0.0;
  mark_inliers(A, P, n, C, mask, red, count, cost);
  if (A.refine_iters > 0) {  // (a thread reads the mask entries it wrote itself)
    s3b_refit(A, P, n, mask, C, red, nullptr, iters, chi0, chi1);
    mark_inliers(A, P, n, C, mask, red, count, cost);
  }
  double* const d = A.out_d + (size_t)OUT_DOUBLES * prob;
  int32_t* const o = A.out_i + (size_t)OUT_INTS * prob;
  const bool pd = information(A, P, n, mask, C, red, d + D_INFO, nullptr);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = C[i];
    d[D_COST] = cost_hyp;
    d[D_RMS] = count > 0 ? sqrt(cost / (2.0 * (double)count)) : 0.0;  // per reprojection, two a match
    d[D_CHI] = chi0; d[D_CHI + 1] = chi1;
    o[0] = count < A.min_inliers ? 3 : (pd ? 0 : 4);
    o[1] = best_h; o[2] = n_hyp; o[3] = count; o[4] = iters;
  }
}

__global__ __launch_bounds__(WG) void k_sim3_ransac(S3bArgs A) {
  __shared__ double s_pts[6 * LDS_POINTS];
  __shared__ double s_model[8 * CHUNK];
  __shared__ int s_valid[CHUNK];
  __shared__ double red[NWAVE * S3B_ACC];
  __shared__ double s_best[NWAVE * 11];
  const int tid = threadIdx.x;
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const PtsGlobal G = Sim3Score::global(A, p0);
  uint8_t* const mask = A.mask + p0;

  if (n < A.min_points) {  // (the whole workgroup: n is the problem's)
    sim3opt_ransac::clear_mask(A.mask, p0, n);
    write_early(A, prob, 1);
    return;
  }
  const bool staged = n <= LDS_POINTS;
  if (staged) stage_points(G, n, s_pts);

  const Sim3Score score{A};
  sim3opt_ransac::Best<8> best;
  double* const hm = A.hyp_model + (size_t)prob * A.H * 8;
  double* const hc = A.hyp_cost + (size_t)prob * A.H;
  int32_t* const hi = A.hyp_int + (size_t)prob * A.H * HYP_INTS;
  for (int first = 0; first < A.H; first += CHUNK) {
    const int h = first + tid;
    if (tid < CHUNK && h < A.H) {
      int idx[3];
      sim3opt_ransac::ransac_sample<3>(A.seed, (uint32_t)h, n, idx);
      double s[3][6], m[8];
#pragma unroll
      for (int j = 0; j < 3; ++j) G.get(idx[j], s[j]);
      const bool valid = s3b_horn(s, A.min_sin2, m);  // (invalid: the identity, never a NaN)
#pragma unroll
      for (int i = 0; i < 8; ++i) { s_model[8 * tid + i] = m[i]; hm[8 * (size_t)h + i] = m[i]; }
      s_valid[tid] = valid ? 1 : 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) hi[HYP_INTS * (size_t)h + j] = idx[j];
      hi[HYP_INTS * (size_t)h + 3] = valid ? 1 : 0;
      hi[HYP_INTS * (size_t)h + 4] = valid ? 1 : 0;
    }
    __syncthreads();  // the chunk's models (and, the first time, the staged matches) are in LDS
    const int m = min(CHUNK, A.H - first);
    if (staged) score_chunk(score, PtsLds{s_pts}, n, s_model, 8, s_valid, m, first, hi + 5, HYP_INTS, hc, best);
    else score_chunk(score, G, n, s_model, 8, s_valid, m, first, hi + 5, HYP_INTS, hc, best);
    __syncthreads();  // ... before the next chunk overwrites them
  }

  int n_hyp, best_h;
  double cost_hyp, C[8];
  sim3opt_ransac::best_of_waves(best, s_best, n_hyp, best_h, cost_hyp, C);
  if (best_h < 0) {  // no valid hypothesis
    sim3opt_ransac::clear_mask(A.mask, p0, n);
    write_early(A, prob, 2);
    return;
  }
  if (staged) finish(A, PtsLds{s_pts}, n, prob, mask, red, best_h, n_hyp, cost_hyp, C);
  else finish(A, G, n, prob, mask, red, best_h, n_hyp, cost_hyp, C);
}

// sim3opt_sim3_batch_debug_refine: s3b_refit from a supplied C on a supplied mask per problem
__global__ __launch_bounds__(WG) void k_sim3_refine(S3bArgs A, const double* sims, const uint8_t* mask_in,
                                                    double* sim_out, int32_t* iterations, double* chi2,
                                                    int32_t* trials) {
  __shared__ double red[NWAVE * S3B_ACC];
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const PtsGlobal G = Sim3Score::global(A, p0);
  double C[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) C[i] = sims[8 * (size_t)prob + i];
  int iters;
  double chi0, chi1;
  s3b_refit(A, G, n, mask_in + p0, C, red, trials + (size_t)prob * A.refine_iters, iters, chi0, chi1);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) sim_out[8 * (size_t)prob + i] = C[i];
    iterations[prob] = iters;
    chi2[2 * (size_t)prob] = chi0;
    chi2[2 * (size_t)prob + 1] = chi1;
  }
}

// sim3opt_sim3_batch_debug_information: Omega and the Huber weights at a supplied C on a supplied mask, no LM
__global__ __launch_bounds__(WG) void k_sim3_information(S3bArgs A, const double* sims, const uint8_t* mask_in,
                                                         double* info, double* weights, int32_t* pd) {
  __shared__ double red[NWAVE * S3B_ACC];
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const PtsGlobal G = Sim3Score::global(A, p0);
  double C[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) C[i] = sims[8 * (size_t)prob + i];
  const bool ok = information(A, G, n, mask_in + p0, C, red, info + (size_t)49 * prob, weights + 2 * p0);
  if (threadIdx.x == 0) pd[prob] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Batch;
struct S3bTraits {  // what the frame's handle needs to know of this stage
  using Options = sim3opt_sim3_batch_options;
  using Args = S3bArgs;
  using Score = Sim3Score;
  static constexpr int IN0 = 3, IN1 = 3;  // (u0, v0, depth0), (u1, v1, depth1)
  static constexpr int SAMPLE = 3, MODEL = 8, HYP_INTS = sim3opt_sim3b::HYP_INTS,
                       OUT_DOUBLES = sim3opt_sim3b::OUT_DOUBLES, OUT_INTS = sim3opt_sim3b::OUT_INTS;
  static constexpr auto KERNEL = &k_sim3_ransac;
  static constexpr const char* PREFIX = "sim3_batch";
  static constexpr const char* IN0_NAME = "observation or depth";
  static int32_t n_inliers(const int32_t* o) { return o[3]; }
};

struct Batch : sim3opt_ransac::RansacBatch<S3bTraits, Batch> {
  S3bArgs args() const {
    S3bArgs A{};
    A.ptr = dev.ptr; A.m0 = dev.in; A.m1 = dev.in + 3 * (size_t)total();
    A.hyp_model = dev.hyp_model; A.hyp_cost = dev.hyp_cost; A.hyp_int = dev.hyp_int;
    A.out_d = dev.out_d; A.out_i = dev.out_i; A.mask = dev.mask;
    A.f = f; A.cx = cx; A.cy = cy;
    A.max2 = opt.max_pixel_error * opt.max_pixel_error;
    A.huber = opt.huber_delta; A.pixel_noise = opt.pixel_noise; A.min_sin2 = opt.min_triangle_sin2;
    A.tau = opt.tau; A.seed = opt.seed;
    A.H = opt.iterations; A.min_points = opt.min_points; A.min_inliers = opt.min_inliers;
    A.refine_iters = opt.refine_iters; A.max_trials = opt.max_trials;
    return A;
  }

  // (u, v, depth) x 2 from the four arrays sim3opt_match_batch_get_matches returns
  int set_matches(int32_t n_problems, const int32_t* point_ptr, const double* uv0, const double* uv1,
                  const double* depth0, const double* depth1, double focal, double pcx, double pcy) {
    return sim3opt::guarded(this, "sim3_batch", "_set_problems: out of host memory", [&]() -> int {
      const std::string w = who("_set_problems");
      if (n_problems < 1 || !point_ptr || !uv0 || !uv1 || !depth0 || !depth1) {
        err = w + ": bad argument";
        return SIM3OPT_ERR_ARG;
      }
      const std::string e = sim3opt::check_point_ptr(n_problems, point_ptr);
      if (!e.empty()) { err = w + ": " + e; return SIM3OPT_ERR_ARG; }
      const size_t P = (size_t)point_ptr[n_problems];
      std::vector<double> a(3 * P), b(3 * P);
      for (size_t i = 0; i < P; ++i) {
        if (!(depth0[i] > 0) || !(depth1[i] > 0)) {
          if (std::isfinite(depth0[i]) && std::isfinite(depth1[i])) {
            err = w + ": depth of match " + std::to_string(i) + " is not positive";
            return SIM3OPT_ERR_ARG;
          }
        }
        a[3 * i] = uv0[2 * i]; a[3 * i + 1] = uv0[2 * i + 1]; a[3 * i + 2] = depth0[i];
        b[3 * i] = uv1[2 * i]; b[3 * i + 1] = uv1[2 * i + 1]; b[3 * i + 2] = depth1[i];
      }
      return set_problems(n_problems, point_ptr, a.data(), b.data(), focal, pcx, pcy);
    });
  }

  // every supplied C of a diagnostic is a similarity: finite, a quaternion that is not zero, s > 0
  int check_sims(const std::string& w, const double* sims) {
    for (int32_t k = 0; k < n(); ++k) {
      const double* s = sims + 8 * (size_t)k;
      const double nq = s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3];
      if (!sim3opt::all_finite(s, 8) || !(s[7] > 0) || !(nq > 0)) {
        err = w + ": sim3 " + std::to_string(k) + " is not a similarity";
        return SIM3OPT_ERR_ARG;
      }
    }
    return SIM3OPT_OK;
  }

  int debug_refine(const double* sims, const uint8_t* msk, double* sim_out, int32_t* iterations, double* chi2,
                   int32_t* trials) {
    err.clear();
    if (int rc = ensure_device("sim3_batch_debug_refine")) return rc;
    const size_t N = (size_t)n(), T = (size_t)total(), I = (size_t)opt.refine_iters;
    sim3opt::DevBuf<double> dp, dq, dchi;
    sim3opt::DevBuf<int32_t> dit, dtr;
    sim3opt::DevBuf<uint8_t> dm;
    HIPCHK(dp.alloc(8 * N));
    HIPCHK(dq.alloc(8 * N));
    HIPCHK(dchi.alloc(2 * N));
    HIPCHK(dit.alloc(N));
    HIPCHK(dtr.alloc(std::max<size_t>(N * I, 1)));
    HIPCHK(dm.alloc(T));
    HIPCHK(hipMemcpyAsync(dp.get(), sims, sizeof(double) * 8 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dm.get(), msk, T, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(dtr.get(), 0, sizeof(int32_t) * std::max<size_t>(N * I, 1), stream));
    hipLaunchKernelGGL(k_sim3_refine, dim3((unsigned)N), dim3(WG), 0, stream, args(), dp.get(), dm.get(), dq.get(),
                       dit.get(), dchi.get(), dtr.get());
    HIPCHK(hipGetLastError());
    std::vector<double> hq, hchi;
    std::vector<int32_t> hit, htr;
    HIPCHK(sim3opt::read_back(hq, dq.get(), 8 * N, stream));
    HIPCHK(sim3opt::read_back(hchi, dchi.get(), 2 * N, stream));
    HIPCHK(sim3opt::read_back(hit, dit.get(), N, stream));
    HIPCHK(sim3opt::read_back(htr, dtr.get(), N * I, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (sim_out) std::memcpy(sim_out, hq.data(), sizeof(double) * 8 * N);
    if (chi2) std::memcpy(chi2, hchi.data(), sizeof(double) * 2 * N);
    if (iterations) std::memcpy(iterations, hit.data(), sizeof(int32_t) * N);
    if (trials && N * I) std::memcpy(trials, htr.data(), sizeof(int32_t) * N * I);
    return SIM3OPT_OK;
  }

  int debug_information(const double* sims, const uint8_t* msk, double* info, double* weights,
                        int32_t* positive_definite) {
    err.clear();
    if (int rc = ensure_device("sim3_batch_debug_information")) return rc;
    const size_t N = (size_t)n(), T = (size_t)total();
    sim3opt::DevBuf<double> dp, di, dw;
    sim3opt::DevBuf<int32_t> dpd;
    sim3opt::DevBuf<uint8_t> dm;
    HIPCHK(dp.alloc(8 * N));
    HIPCHK(di.alloc(49 * N));
    HIPCHK(dw.alloc(2 * T));
    HIPCHK(dpd.alloc(N));
    HIPCHK(dm.alloc(T));
    HIPCHK(hipMemcpyAsync(dp.get(), sims, sizeof(double) * 8 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dm.get(), msk, T, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_sim3_information, dim3((unsigned)N), dim3(WG), 0, stream, args(), dp.get(), dm.get(),
                       di.get(), dw.get(), dpd.get());
    HIPCHK(hipGetLastError());
    std::vector<double> hi, hw;
    std::vector<int32_t> hp;
    HIPCHK(sim3opt::read_back(hi, di.get(), 49 * N, stream));
    HIPCHK(sim3opt::read_back(hw, dw.get(), 2 * T, stream));
    HIPCHK(sim3opt::read_back(hp, dpd.get(), N, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (info) std::memcpy(info, hi.data(), sizeof(double) * 49 * N);
    if (weights) std::memcpy(weights, hw.data(), sizeof(double) * 2 * T);
    if (positive_definite) std::memcpy(positive_definite, hp.data(), sizeof(int32_t) * N);
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_sim3b

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched Sim(3) RANSAC and refinement")
// ------------------------------------------------------------------------------------------
struct sim3opt_sim3_batch : sim3opt_sim3b::Batch {};

extern "C" {

void sim3opt_sim3_batch_options_default(sim3opt_sim3_batch_options* o) {
  if (!o) return;
  o->max_pixel_error = 3.034798181098704;  // sqrt(9.210): chi^2_2 at 0.99, sigma = 1 px (ORB-SLAM's th2)
  o->huber_delta = o->max_pixel_error;
  o->pixel_noise = 1.0;
  o->min_triangle_sin2 = 1e-6;
  o->tau = 1e-5;
  o->seed = 0;
  o->iterations = 300;  // ORB-SLAM's SetRansacParameters(0.99, 20, 300)
  o->min_points = 9;
  o->min_inliers = 10;
  o->refine_iters = 10;
  o->max_trials = 5;
  o->device = -1;
}

sim3opt_sim3_batch* sim3opt_sim3_batch_create(void) {
  return sim3opt::handle_create<sim3opt_sim3_batch>(sim3opt_sim3_batch_options_default);
}

void sim3opt_sim3_batch_destroy(sim3opt_sim3_batch* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_sim3_batch_last_error(const sim3opt_sim3_batch* b) { return b ? b->err.c_str() : "null batch"; }

int sim3opt_sim3_batch_set_options(sim3opt_sim3_batch* b, const sim3opt_sim3_batch_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  if (o->iterations < 1 || o->iterations > 4096 || !(o->max_pixel_error > 0) || !std::isfinite(o->max_pixel_error) ||
      !(o->huber_delta >= 0) || !std::isfinite(o->huber_delta) || !(o->pixel_noise > 0) ||
      !std::isfinite(o->pixel_noise) || !(o->min_triangle_sin2 >= 0) || !(o->min_triangle_sin2 < 1) ||
      o->min_inliers < 0 || o->min_points < 3 || o->refine_iters < 0 || o->max_trials < 1 || !(o->tau > 0) ||
      !std::isfinite(o->tau)) {
    b->err = "sim3_batch_set_options: value out of range";
    return SIM3OPT_ERR_ARG;
  }
  if (o->device != b->opt.device) b->release();  // the device is chosen at the next solve
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_sim3_batch_set_problems(sim3opt_sim3_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                    const double* uv0, const double* uv1, const double* depth0, const double* depth1,
                                    double focal, double cx, double cy) {
  return b ? b->set_matches(n_problems, point_ptr, uv0, uv1, depth0, depth1, focal, cx, cy) : SIM3OPT_ERR_ARG;
}

int sim3opt_sim3_batch_dims(const sim3opt_sim3_batch* b, int32_t* n_problems, int32_t* total_points,
                            int32_t tiles[2]) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (tiles) { tiles[0] = sim3opt_sim3b::LDS_POINTS; tiles[1] = sim3opt_sim3b::CHUNK; }
  return b->dims(n_problems, total_points);
}

int sim3opt_sim3_batch_solve(sim3opt_sim3_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "sim3_batch_solve", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve(); });
}

int sim3opt_sim3_batch_get_sim3(const sim3opt_sim3_batch* b, double* sim3, double* information) {
  using namespace sim3opt_sim3b;
  if (!b || (!sim3 && !information)) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k) {
    const double* d = b->out_d.data() + (size_t)OUT_DOUBLES * k;
    if (sim3) std::memcpy(sim3 + 8 * (size_t)k, d, sizeof(double) * 8);
    if (information) std::memcpy(information + 49 * (size_t)k, d + D_INFO, sizeof(double) * 49);
  }
  return SIM3OPT_OK;
}

int sim3opt_sim3_batch_get_inliers(const sim3opt_sim3_batch* b, uint8_t* mask, int32_t* n_inliers) {
  return b ? b->get_inliers(mask, n_inliers) : SIM3OPT_ERR_ARG;
}

int sim3opt_sim3_batch_get_summary(const sim3opt_sim3_batch* b, int32_t* status, int32_t* best_hypothesis,
                                   int32_t* n_inliers_hypothesis, double* cost_hypothesis, double* rms_px,
                                   int32_t* refine_iterations, double* chi2) {
  using namespace sim3opt_sim3b;
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k) {
    const int32_t* o = b->out_i.data() + (size_t)OUT_INTS * k;
    const double* d = b->out_d.data() + (size_t)OUT_DOUBLES * k;
    if (status) status[k] = o[0];
    if (best_hypothesis) best_hypothesis[k] = o[1];
    if (n_inliers_hypothesis) n_inliers_hypothesis[k] = o[2];
    if (cost_hypothesis) cost_hypothesis[k] = d[D_COST];
    if (rms_px) rms_px[k] = d[D_RMS];
    if (refine_iterations) refine_iterations[k] = o[4];
    if (chi2) { chi2[2 * (size_t)k] = d[D_CHI]; chi2[2 * (size_t)k + 1] = d[D_CHI + 1]; }
  }
  return SIM3OPT_OK;
}

int sim3opt_sim3_batch_debug_hypotheses(sim3opt_sim3_batch* b, int32_t problem, int32_t* sample, int32_t* n_solutions,
                                        int32_t* valid, double* sim3, int32_t* count, double* cost) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "sim3_batch_debug_hypotheses", sim3opt::NO_MEMORY,
                          [&] { return b->debug_hypotheses(problem, sample, n_solutions, valid, sim3, count, cost); });
}

int sim3opt_sim3_batch_debug_score(sim3opt_sim3_batch* b, int32_t P, const double* sims, int32_t* count,
                                   double* cost) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (P < 1 || P > 4096 || !sims || (!count && !cost)) {
    b->err = "sim3_batch_debug_score: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  if (b->n() >= 1 && !sim3opt::all_finite(sims, 8 * (size_t)b->n() * (size_t)P)) {
    b->err = "sim3_batch_debug_score: non-finite sim3";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "sim3_batch_debug_score", sim3opt::NO_MEMORY,
                          [&] { return b->debug_score(P, sims, count, cost); });
}

int sim3opt_sim3_batch_debug_refine(sim3opt_sim3_batch* b, const double* sims, const uint8_t* mask, double* sim_out,
                                    int32_t* iterations, double* chi2, int32_t* trials) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!sims || !mask) { b->err = "sim3_batch_debug_refine: bad argument"; return SIM3OPT_ERR_ARG; }
  if (int rc = b->check_sims("sim3_batch_debug_refine", sims)) return rc;
  return sim3opt::guarded(b, "sim3_batch_debug_refine", sim3opt::NO_MEMORY,
                          [&] { return b->debug_refine(sims, mask, sim_out, iterations, chi2, trials); });
}

int sim3opt_sim3_batch_debug_information(sim3opt_sim3_batch* b, const double* sims, const uint8_t* mask,
                                         double* information, double* weights, int32_t* positive_definite) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!sims || !mask || (!information && !weights && !positive_definite)) {
    b->err = "sim3_batch_debug_information: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  if (int rc = b->check_sims("sim3_batch_debug_information", sims)) return rc;
  return sim3opt::guarded(b, "sim3_batch_debug_information", sim3opt::NO_MEMORY, [&] {
    return b->debug_information(sims, mask, information, weights, positive_definite);
  });
}

}  // extern "C"
