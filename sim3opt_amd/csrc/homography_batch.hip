// homography_batch.hip -- the loop detector's planar relative pose (HomographyInit::Compute(vMatches, 5.0, se3),
// kittiDetector.h:1387-1443, the USE_KLEIN record line; HomographyInit.cc, MEstimator.h) for a whole batch of
// candidates in ONE launch: 300 MLESAC trials of a four-point homography, the inliers of the best one, five
// Tukey-reweighted refinement rounds on that fixed set, the Faugeras-Lustman decomposition into eight (R, t, n, d),
// the two visibility tests and the Sampson tie-break.
//
// PARITY UNPINNED: the reference cannot be built here (TooN and libCVD are absent) and its rand() sampling is not
// reproducible.  Unlike the OpenCV stages this one follows the reference's own statements step by step; ours are the
// sampler (ransac_sample<4>) and the linear algebra (homography_math.hpp), the tie rule of its std::sort (the
// decomposition's number), the pinhole camera in ATANCamera's place and the ten-point minimum (its least-squares
// branch for nine points is not here: status 1).  tests/homography_ref.py restates the whole pipeline independently
// (SVD null space, numpy's SVD, a sorted median); planted truth checks both.
//
// k_homography_ransac: workgroup = problem, 256 threads, on ransac_frame.hpp as pnp_batch.hip and essential_batch.hip.
// Nothing crosses workgroups, there are no atomics; every loop is bounded by an option or a constant; a problem's
// result depends on its own data and the options only.
//   hypotheses   in chunks of CHUNK = 256: thread t makes hypothesis first + t, a closed form of about 150 operations
//                with no work space.  Making one is about 1 % of scoring it, so who makes them hardly matters; one per
//                thread keeps every lane busy, needs two barriers per 256 hypotheses, and the default 300 are two chunks.
//   scoring      the frame's score_chunk / best_of_waves with HomScore: MLESAC -- every point counts and costs
//                min(e2, max_pixel_error^2), so every hypothesis has count n and the frame's order (count, cost,
//                index) is the smallest truncated sum, then the smallest index.
//   inliers      thread t owns the points t, t + 256, ...: e2 < max_pixel_error^2 under the best H, written to the
//                mask once; the set is fixed from here on.
//   refinement   per round: the inliers' squared errors into LDS (the handle's device block when the problem has more
//                than LDS_POINTS points), the median as the exact order statistic by a rank count (ties by index:
//                every thread counts, for its own points, the errors that sort before them; one finds rank m / 2),
//                the 33 sums of the normal equations by wg_sum in a fixed order, the 9 x 9 Cholesky solve by every
//                thread from the same bits.
//   decompose,   the SVD and the decompositions redundantly per thread from the same bits; the visibility counts
//   choose       and the two Sampson sums by wg_sum over the owned points.
// What this mapping leaves idle: nothing while scoring; the rank count is m^2 / 256 comparisons a thread and round
// (4300 at 1047 points) where a selection would do with fewer, and the 9 x 9 solve and the SVD are done 256 times
// over instead of once and broadcast -- they are short, and a broadcast would cost the barrier they save.
// Static LDS of k_homography_ransac: points 4 x 1072 x 8 = 34304, errors 1072 x 8 = 8576, the chunk's matrices
// 256 x 9 x 8 = 18432, validity 1024, reduction 4 x 33 x 8 = 1056, best 384, median 8: 63784 bytes, below the 64 KiB
// a workgroup may declare statically.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "ba_math.hpp"
#include "handle_device.hpp"
#include "homography_math.hpp"
#include "ransac_frame.hpp"

namespace sim3opt_homography {

using sim3opt_bundle::wg_sum;
using sim3opt_ransac::NWAVE;
using sim3opt_ransac::WG;

constexpr int CHUNK = WG;         // hypotheses made, then scored, at a time: one per thread
constexpr int LDS_POINTS = 1072;  // KITTI-00's candidates have 219-1047 points: all of them are staged
constexpr int HYP_INTS = 7;       // per hypothesis: sample (4), solutions (0 / 1), valid, count (= n)
// per problem: pose (7), the MLESAC H (9), the refined H (9), the best cost, sigma^2 of each round (MAX_ROUNDS), the
// two Sampson sums
constexpr int OUT_DOUBLES = 7 + 9 + 9 + 1 + MAX_ROUNDS + 2;
// status, best hypothesis, inliers, first-round counts (8), the four kept, their second-round counts (4), the chosen
// decomposition, whether the ambiguity branch ran
constexpr int OUT_INTS = 3 + 8 + 4 + 4 + 2;
constexpr int D_HM = 7, D_HR = 16, D_COST = 25, D_SIGMA = 26, D_SAMPSON = 26 + MAX_ROUNDS;
constexpr int I_C1 = 3, I_KEPT = 11, I_C2 = 15, I_CHOICE = 19, I_AMBIGUOUS = 20;

struct HomArgs {
  const int32_t* ptr;  // n_problems + 1
  const double* uv0;   // total x 2
  const double* uv1;   // total x 2
  double* hyp_H;       // n x H x 9
  double* hyp_cost;    // n x H
  int32_t* hyp_int;    // n x H x HYP_INTS
  double* out_d;       // n x OUT_DOUBLES
  int32_t* out_i;      // n x OUT_INTS
  uint8_t* mask;       // total
  double* err;         // total: the squared errors of a problem too large for LDS
  double f, cx, cy, max2;
  uint64_t seed;
  int32_t H, min_points, rounds;
};

struct PtsGlobal {  // the correspondences of a problem where the caller's pixels lie: v2CamPlane as they are read
  const double* a;
  const double* b;
  double f, cx, cy;
  __device__ __forceinline__ void get(int i, double& x0, double& y0, double& x1, double& y1) const {
    x0 = (a[2 * (size_t)i] - cx) / f; y0 = (a[2 * (size_t)i + 1] - cy) / f;
    x1 = (b[2 * (size_t)i] - cx) / f; y1 = (b[2 * (size_t)i + 1] - cy) / f;
  }
};

struct PtsLds {  // ... and staged: four rows of LDS_POINTS
  const double* s;
  __device__ __forceinline__ void get(int i, double& x0, double& y0, double& x1, double& y1) const {
    x0 = s[i]; y0 = s[LDS_POINTS + i]; x1 = s[2 * LDS_POINTS + i]; y1 = s[3 * LDS_POINTS + i];
  }
};

__device__ __forceinline__ void stage_points(const PtsGlobal& G, int n, double* s) {
  for (int i = threadIdx.x; i < n; i += WG)
    G.get(i, s[i], s[LDS_POINTS + i], s[2 * LDS_POINTS + i], s[3 * LDS_POINTS + i]);
}

struct HomScore {  // the frame's scoring policy: MLESAC (MLESACScore, HomographyInit.cc:23-33)
  static constexpr int DOUBLES = 9, CHUNK = sim3opt_homography::CHUNK, LDS_POINTS = sim3opt_homography::LDS_POINTS,
                       POINT_DOUBLES = 4;
  using Args = HomArgs;
  using Lds = PtsLds;
  struct Prepared { double H[9]; };
  const HomArgs& A;
  static __device__ __forceinline__ PtsGlobal global(const HomArgs& A, int64_t p0) {
    return PtsGlobal{A.uv0 + 2 * p0, A.uv1 + 2 * p0, A.f, A.cx, A.cy};
  }
  static __device__ __forceinline__ void stage(const PtsGlobal& G, int n, double* s) { stage_points(G, n, s); }
  __device__ __forceinline__ void prepare(const double* Hs, Prepared& p) const {
#pragma unroll
    for (int i = 0; i < 9; ++i) p.H[i] = Hs[i];
  }
  template <class Pts>
  __device__ __forceinline__ bool inlier(const Prepared& p, const Pts& P, int i, double& e2) const {
    double x0, y0, x1, y1;
    P.get(i, x0, y0, x1, y1);
    e2 = hom_mlesac(hom_sqerr(p.H, x0, y0, x1, y1, A.f), A.max2);
    return true;  // every point counts: the order among hypotheses is the cost's
  }
};

// RefineHomographyWithInliers (:120-177), A.rounds times, on the fixed inlier set `in` (the problem's mask entries,
// m of them set, m >= 4).  e: n doubles every thread of the workgroup can read and write (LDS or the handle's block).
// sigma_out (MAX_ROUNDS) and H_rounds (rounds x 9, may be null) are written by thread 0.  H ends the same in every
// thread.
template <class Pts, class Err>
__device__ __forceinline__ void refine(const HomArgs& A, const Pts& P, int n, const uint8_t* in, Err e, int m,
                                       double H[9], double* red, double* s_med, double* sigma_out,
                                       double* H_rounds) {
  const int tid = threadIdx.x;
  for (int r = 0; r < A.rounds; ++r) {
    for (int i = tid; i < n; i += WG) {
      double key = -1.0;  // (no inlier)
      if (in[i] != 0) {
        double x0, y0, x1, y1;
        P.get(i, x0, y0, x1, y1);
        const double e2 = hom_sqerr(H, x0, y0, x1, y1, A.f);
        key = std::isfinite(e2) ? e2 : INFINITY;  // (a non-finite error sorts last)
      }
      e[i] = key;
    }
    __syncthreads();
    // the element of rank m / 2 among the inliers' errors, ties in the order of the points
    for (int i = tid; i < n; i += WG) {
      const double ei = e[i];
      if (ei >= 0.0) {
        int rank = 0;
        for (int j = 0; j < n; ++j) {
          const double ej = e[j];
          rank += (ej >= 0.0 && (ej < ei || (ej == ei && j < i))) ? 1 : 0;
        }
        if (rank == m / 2) s_med[0] = ei;
      }
    }
    __syncthreads();
    const double sigma2 = hom_sigma2(s_med[0], m);
    double acc[HOM_ACC];
#pragma unroll
    for (int q = 0; q < HOM_ACC; ++q) acc[q] = 0.0;
    for (int i = tid; i < n; i += WG) {
      if (in[i] == 0) continue;
      double x0, y0, x1, y1, ex, ey, p0, p1, den;
      P.get(i, x0, y0, x1, y1);
      const double e2 = hom_error(H, x0, y0, x1, y1, A.f, ex, ey, p0, p1, den);
      hom_accumulate(acc, hom_weight(e2, sigma2), x0, y0, A.f, ex, ey, p0, p1, den);
    }
    wg_sum(acc, red);
    double upd[9];
    hom_solve_update(acc, 1.0, upd);
#pragma unroll
    for (int q = 0; q < 9; ++q) H[q] += upd[q];
    if (tid == 0) {
      sigma_out[r] = sigma2;
      if (H_rounds) {
#pragma unroll
        for (int q = 0; q < 9; ++q) H_rounds[9 * r + q] = H[q];
      }
    }
  }
}

struct Choice {  // of DecomposeHomography and ChooseBestDecomposition: the same in every thread
  int status;    // 0, or 4: not the reference's case 1, or a non-finite number
  int c1[8], kept[4], c2[4], choice, ambiguous;
  double sampson[2], pose[7];
};

// DecomposeHomography (:232-339) and ChooseBestDecomposition (:363-435) of H on the inlier set `in`; the Sampson sums
// run over all n points.  decomp_out (8 x 16: R, t, n, d; may be null) is written by thread 0.
template <class Pts>
__device__ __forceinline__ void decompose_choose(const HomArgs& A, const Pts& P, int n, const uint8_t* in,
                                                 const double H[9], double* red, Choice& C, double* decomp_out) {
  const int tid = threadIdx.x;
  C.status = 0; C.choice = 0; C.ambiguous = 0;
  C.sampson[0] = 0.0; C.sampson[1] = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) C.c1[k] = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { C.kept[k] = 0; C.c2[k] = 0; }
#pragma unroll
  for (int k = 0; k < 7; ++k) C.pose[k] = k == 3 ? 1.0 : 0.0;
  HomSvd S;
  if (!hom_svd(H, S)) {  // (the whole workgroup: H has the same bits in every thread)
    C.status = 4;
    return;
  }
  if (decomp_out && tid == 0) {
    for (int k = 0; k < 8; ++k) {
      double R[9], t[3], nn[3], d;
      hom_decomposition(S, k, R, t, nn, d);
      double* o = decomp_out + 16 * k;
#pragma unroll
      for (int q = 0; q < 9; ++q) o[q] = R[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) { o[9 + q] = t[q]; o[12 + q] = nn[q]; }
      o[15] = d;
    }
  }
  // first test: the projective depth of an inlier over d (counts are integers below 2^31: a double carries them)
  double a8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += WG) {
    if (in[i] == 0) continue;
    double x0, y0, x1, y1;
    P.get(i, x0, y0, x1, y1);
#pragma unroll
    for (int k = 0; k < 8; ++k) a8[k] += hom_visible_h(H, x0, y0, hom_decomposition_d(S, k)) ? 1.0 : 0.0;
  }
  wg_sum(a8, red);
  const int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  int k1[4];
#pragma unroll
  for (int k = 0; k < 8; ++k) C.c1[k] = (int)a8[k];
  hom_keep<8, 4>(ids, C.c1, C.kept, k1);
  // second test: the plane's side of the camera
  double n4[4][3], d4[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    double R[9], t[3];
    hom_decomposition(S, C.kept[p], R, t, n4[p], d4[p]);
  }
  double a4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += WG) {
    if (in[i] == 0) continue;
    double x0, y0, x1, y1;
    P.get(i, x0, y0, x1, y1);
#pragma unroll
    for (int p = 0; p < 4; ++p) a4[p] += hom_visible_n(n4[p], x0, y0, d4[p]) ? 1.0 : 0.0;
  }
  wg_sum(a4, red);
#pragma unroll
  for (int p = 0; p < 4; ++p) C.c2[p] = (int)a4[p];
  int kept2[2], k2[2];
  hom_keep<4, 2>(C.kept, C.c2, kept2, k2);
  C.choice = kept2[0];
  C.ambiguous = hom_ambiguous(k2[0], k2[1]) ? 1 : 0;
  double R[9], t[3], nn[3], d;
  if (C.ambiguous) {  // (the whole workgroup)
    double E[2][9];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      hom_decomposition(S, kept2[c], R, t, nn, d);
      hom_essential(R, t, E[c]);
    }
    double a2[2] = {0.0, 0.0};
    const double limit = A.max2 * 4;
    for (int i = tid; i < n; i += WG) {
      double x0, y0, x1, y1;
      P.get(i, x0, y0, x1, y1);
      a2[0] += hom_sampson(E[0], x0, y0, x1, y1, limit);
      a2[1] += hom_sampson(E[1], x0, y0, x1, y1, limit);
    }
    wg_sum(a2, red);
    C.sampson[0] = a2[0]; C.sampson[1] = a2[1];
    C.choice = a2[0] <= a2[1] ? kept2[0] : kept2[1];
  }
  hom_decomposition(S, C.choice, R, t, nn, d);
  hom_R_to_quat(R, C.pose);
#pragma unroll
  for (int q = 0; q < 3; ++q) C.pose[4 + q] = t[q];
}

__device__ __forceinline__ void write_choice(int32_t* o, const Choice& C) {
#pragma unroll
  for (int k = 0; k < 8; ++k) o[I_C1 + k] = C.c1[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) { o[I_KEPT + k] = C.kept[k]; o[I_C2 + k] = C.c2[k]; }
  o[I_CHOICE] = C.choice;
  o[I_AMBIGUOUS] = C.ambiguous;
}

// a problem that ends before the choice: the identity pose, the given matrices (null: zero), nothing else
__device__ __forceinline__ void write_early(const HomArgs& A, int prob, int status, int best_h, int m, double cost,
                                            const double* Hm) {
  if (threadIdx.x != 0) return;
  double* d = A.out_d + (size_t)OUT_DOUBLES * prob;
  int32_t* o = A.out_i + (size_t)OUT_INTS * prob;
  for (int i = 0; i < OUT_DOUBLES; ++i) d[i] = 0.0;
  for (int i = 0; i < OUT_INTS; ++i) o[i] = 0;
  d[3] = 1.0;
  if (Hm) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { d[D_HM + i] = Hm[i]; d[D_HR + i] = Hm[i]; }
  }
  d[D_COST] = cost;
  o[0] = status; o[1] = best_h; o[2] = m;
}

// the inliers among the points a thread owns: e2 < max2 (IsHomographyInlier, :14-21), into the mask; their number
template <class Pts>
__device__ __forceinline__ int mark_inliers(const HomArgs& A, const Pts& P, int n, const double H[9], uint8_t* mask,
                                            double* red) {
  double c[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += WG) {
    double x0, y0, x1, y1;
    P.get(i, x0, y0, x1, y1);
    const bool in = hom_sqerr(H, x0, y0, x1, y1, A.f) < A.max2;
    mask[i] = in ? 1 : 0;
    c[0] += in ? 1.0 : 0.0;
  }
  wg_sum(c, red);
  return (int)c[0];
}

__device__ __forceinline__ int count_mask(const uint8_t* in, int n, double* red) {
  double c[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += WG) c[0] += in[i] != 0 ? 1.0 : 0.0;
  wg_sum(c, red);
  return (int)c[0];
}

__global__ __launch_bounds__(WG) void k_homography_ransac(HomArgs A) {
  __shared__ double s_pts[4 * LDS_POINTS];
  __shared__ double s_err[LDS_POINTS];
  __shared__ double s_model[9 * CHUNK];
  __shared__ int s_valid[CHUNK];
  __shared__ double red[NWAVE * HOM_ACC];
  __shared__ double s_best[NWAVE * 12];
  __shared__ double s_med[1];
  const int tid = threadIdx.x;
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const PtsGlobal G = HomScore::global(A, p0);
  uint8_t* const mask = A.mask + p0;

  if (n < A.min_points) {  // (the whole workgroup: n is the problem's)
    sim3opt_ransac::clear_mask(A.mask, p0, n);
    write_early(A, prob, 1, -1, 0, 0.0, nullptr);
    return;
  }
  const bool staged = n <= LDS_POINTS;
  if (staged) stage_points(G, n, s_pts);

  const HomScore score{A};
  sim3opt_ransac::Best<9> best;
  double* const hH = A.hyp_H + (size_t)prob * A.H * 9;
  double* const hc = A.hyp_cost + (size_t)prob * A.H;
  int32_t* const hi = A.hyp_int + (size_t)prob * A.H * HYP_INTS;
  for (int first = 0; first < A.H; first += CHUNK) {
    const int h = first + tid;
    if (h < A.H) {
      int idx[4];
      sim3opt_ransac::ransac_sample<4>(A.seed, (uint32_t)h, n, idx);
      double q[4][4], Hh[9];
#pragma unroll
      for (int j = 0; j < 4; ++j) G.get(idx[j], q[j][0], q[j][1], q[j][2], q[j][3]);
      const bool valid = hom_four_point(q, Hh);  // (invalid: the identity, never a NaN)
#pragma unroll
      for (int i = 0; i < 9; ++i) { s_model[9 * tid + i] = Hh[i]; hH[9 * (size_t)h + i] = Hh[i]; }
      s_valid[tid] = valid ? 1 : 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) hi[HYP_INTS * (size_t)h + j] = idx[j];
      hi[HYP_INTS * (size_t)h + 4] = valid ? 1 : 0;
      hi[HYP_INTS * (size_t)h + 5] = valid ? 1 : 0;
    }
    __syncthreads();  // the chunk's matrices (and, the first time, the staged points) are in LDS
    const int m = min(CHUNK, A.H - first);
    if (staged) score_chunk(score, PtsLds{s_pts}, n, s_model, 9, s_valid, m, first, hi + 6, HYP_INTS, hc, best);
    else score_chunk(score, G, n, s_model, 9, s_valid, m, first, hi + 6, HYP_INTS, hc, best);
    __syncthreads();  // ... before the next chunk overwrites them
  }

  int n_hyp, best_h;
  double cost_hyp, Hm[9];
  sim3opt_ransac::best_of_waves(best, s_best, n_hyp, best_h, cost_hyp, Hm);
  if (best_h < 0) {  // no valid hypothesis
    sim3opt_ransac::clear_mask(A.mask, p0, n);
    write_early(A, prob, 2, -1, 0, 0.0, nullptr);
    return;
  }
  const int m = staged ? mark_inliers(A, PtsLds{s_pts}, n, Hm, mask, red) : mark_inliers(A, G, n, Hm, mask, red);
  if (m < 4) {
    write_early(A, prob, 3, best_h, m, cost_hyp, Hm);
    return;
  }
  double* const d = A.out_d + (size_t)OUT_DOUBLES * prob;
  int32_t* const o = A.out_i + (size_t)OUT_INTS * prob;
  if (tid == 0) {
    for (int r = 0; r < MAX_ROUNDS; ++r) d[D_SIGMA + r] = 0.0;
  }
  double Hr[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Hr[i] = Hm[i];
  Choice C;
  if (staged) {
    refine(A, PtsLds{s_pts}, n, mask, s_err, m, Hr, red, s_med, d + D_SIGMA, nullptr);
    decompose_choose(A, PtsLds{s_pts}, n, mask, Hr, red, C, nullptr);
  } else {
    refine(A, G, n, mask, A.err + p0, m, Hr, red, s_med, d + D_SIGMA, nullptr);
    decompose_choose(A, G, n, mask, Hr, red, C, nullptr);
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) d[i] = C.pose[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) { d[D_HM + i] = Hm[i]; d[D_HR + i] = Hr[i]; }
    d[D_COST] = cost_hyp;
    d[D_SAMPSON] = C.sampson[0]; d[D_SAMPSON + 1] = C.sampson[1];
    o[0] = C.status; o[1] = best_h; o[2] = m;
    write_choice(o, C);
  }
}

// sim3opt_homography_batch_debug_refine: refine() from a supplied H on a supplied inlier set per problem.  A set of
// fewer than four leaves the problem's outputs as the host cleared them.
__global__ __launch_bounds__(WG) void k_homography_refine(HomArgs A, const double* Hs, const uint8_t* mask_in,
                                                          double* sigma_out, double* H_rounds) {
  __shared__ double s_pts[4 * LDS_POINTS];
  __shared__ double s_err[LDS_POINTS];
  __shared__ double red[NWAVE * HOM_ACC];
  __shared__ double s_med[1];
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const PtsGlobal G = HomScore::global(A, p0);
  const uint8_t* const in = mask_in + p0;
  const int m = count_mask(in, n, red);
  if (m < 4) return;
  double H[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) H[i] = Hs[9 * (size_t)prob + i];
  double* const so = sigma_out + (size_t)MAX_ROUNDS * prob;
  double* const ho = H_rounds + (size_t)MAX_ROUNDS * 9 * prob;
  if (n <= LDS_POINTS) {
    stage_points(G, n, s_pts);
    __syncthreads();
    refine(A, PtsLds{s_pts}, n, in, s_err, m, H, red, s_med, so, ho);
  } else {
    refine(A, G, n, in, A.err + p0, m, H, red, s_med, so, ho);
  }
}

// sim3opt_homography_batch_debug_decompose: decompose_choose() of a supplied H on a supplied inlier set per problem
__global__ __launch_bounds__(WG) void k_homography_decompose(HomArgs A, const double* Hs, const uint8_t* mask_in,
                                                             double* decomp_out, int32_t* int_out, double* dbl_out) {
  __shared__ double red[NWAVE * HOM_ACC];
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const PtsGlobal G = HomScore::global(A, p0);
  const uint8_t* const in = mask_in + p0;
  const int m = count_mask(in, n, red);
  double H[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) H[i] = Hs[9 * (size_t)prob + i];
  Choice C;
  decompose_choose(A, G, n, in, H, red, C, decomp_out + (size_t)128 * prob);
  if (threadIdx.x == 0) {
    int32_t* o = int_out + (size_t)OUT_INTS * prob;
    double* d = dbl_out + (size_t)9 * prob;
    o[0] = C.status; o[1] = -1; o[2] = m;
    write_choice(o, C);
#pragma unroll
    for (int i = 0; i < 7; ++i) d[i] = C.pose[i];
    d[7] = C.sampson[0]; d[8] = C.sampson[1];
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Batch;
struct HomTraits {  // what the frame's handle needs to know of this stage
  using Options = sim3opt_homography_batch_options;
  using Args = HomArgs;
  using Score = HomScore;
  static constexpr int IN0 = 2, IN1 = 2;  // uv0, uv1
  static constexpr int SAMPLE = 4, MODEL = 9, HYP_INTS = sim3opt_homography::HYP_INTS,
                       OUT_DOUBLES = sim3opt_homography::OUT_DOUBLES, OUT_INTS = sim3opt_homography::OUT_INTS;
  static constexpr auto KERNEL = &k_homography_ransac;
  static constexpr const char* PREFIX = "homography_batch";
  static constexpr const char* IN0_NAME = "observation";
  static int32_t n_inliers(const int32_t* o) { return o[2]; }
};

struct Batch : sim3opt_ransac::RansacBatch<HomTraits, Batch> {
  using Base = sim3opt_ransac::RansacBatch<HomTraits, Batch>;
  double* err_blk = nullptr;  // total doubles in the frame's arena: HomArgs::err

  void release() {
    Base::release();
    err_blk = nullptr;
  }

  // the frame's blocks and, with them, this stage's ninth
  int ensure(const std::string& w) {
    if (n() >= 1 && ((int64_t)n() != dev.cap_n || total() != dev.cap_total || (int64_t)opt.iterations != dev.cap_H))
      err_blk = nullptr;  // (ensure_device is about to give every block of the arena back)
    if (int rc = ensure_device(w)) {
      if (!dev.ptr) err_blk = nullptr;
      return rc;
    }
    if (!err_blk) HIPCHK(mem.raw(err_blk, (size_t)total()));
    return SIM3OPT_OK;
  }

  HomArgs args() const {
    HomArgs A{};
    A.ptr = dev.ptr; A.uv0 = dev.in; A.uv1 = dev.in + 2 * (size_t)total();
    A.hyp_H = dev.hyp_model; A.hyp_cost = dev.hyp_cost; A.hyp_int = dev.hyp_int;
    A.out_d = dev.out_d; A.out_i = dev.out_i; A.mask = dev.mask; A.err = err_blk;
    A.f = f; A.cx = cx; A.cy = cy;
    A.max2 = opt.max_pixel_error * opt.max_pixel_error;  // mdMaxPixelErrorSquared, HomographyInit.cc:37
    A.seed = opt.seed;
    A.H = opt.iterations; A.min_points = opt.min_points; A.rounds = opt.refine_rounds;
    return A;
  }

  int solve() {
    err.clear();
    if (int rc = ensure(who("_solve"))) return rc;
    return Base::solve();
  }

  int debug_score(int32_t P, const double* models, int32_t* count, double* cost) {
    err.clear();
    if (int rc = ensure(who("_debug_score"))) return rc;
    return Base::debug_score(P, models, count, cost);
  }

  int debug_refine(const double* Hs, const uint8_t* msk, double* sigma2, double* H_rounds) {
    err.clear();
    if (int rc = ensure("homography_batch_debug_refine")) return rc;
    const size_t N = (size_t)n(), T = (size_t)total(), R = (size_t)opt.refine_rounds;
    sim3opt::DevBuf<double> dh, ds, dr;
    sim3opt::DevBuf<uint8_t> dm;
    HIPCHK(dh.alloc(9 * N));
    HIPCHK(ds.alloc(MAX_ROUNDS * N));
    HIPCHK(dr.alloc(MAX_ROUNDS * 9 * N));
    HIPCHK(dm.alloc(T));
    HIPCHK(hipMemcpyAsync(dh.get(), Hs, sizeof(double) * 9 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dm.get(), msk, T, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(ds.get(), 0, sizeof(double) * MAX_ROUNDS * N, stream));
    HIPCHK(hipMemsetAsync(dr.get(), 0, sizeof(double) * MAX_ROUNDS * 9 * N, stream));
    hipLaunchKernelGGL(k_homography_refine, dim3((unsigned)N), dim3(WG), 0, stream, args(), dh.get(), dm.get(),
                       ds.get(), dr.get());
    HIPCHK(hipGetLastError());
    std::vector<double> hs, hr;
    HIPCHK(sim3opt::read_back(hs, ds.get(), MAX_ROUNDS * N, stream));
    HIPCHK(sim3opt::read_back(hr, dr.get(), MAX_ROUNDS * 9 * N, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (size_t k = 0; k < N; ++k) {
      if (sigma2) std::memcpy(sigma2 + R * k, hs.data() + MAX_ROUNDS * k, sizeof(double) * R);
      if (H_rounds) std::memcpy(H_rounds + 9 * R * k, hr.data() + MAX_ROUNDS * 9 * k, sizeof(double) * 9 * R);
    }
    return SIM3OPT_OK;
  }

  int debug_decompose(const double* Hs, const uint8_t* msk, double* decompositions, int32_t* status,
                      int32_t* counts_first, int32_t* kept, int32_t* counts_second, int32_t* choice,
                      int32_t* ambiguous, double* sampson, double* poses) {
    err.clear();
    if (int rc = ensure("homography_batch_debug_decompose")) return rc;
    const size_t N = (size_t)n(), T = (size_t)total();
    sim3opt::DevBuf<double> dh, dd, dp;
    sim3opt::DevBuf<int32_t> di;
    sim3opt::DevBuf<uint8_t> dm;
    HIPCHK(dh.alloc(9 * N));
    HIPCHK(dd.alloc(128 * N));
    HIPCHK(dp.alloc(9 * N));
    HIPCHK(di.alloc(OUT_INTS * N));
    HIPCHK(dm.alloc(T));
    HIPCHK(hipMemcpyAsync(dh.get(), Hs, sizeof(double) * 9 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dm.get(), msk, T, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(dd.get(), 0, sizeof(double) * 128 * N, stream));
    hipLaunchKernelGGL(k_homography_decompose, dim3((unsigned)N), dim3(WG), 0, stream, args(), dh.get(), dm.get(),
                       dd.get(), di.get(), dp.get());
    HIPCHK(hipGetLastError());
    std::vector<double> hd, hp;
    std::vector<int32_t> hi;
    HIPCHK(sim3opt::read_back(hd, dd.get(), 128 * N, stream));
    HIPCHK(sim3opt::read_back(hp, dp.get(), 9 * N, stream));
    HIPCHK(sim3opt::read_back(hi, di.get(), OUT_INTS * N, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (decompositions) std::memcpy(decompositions, hd.data(), sizeof(double) * 128 * N);
    for (size_t k = 0; k < N; ++k) {
      const int32_t* o = hi.data() + OUT_INTS * k;
      if (status) status[k] = o[0];
      if (counts_first) std::memcpy(counts_first + 8 * k, o + I_C1, sizeof(int32_t) * 8);
      if (kept) std::memcpy(kept + 4 * k, o + I_KEPT, sizeof(int32_t) * 4);
      if (counts_second) std::memcpy(counts_second + 4 * k, o + I_C2, sizeof(int32_t) * 4);
      if (choice) choice[k] = o[I_CHOICE];
      if (ambiguous) ambiguous[k] = o[I_AMBIGUOUS];
      if (sampson) std::memcpy(sampson + 2 * k, hp.data() + 9 * k + 7, sizeof(double) * 2);
      if (poses) std::memcpy(poses + 7 * k, hp.data() + 9 * k, sizeof(double) * 7);
    }
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_homography

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched homography MLESAC")
// ------------------------------------------------------------------------------------------
struct sim3opt_homography_batch : sim3opt_homography::Batch {};

extern "C" {

void sim3opt_homography_batch_options_default(sim3opt_homography_batch_options* o) {
  if (!o) return;
  o->max_pixel_error = 5.0;  // kittiDetector.h:1414
  o->seed = 0;
  o->iterations = 300;       // HomographyInit.cc:195
  o->refine_rounds = 5;      // HomographyInit.cc:48
  o->min_points = 10;        // HomographyInit.cc:182: the MLESAC branch
  o->device = -1;
}

sim3opt_homography_batch* sim3opt_homography_batch_create(void) {
  return sim3opt::handle_create<sim3opt_homography_batch>(sim3opt_homography_batch_options_default);
}

void sim3opt_homography_batch_destroy(sim3opt_homography_batch* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_homography_batch_last_error(const sim3opt_homography_batch* b) {
  return b ? b->err.c_str() : "null batch";
}

int sim3opt_homography_batch_set_options(sim3opt_homography_batch* b, const sim3opt_homography_batch_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  if (o->iterations < 1 || o->iterations > 4096 || !(o->max_pixel_error > 0) || !std::isfinite(o->max_pixel_error) ||
      o->refine_rounds < 0 || o->refine_rounds > sim3opt_homography::MAX_ROUNDS || o->min_points < 4) {
    b->err = "homography_batch_set_options: value out of range";
    return SIM3OPT_ERR_ARG;
  }
  if (o->device != b->opt.device) b->release();  // the device is chosen at the next solve
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_homography_batch_set_problems(sim3opt_homography_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                          const double* uv0, const double* uv1, double focal, double cx, double cy) {
  return b ? b->set_problems(n_problems, point_ptr, uv0, uv1, focal, cx, cy) : SIM3OPT_ERR_ARG;
}

int sim3opt_homography_batch_dims(const sim3opt_homography_batch* b, int32_t* n_problems, int32_t* total_points,
                                  int32_t tiles[2]) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (tiles) { tiles[0] = sim3opt_homography::LDS_POINTS; tiles[1] = sim3opt_homography::CHUNK; }
  return b->dims(n_problems, total_points);
}

int sim3opt_homography_batch_solve(sim3opt_homography_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "homography_batch_solve", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve(); });
}

int sim3opt_homography_batch_get_poses(const sim3opt_homography_batch* b, double* poses) {
  return b ? b->get_poses(poses) : SIM3OPT_ERR_ARG;
}

int sim3opt_homography_batch_get_homographies(const sim3opt_homography_batch* b, double* mlesac, double* refined) {
  using namespace sim3opt_homography;
  if (!b || (!mlesac && !refined)) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k) {
    const double* d = b->out_d.data() + (size_t)OUT_DOUBLES * k;
    if (mlesac) std::memcpy(mlesac + 9 * (size_t)k, d + D_HM, sizeof(double) * 9);
    if (refined) std::memcpy(refined + 9 * (size_t)k, d + D_HR, sizeof(double) * 9);
  }
  return SIM3OPT_OK;
}

int sim3opt_homography_batch_get_inliers(const sim3opt_homography_batch* b, uint8_t* mask, int32_t* n_inliers) {
  return b ? b->get_inliers(mask, n_inliers) : SIM3OPT_ERR_ARG;
}

int sim3opt_homography_batch_get_summary(const sim3opt_homography_batch* b, int32_t* status, int32_t* best_hypothesis,
                                         double* cost_hypothesis, int32_t* n_inliers, double* sigma2,
                                         int32_t* counts_first, int32_t* kept, int32_t* counts_second,
                                         int32_t* choice, int32_t* ambiguous, double* sampson) {
  using namespace sim3opt_homography;
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k) {
    const int32_t* o = b->out_i.data() + (size_t)OUT_INTS * k;
    const double* d = b->out_d.data() + (size_t)OUT_DOUBLES * k;
    if (status) status[k] = o[0];
    if (best_hypothesis) best_hypothesis[k] = o[1];
    if (cost_hypothesis) cost_hypothesis[k] = d[D_COST];
    if (n_inliers) n_inliers[k] = o[2];
    if (sigma2) std::memcpy(sigma2 + (size_t)MAX_ROUNDS * k, d + D_SIGMA, sizeof(double) * MAX_ROUNDS);
    if (counts_first) std::memcpy(counts_first + 8 * (size_t)k, o + I_C1, sizeof(int32_t) * 8);
    if (kept) std::memcpy(kept + 4 * (size_t)k, o + I_KEPT, sizeof(int32_t) * 4);
    if (counts_second) std::memcpy(counts_second + 4 * (size_t)k, o + I_C2, sizeof(int32_t) * 4);
    if (choice) choice[k] = o[I_CHOICE];
    if (ambiguous) ambiguous[k] = o[I_AMBIGUOUS];
    if (sampson) std::memcpy(sampson + 2 * (size_t)k, d + D_SAMPSON, sizeof(double) * 2);
  }
  return SIM3OPT_OK;
}

int sim3opt_homography_batch_debug_hypotheses(sim3opt_homography_batch* b, int32_t problem, int32_t* sample,
                                              int32_t* n_solutions, int32_t* valid, double* homography,
                                              int32_t* count, double* cost) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "homography_batch_debug_hypotheses", sim3opt::NO_MEMORY, [&] {
    return b->debug_hypotheses(problem, sample, n_solutions, valid, homography, count, cost);
  });
}

int sim3opt_homography_batch_debug_score(sim3opt_homography_batch* b, int32_t P, const double* homographies,
                                         int32_t* count, double* cost) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (P < 1 || P > 4096 || !homographies || (!count && !cost)) {
    b->err = "homography_batch_debug_score: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  if (b->n() >= 1 && !sim3opt::all_finite(homographies, 9 * (size_t)b->n() * (size_t)P)) {
    b->err = "homography_batch_debug_score: non-finite matrix";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "homography_batch_debug_score", sim3opt::NO_MEMORY,
                          [&] { return b->debug_score(P, homographies, count, cost); });
}

int sim3opt_homography_batch_debug_refine(sim3opt_homography_batch* b, const double* homographies,
                                          const uint8_t* mask, double* sigma2, double* refined) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!homographies || !mask || (!sigma2 && !refined)) {
    b->err = "homography_batch_debug_refine: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  if (b->n() >= 1 && !sim3opt::all_finite(homographies, 9 * (size_t)b->n())) {
    b->err = "homography_batch_debug_refine: non-finite matrix";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "homography_batch_debug_refine", sim3opt::NO_MEMORY,
                          [&] { return b->debug_refine(homographies, mask, sigma2, refined); });
}

int sim3opt_homography_batch_debug_decompose(sim3opt_homography_batch* b, const double* homographies,
                                             const uint8_t* mask, double* decompositions, int32_t* status,
                                             int32_t* counts_first, int32_t* kept, int32_t* counts_second,
                                             int32_t* choice, int32_t* ambiguous, double* sampson, double* poses) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!homographies || !mask) {
    b->err = "homography_batch_debug_decompose: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  if (b->n() >= 1 && !sim3opt::all_finite(homographies, 9 * (size_t)b->n())) {
    b->err = "homography_batch_debug_decompose: non-finite matrix";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "homography_batch_debug_decompose", sim3opt::NO_MEMORY, [&] {
    return b->debug_decompose(homographies, mask, decompositions, status, counts_first, kept, counts_second, choice,
                              ambiguous, sampson, poses);
  });
}

}  // extern "C"
