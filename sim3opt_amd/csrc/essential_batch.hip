// essential_batch.hip -- the loop detector's essential matrix and relative pose (ExtractCameras,
// kittiDetector.h:279-293: cv::findEssentialMat(points1, points2, focal, pp, RANSAC, 0.999, 1.0, mask) and
// cv::recoverPose, called once per accepted loop candidate at :1161-1185; line 2 of a loopConstraints.txt record)
// for a whole batch of candidates in ONE launch.
//
// PARITY UNPINNED: loopConstraints.txt stores what the reference's runs returned, not the matched pixels they were
// given, and OpenCV's sampling is not reproducible.  This is not OpenCV's algorithm restated: a hypothesis is the
// five-point solution a sixth point chooses (OpenCV scores every solution), every one of `iterations` hypotheses is
// evaluated (OpenCV leaves early on its confidence estimate), the sampler is counter based and reproducible, and the
// pose candidates come from Horn's closed form with a least-squares triangulation (OpenCV: SVD and a DLT).  What is
// OpenCV's: the inlier criterion (Sampson error <= (threshold / focal)^2), the cheirality vote with its distance
// threshold, the narrowing of the mask, and the order of the steps.  tests/essential_ref.py restates the whole
// pipeline independently (action-matrix solver, SVD pose recovery); planted truth checks both.
//
// k_essential_ransac: workgroup = problem, 256 threads, as pnp_batch.hip.  Nothing crosses workgroups, there are no
// atomics and no waits on other workgroups; every loop is bounded by the options or a constant; a problem's result
// depends on its own data and the options only.
//   hypotheses   in chunks of CHUNK = 16: a group of GROUP = 16 lanes makes one hypothesis (essential_math.hpp) in
//                the group's WS_DOUBLES doubles of LDS: ten lanes own one row each of the 10 x 20 matrix (they build
//                it, and reduce it under a pivot every lane finds from the same numbers), then one root each of the
//                degree-10 polynomial; the 5 x 9 null space and the Sturm chain are the first lane's.  Nothing picked
//                at run time is a private array, so nothing of it goes to scratch.  16 lanes because a group must
//                not straddle a wavefront and ten rows need ten lanes; CHUNK = 256 / 16, and its 16 work spaces
//                (29.5 KiB) are what LDS has room for beside the points.
//   scoring,     ransac_frame.hpp (score_chunk, best_of_waves) with EssScore: the Sampson error of the normalised
//   best         correspondences, staged in LDS when the problem has at most LDS_POINTS of them
//   pose, vote   thread t owns the points t, t + 256, ...: the four candidates redundantly per thread from the same
//                bits, every inlier's vote under each, sums by wg_sum; the mask narrowed to the winner's voters
// What this mapping leaves idle: the null space and the polynomials with their Sturm chain are the first lane's
// alone (15 of 16 lanes wait), and the roots use ten lanes of 16; with 352 registers a lane there is one wavefront per
// SIMD.  Spreading those serial phases over the group's lanes is the next thing to do for its time.
// One launch per batch.  k_ransac_score<EssScore> and k_essential_pose run the same scoring and pose code on supplied
// matrices (sim3opt_essential_batch_debug_*).  The handle is the frame's RansacBatch; this file adds args() and the
// pose step's debug entry.
// Static LDS of k_essential_ransac: points 4 x 1072 x 8 = 34304, work spaces 16 x 236 x 8 = 30208 (a hypothesis's E
// lies in its work space), validity 64, reduction 256, best 384: 65216 bytes, below the 64 KiB a workgroup may
// declare statically.
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
#include "essential_math.hpp"
#include "handle_device.hpp"
#include "ransac_frame.hpp"

namespace sim3opt_essential {

using sim3opt_bundle::wg_sum;
using sim3opt_ransac::NWAVE;
using sim3opt_ransac::WG;

constexpr int GROUP = 16;             // lanes of a hypothesis group
constexpr int CHUNK = WG / GROUP;     // hypotheses made, then scored, at a time
constexpr int LDS_POINTS = 1072;      // KITTI-00's candidates have 219-1047 points: all of them are staged
constexpr int HYP_INTS = 9;           // per hypothesis: sample (6), real solutions, valid, inlier count
constexpr int OUT_DOUBLES = 17;       // per problem: pose (7), E (9), cost of the best hypothesis
constexpr int OUT_INTS = 8;           // status, best hypothesis, its inlier count, winning candidate, votes (4)

struct EssArgs {
  const int32_t* ptr;  // n_problems + 1
  const double* uv0;   // total x 2
  const double* uv1;   // total x 2
  double* hyp_E;       // n x H x 9
  double* hyp_cost;    // n x H
  int32_t* hyp_int;    // n x H x HYP_INTS
  double* out_d;       // n x OUT_DOUBLES
  int32_t* out_i;      // n x OUT_INTS
  uint8_t* mask;       // total
  double f, cx, cy, thr2, dist;
  uint64_t seed;
  int32_t H, min_points;
};

struct LaneGroup {  // essential_math.hpp's group on the device: GROUP consecutive lanes of one wavefront
  int lane;
  __device__ __forceinline__ int first() const { return lane; }
  __device__ __forceinline__ int step() const { return GROUP; }
  __device__ __forceinline__ bool leader() const { return lane == 0; }
  // The lanes of a wavefront run in lockstep and its LDS operations complete in order: what is left to do is to keep
  // the compiler from moving an access across the phase boundary.
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};

struct PtsGlobal {  // the correspondences of a problem where the caller's pixels lie, normalised as they are read
  const double* a;
  const double* b;
  double f, cx, cy;
  __device__ __forceinline__ void get(int i, double& x0, double& y0, double& x1, double& y1) const {
    x0 = (a[2 * (size_t)i] - cx) / f; y0 = (a[2 * (size_t)i + 1] - cy) / f;
    x1 = (b[2 * (size_t)i] - cx) / f; y1 = (b[2 * (size_t)i + 1] - cy) / f;
  }
};

struct PtsLds {  // ... and staged: four rows of LDS_POINTS (consecutive lanes, consecutive addresses)
  const double* s;
  __device__ __forceinline__ void get(int i, double& x0, double& y0, double& x1, double& y1) const {
    x0 = s[i]; y0 = s[LDS_POINTS + i]; x1 = s[2 * LDS_POINTS + i]; y1 = s[3 * LDS_POINTS + i];
  }
};

__device__ __forceinline__ void stage_points(const PtsGlobal& G, int n, double* s) {
  for (int i = threadIdx.x; i < n; i += WG)
    G.get(i, s[i], s[LDS_POINTS + i], s[2 * LDS_POINTS + i], s[3 * LDS_POINTS + i]);
}

struct EssScore {  // the frame's scoring policy: an E counts the correspondences within thr2 of it (Sampson)
  static constexpr int DOUBLES = 9, CHUNK = sim3opt_essential::CHUNK, LDS_POINTS = sim3opt_essential::LDS_POINTS,
                       POINT_DOUBLES = 4;
  using Args = EssArgs;
  using Lds = PtsLds;
  struct Prepared { double E[9]; };
  const EssArgs& A;
  static __device__ __forceinline__ PtsGlobal global(const EssArgs& A, int64_t p0) {
    return PtsGlobal{A.uv0 + 2 * p0, A.uv1 + 2 * p0, A.f, A.cx, A.cy};
  }
  static __device__ __forceinline__ void stage(const PtsGlobal& G, int n, double* s) { stage_points(G, n, s); }
  __device__ __forceinline__ void prepare(const double* Es, Prepared& p) const {
#pragma unroll
    for (int i = 0; i < 9; ++i) p.E[i] = Es[i];
  }
  template <class Pts>
  __device__ __forceinline__ bool inlier(const Prepared& p, const Pts& P, int i, double& e2) const {
    double x0, y0, x1, y1;
    P.get(i, x0, y0, x1, y1);
    e2 = ess_sampson(p.E, x0, y0, x1, y1);
    return e2 <= A.thr2;
  }
};

// recoverPose on the points a thread owns.  The inliers are those of E under thr2 (GIVEN = false) or mask_in's
// (GIVEN = true); each votes for the candidates that put it in front of both cameras and nearer than dist.  Leaves
// the four candidates in cand (4 x 7: quaternion, unit t), the votes, the winner (most votes, the lower index on a
// tie) and mask_out narrowed to the winner's voters; count and cost are the inliers' before the narrowing.  Thread t
// reads and writes the mask entries of its own points only.
template <bool GIVEN>
__device__ __forceinline__ void pose_vote(const EssArgs& A, int64_t p0, int n, const double E[9],
                                          const uint8_t* mask_in, uint8_t* mask_out, double* red, double cand[4][7],
                                          int votes[4], int& winner, int& count, double& cost) {
  double R[2][9], t[3];
  const bool ok = ess_candidates(E, R, t);
  const double tm[3] = {-t[0], -t[1], -t[2]};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    ess_R_to_quat(R[c & 1], cand[c]);
#pragma unroll
    for (int i = 0; i < 3; ++i) cand[c][4 + i] = c < 2 ? t[i] : tm[i];
  }
  const PtsGlobal G = EssScore::global(A, p0);
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // (counts are integers below 2^31: a double carries them exactly)
  for (int i = threadIdx.x; i < n; i += WG) {
    double x0, y0, x1, y1;
    G.get(i, x0, y0, x1, y1);
    bool in;
    double e2 = 0.0;
    if (GIVEN) {
      in = mask_in[p0 + i] != 0;
    } else {
      e2 = ess_sampson(E, x0, y0, x1, y1);
      in = e2 <= A.thr2;
    }
    unsigned bits = 0;
    if (in) {
      acc[0] += 1.0; acc[1] += e2;
      if (ok) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (ess_votes(R[c & 1], c < 2 ? t : tm, x0, y0, x1, y1, A.dist)) { bits |= 2u << c; acc[2 + c] += 1.0; }
      }
      bits |= 1u;
    }
    mask_out[p0 + i] = (uint8_t)bits;
  }
  wg_sum(acc, red);
  count = (int)acc[0];
  cost = acc[1];
  winner = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    votes[c] = (int)acc[2 + c];
    if (votes[c] > votes[winner]) winner = c;
  }
  for (int i = threadIdx.x; i < n; i += WG) mask_out[p0 + i] = (mask_out[p0 + i] >> (1 + winner)) & 1u;
}

__device__ __forceinline__ void write_result(const EssArgs& A, int prob, int status, int best_h, int n_hyp,
                                             double cost_hyp, int winner, const int votes[4], const double pose[7],
                                             const double E[9]) {
  if (threadIdx.x != 0) return;
  double* d = A.out_d + (size_t)OUT_DOUBLES * prob;
  int32_t* o = A.out_i + (size_t)OUT_INTS * prob;
#pragma unroll
  for (int i = 0; i < 7; ++i) d[i] = pose[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) d[7 + i] = E[i];
  d[16] = cost_hyp;
  o[0] = status; o[1] = best_h; o[2] = n_hyp; o[3] = winner;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[4 + c] = votes[c];
}

__global__ __launch_bounds__(WG) void k_essential_ransac(EssArgs A) {
  __shared__ double s_pts[4 * LDS_POINTS];
  __shared__ double s_ws[CHUNK * WS_DOUBLES];
  __shared__ int s_valid[CHUNK];
  __shared__ double red[NWAVE * 8];
  __shared__ double s_best[NWAVE * 12];
  const int tid = threadIdx.x;
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const PtsGlobal G = EssScore::global(A, p0);
  const double ident[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, zeroE[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int novotes[4] = {0, 0, 0, 0};

  if (n < A.min_points) {  // (the whole workgroup: n is the problem's)
    sim3opt_ransac::clear_mask(A.mask, p0, n);
    write_result(A, prob, 1, -1, 0, 0.0, 0, novotes, ident, zeroE);
    return;
  }
  const bool staged = n <= LDS_POINTS;
  if (staged) stage_points(G, n, s_pts);

  const EssScore score{A};
  sim3opt_ransac::Best<9> best;
  double* const hE = A.hyp_E + (size_t)prob * A.H * 9;
  double* const hc = A.hyp_cost + (size_t)prob * A.H;
  int32_t* const hi = A.hyp_int + (size_t)prob * A.H * HYP_INTS;
  for (int first = 0; first < A.H; first += CHUNK) {
    const int k = tid / GROUP, h = first + k;
    if (h < A.H) {  // (the same for the lanes of a group)
      const LaneGroup grp{tid % GROUP};
      int idx[6], nsol = 0;
      sim3opt_ransac::ransac_sample<6>(A.seed, (uint32_t)h, n, idx);
      double q[6][4], E[9];
#pragma unroll
      for (int j = 0; j < 6; ++j) G.get(idx[j], q[j][0], q[j][1], q[j][2], q[j][3]);
      double* const ws = s_ws + WS_DOUBLES * k;
      const bool valid = ess_hypothesis(grp, q, ws, E, nsol);  // every lane of the group: the same E
      if (grp.leader()) {
#pragma unroll
        for (int i = 0; i < 9; ++i) { ws[WS_E + i] = E[i]; hE[9 * (size_t)h + i] = E[i]; }
        s_valid[k] = valid ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) hi[HYP_INTS * (size_t)h + j] = idx[j];
        hi[HYP_INTS * (size_t)h + 6] = nsol;
        hi[HYP_INTS * (size_t)h + 7] = valid ? 1 : 0;
      }
    }
    __syncthreads();  // the chunk's matrices (and, the first time, the staged points) are in LDS
    const int m = min(CHUNK, A.H - first);
    const double* const s_E = s_ws + WS_E;  // (a hypothesis's E lies in its work space)
    if (staged) score_chunk(score, PtsLds{s_pts}, n, s_E, WS_DOUBLES, s_valid, m, first, hi + 8, HYP_INTS, hc, best);
    else score_chunk(score, G, n, s_E, WS_DOUBLES, s_valid, m, first, hi + 8, HYP_INTS, hc, best);
    __syncthreads();  // ... before the next chunk overwrites them
  }

  int n_hyp, best_h;
  double cost_hyp, E[9], cand[4][7];
  sim3opt_ransac::best_of_waves(best, s_best, n_hyp, best_h, cost_hyp, E);
  if (best_h < 0) {  // no valid hypothesis
    sim3opt_ransac::clear_mask(A.mask, p0, n);
    write_result(A, prob, 2, -1, 0, 0.0, 0, novotes, ident, zeroE);
    return;
  }
  int votes[4], winner, count;
  double cost;
  pose_vote<false>(A, p0, n, E, nullptr, A.mask, red, cand, votes, winner, count, cost);
  double pose[7];
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c == winner) {
#pragma unroll
      for (int i = 0; i < 7; ++i) pose[i] = cand[c][i];
    }
  write_result(A, prob, votes[winner] > 0 ? 0 : 3, best_h, n_hyp, cost_hyp, winner, votes, pose, E);
}

// sim3opt_essential_batch_debug_pose: pose_vote on a supplied matrix and a supplied inlier set per problem
__global__ __launch_bounds__(WG) void k_essential_pose(EssArgs A, const double* essentials, const uint8_t* mask_in,
                                                       double* cand_out, int32_t* votes_out, int32_t* winner_out,
                                                       uint8_t* mask_out) {
  __shared__ double red[NWAVE * 8];
  const int prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  double E[9], cand[4][7];
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = essentials[9 * (size_t)prob + i];
  int votes[4], winner, count;
  double cost;
  pose_vote<true>(A, p0, n, E, mask_in, mask_out, red, cand, votes, winner, count, cost);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int i = 0; i < 7; ++i) cand_out[(4 * (size_t)prob + c) * 7 + i] = cand[c][i];
      votes_out[4 * (size_t)prob + c] = votes[c];
    }
    winner_out[prob] = winner;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Batch;
struct EssTraits {  // what the frame's handle needs to know of this stage
  using Options = sim3opt_essential_batch_options;
  using Args = EssArgs;
  using Score = EssScore;
  static constexpr int IN0 = 2, IN1 = 2;  // uv0, uv1
  static constexpr int SAMPLE = 6, MODEL = 9, HYP_INTS = sim3opt_essential::HYP_INTS,
                       OUT_DOUBLES = sim3opt_essential::OUT_DOUBLES, OUT_INTS = sim3opt_essential::OUT_INTS;
  static constexpr auto KERNEL = &k_essential_ransac;
  static constexpr const char* PREFIX = "essential_batch";
  static constexpr const char* IN0_NAME = "observation";
  static int32_t n_inliers(const int32_t* o) { return o[4 + o[3]]; }  // the winner's votes
};

struct Batch : sim3opt_ransac::RansacBatch<EssTraits, Batch> {
  EssArgs args() const {
    EssArgs A{};
    A.ptr = dev.ptr; A.uv0 = dev.in; A.uv1 = dev.in + 2 * (size_t)total();
    A.hyp_E = dev.hyp_model; A.hyp_cost = dev.hyp_cost; A.hyp_int = dev.hyp_int;
    A.out_d = dev.out_d; A.out_i = dev.out_i; A.mask = dev.mask;
    A.f = f; A.cx = cx; A.cy = cy;
    const double thr = opt.threshold / f;  // OpenCV divides its threshold by the focal length
    A.thr2 = thr * thr;
    A.dist = opt.distance_threshold; A.seed = opt.seed;
    A.H = opt.iterations; A.min_points = opt.min_points;
    return A;
  }

  int debug_pose(const double* essentials, const uint8_t* msk, double* candidates, int32_t* votes, int32_t* winner,
                 uint8_t* mask_out) {
    err.clear();
    const int rc = ensure_device("essential_batch_debug_pose");
    if (rc != SIM3OPT_OK) return rc;
    const size_t N = (size_t)n(), T = (size_t)total();
    sim3opt::DevBuf<double> de, dcand;
    sim3opt::DevBuf<int32_t> dv, dw;
    sim3opt::DevBuf<uint8_t> dm, dmo;
    HIPCHK(de.alloc(9 * N));
    HIPCHK(dcand.alloc(28 * N));
    HIPCHK(dv.alloc(4 * N));
    HIPCHK(dw.alloc(N));
    HIPCHK(dm.alloc(T));
    HIPCHK(dmo.alloc(T));
    HIPCHK(hipMemcpyAsync(de.get(), essentials, sizeof(double) * 9 * N, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dm.get(), msk, T, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_essential_pose, dim3((unsigned)N), dim3(WG), 0, stream, args(), de.get(), dm.get(),
                       dcand.get(), dv.get(), dw.get(), dmo.get());
    HIPCHK(hipGetLastError());
    std::vector<double> hcand;
    std::vector<int32_t> hv, hw;
    std::vector<uint8_t> hm;
    HIPCHK(sim3opt::read_back(hcand, dcand.get(), 28 * N, stream));
    HIPCHK(sim3opt::read_back(hv, dv.get(), 4 * N, stream));
    HIPCHK(sim3opt::read_back(hw, dw.get(), N, stream));
    HIPCHK(sim3opt::read_back(hm, dmo.get(), T, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (candidates) std::memcpy(candidates, hcand.data(), sizeof(double) * 28 * N);
    if (votes) std::memcpy(votes, hv.data(), sizeof(int32_t) * 4 * N);
    if (winner) std::memcpy(winner, hw.data(), sizeof(int32_t) * N);
    if (mask_out) std::memcpy(mask_out, hm.data(), T);
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_essential

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched essential-matrix RANSAC")
// ------------------------------------------------------------------------------------------
struct sim3opt_essential_batch : sim3opt_essential::Batch {};

extern "C" {

void sim3opt_essential_batch_options_default(sim3opt_essential_batch_options* o) {
  if (!o) return;
  o->threshold = 1.0;            // kittiDetector.h:290
  o->distance_threshold = 50.0;  // cv::recoverPose's [upstream-recall]
  o->seed = 0;
  o->iterations = 1000;          // cv::findEssentialMat's maxIters [upstream-recall]
  o->min_points = 9;             // point_count > 8, :1163
  o->device = -1;
}

sim3opt_essential_batch* sim3opt_essential_batch_create(void) {
  return sim3opt::handle_create<sim3opt_essential_batch>(sim3opt_essential_batch_options_default);
}

void sim3opt_essential_batch_destroy(sim3opt_essential_batch* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_essential_batch_last_error(const sim3opt_essential_batch* b) {
  return b ? b->err.c_str() : "null batch";
}

int sim3opt_essential_batch_set_options(sim3opt_essential_batch* b, const sim3opt_essential_batch_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  if (o->iterations < 1 || o->iterations > 4096 || !(o->threshold > 0) || !std::isfinite(o->threshold) ||
      !(o->distance_threshold > 0) || !std::isfinite(o->distance_threshold) || o->min_points < 6) {
    b->err = "essential_batch_set_options: value out of range";
    return SIM3OPT_ERR_ARG;
  }
  if (o->device != b->opt.device) b->release();  // the device is chosen at the next solve
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_essential_batch_set_problems(sim3opt_essential_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                         const double* uv0, const double* uv1, double focal, double cx, double cy) {
  return b ? b->set_problems(n_problems, point_ptr, uv0, uv1, focal, cx, cy) : SIM3OPT_ERR_ARG;
}

int sim3opt_essential_batch_dims(const sim3opt_essential_batch* b, int32_t* n_problems, int32_t* total_points,
                                 int32_t tiles[2]) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (tiles) { tiles[0] = sim3opt_essential::LDS_POINTS; tiles[1] = sim3opt_essential::CHUNK; }
  return b->dims(n_problems, total_points);
}

int sim3opt_essential_batch_solve(sim3opt_essential_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "essential_batch_solve", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve(); });
}

int sim3opt_essential_batch_get_poses(const sim3opt_essential_batch* b, double* poses) {
  return b ? b->get_poses(poses) : SIM3OPT_ERR_ARG;
}

int sim3opt_essential_batch_get_essentials(const sim3opt_essential_batch* b, double* essentials) {
  if (!b || !essentials) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k)
    std::memcpy(essentials + 9 * (size_t)k, b->out_d.data() + (size_t)sim3opt_essential::OUT_DOUBLES * k + 7,
                sizeof(double) * 9);
  return SIM3OPT_OK;
}

int sim3opt_essential_batch_get_inliers(const sim3opt_essential_batch* b, uint8_t* mask, int32_t* n_inliers) {
  return b ? b->get_inliers(mask, n_inliers) : SIM3OPT_ERR_ARG;
}

int sim3opt_essential_batch_get_summary(const sim3opt_essential_batch* b, int32_t* status, int32_t* best_hypothesis,
                                        int32_t* n_inliers_hypothesis, double* cost_hypothesis, int32_t* winner,
                                        int32_t* votes_winner, int32_t* votes) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n(); ++k) {
    const int32_t* o = b->out_i.data() + (size_t)sim3opt_essential::OUT_INTS * k;
    const double* d = b->out_d.data() + (size_t)sim3opt_essential::OUT_DOUBLES * k;
    if (status) status[k] = o[0];
    if (best_hypothesis) best_hypothesis[k] = o[1];
    if (n_inliers_hypothesis) n_inliers_hypothesis[k] = o[2];
    if (cost_hypothesis) cost_hypothesis[k] = d[16];
    if (winner) winner[k] = o[3];
    if (votes_winner) votes_winner[k] = o[4 + o[3]];
    if (votes)
      for (int c = 0; c < 4; ++c) votes[4 * (size_t)k + c] = o[4 + c];
  }
  return SIM3OPT_OK;
}

int sim3opt_essential_batch_debug_hypotheses(sim3opt_essential_batch* b, int32_t problem, int32_t* sample,
                                             int32_t* n_solutions, int32_t* valid, double* essential, int32_t* count,
                                             double* cost) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "essential_batch_debug_hypotheses", sim3opt::NO_MEMORY, [&] {
    return b->debug_hypotheses(problem, sample, n_solutions, valid, essential, count, cost);
  });
}

int sim3opt_essential_batch_debug_score(sim3opt_essential_batch* b, int32_t P, const double* essentials,
                                        int32_t* count, double* cost) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (P < 1 || P > 4096 || !essentials || (!count && !cost)) {
    b->err = "essential_batch_debug_score: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  if (b->n() >= 1 && !sim3opt::all_finite(essentials, 9 * (size_t)b->n() * (size_t)P)) {
    b->err = "essential_batch_debug_score: non-finite matrix";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "essential_batch_debug_score", sim3opt::NO_MEMORY,
                          [&] { return b->debug_score(P, essentials, count, cost); });
}

int sim3opt_essential_batch_debug_pose(sim3opt_essential_batch* b, const double* essentials, const uint8_t* mask,
                                       double* candidates, int32_t* votes, int32_t* winner, uint8_t* mask_out) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!essentials || !mask) { b->err = "essential_batch_debug_pose: bad argument"; return SIM3OPT_ERR_ARG; }
  if (b->n() >= 1 && !sim3opt::all_finite(essentials, 9 * (size_t)b->n())) {
    b->err = "essential_batch_debug_pose: non-finite matrix";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "essential_batch_debug_pose", sim3opt::NO_MEMORY,
                          [&] { return b->debug_pose(essentials, mask, candidates, votes, winner, mask_out); });
}

}  // extern "C"
