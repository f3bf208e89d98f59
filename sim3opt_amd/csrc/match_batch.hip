// match_batch.hip -- the front of the loop detector's computeConstraints for a whole batch of candidates: descriptor
// matching with its filters (kittiDetector.h:1085-1160) and the depth of every kept match from the map
// (:1229-1279).  include/sim3opt.h ("batched descriptor matching") holds the definition the kernels follow.
//
// A solve is two memsets and five launches, whatever the number of pairs:
//   k_match_nn       one workgroup per (pair, tile of QUERY_TILE queries) of a host-built table.  A lane keeps its query
//                    descriptor in 64 registers; the train descriptors pass through LDS TRAIN_TILE at a time, every
//                    lane reading the same address (a broadcast, no bank conflicts); d2 in the difference form with
//                    packed FP32 subtract and multiply-add; (best d2, best index, second d2, second index) per lane.
//                    The lane then applies the ratio, border and skew tests to its query and votes for it with a
//                    64-bit atomicMin on (bits of d2) << 32 | query index at its train keypoint: d2 >= 0, so the bits
//                    order as the value does, and a minimum does not depend on the order of arrival.
//   k_match_count    one workgroup per pair: the queries that won their vote.
//   k_match_scan     one workgroup: match_ptr = the exclusive prefix sum of those counts.
//   k_match_compact  one workgroup per pair: a prefix scan over the survivors' flags, QUERY_TILE queries at a time, so
//                    the matches come out by ascending query index and not by arrival.
//   k_match_depth    one workgroup per (pair, tile of matches, side), one lane per match: the frame's observations pass
//                    through LDS OBS_CHUNK at a time, the K nearest are a sorted list in registers.
// The number of matches is known on the device only, so k_match_depth runs over the tile table of the queries and
// the tiles past a pair's matches return at once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "frames_host.hpp"
#include "handle_device.hpp"
#include "match_host.hpp"

namespace sim3opt_match {

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int WG = QUERY_TILE;
static_assert(WG % WAVE == 0 && (TRAIN_TILE * DESC / 4) % WG == 0, "tile sizes");
constexpr uint8_t PASS_RATIO = 1, PASS_FILTERS = 2;

struct MatchArgs {
  // frames
  const float2* kp;
  const float* desc;
  const float2* obs_uv;
  const float* obs_depth;
  const int32_t *kp_ptr, *obs_ptr;
  // pairs and their plan
  const int32_t *pairs, *qptr, *tptr;
  const Tile* tiles;
  // per query of the OK pairs
  int32_t *best_idx, *second_idx;
  float *best_d2, *second_d2;
  uint8_t* pass;
  // per train keypoint of the OK pairs, per pair
  unsigned long long* vote;
  int32_t *counts, *match_ptr;
  // per match (room for one per query)
  int32_t *m_query, *m_train;
  float* m_dist;
  double *m_uv0, *m_uv1, *m_depth0, *m_depth1, *m_pts;
  // options and intrinsics
  double ratio, x_lo, x_hi, y_lo, y_hi, skew_x, skew_y, f, cx, cy;
  int32_t n_pairs, K, use_ratio;
};

__device__ inline unsigned long long vote_key(float d2, int32_t q) {
  return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(uint32_t)q;
}

// sqrtf, correctly rounded whatever the compiler's flags make of the FP32 instruction: the root of a float taken in
// double and rounded once more is the correctly rounded float root (53 >= 2 * 24 + 2 bits)
__device__ inline float sqrt_rn(float x) { return (float)sqrt((double)x); }

__global__ __launch_bounds__(WG) void k_match_nn(MatchArgs A) {
  __shared__ __attribute__((aligned(16))) float tile[TRAIN_TILE * DESC];
  const Tile t = A.tiles[blockIdx.x];
  const int32_t f0 = A.pairs[2 * t.pair], f1 = A.pairs[2 * t.pair + 1];
  const int32_t q_lo = A.kp_ptr[f0], nq = A.kp_ptr[f0 + 1] - q_lo;
  const int32_t t_lo = A.kp_ptr[f1], nt = A.kp_ptr[f1 + 1] - t_lo;
  const int32_t q = t.q0 + (int32_t)threadIdx.x;
  const bool active = q < nq;
  // (a lane past the pair's last query computes on that query's descriptor and writes nothing)
  const float4* mine = reinterpret_cast<const float4*>(A.desc + (size_t)(q_lo + (active ? q : nq - 1)) * DESC);
  v2f a[DESC / 2];
#pragma unroll
  for (int k = 0; k < DESC / 4; ++k) {
    const float4 v = mine[k];
    a[2 * k] = v2f{v.x, v.y};
    a[2 * k + 1] = v2f{v.z, v.w};
  }
  float best = INFINITY, second = INFINITY;
  int32_t bi = -1, si = -1;
  for (int32_t j0 = 0; j0 < nt; j0 += TRAIN_TILE) {
    const int32_t m = min(TRAIN_TILE, nt - j0);
    const float4* src = reinterpret_cast<const float4*>(A.desc + (size_t)(t_lo + j0) * DESC);
    __syncthreads();  // the tile before is read
    for (int32_t i = threadIdx.x; i < m * (DESC / 4); i += WG) reinterpret_cast<float4*>(tile)[i] = src[i];
    __syncthreads();
#pragma unroll 2
    for (int32_t j = 0; j < m; ++j) {
      const float4* b = reinterpret_cast<const float4*>(tile + j * DESC);
      v2f acc0 = v2f{0.f, 0.f}, acc1 = v2f{0.f, 0.f};
#pragma unroll
      for (int k = 0; k < DESC / 4; ++k) {
        const float4 v = b[k];
        const v2f d0 = a[2 * k] - v2f{v.x, v.y}, d1 = a[2 * k + 1] - v2f{v.z, v.w};
        acc0 = __builtin_elementwise_fma(d0, d0, acc0);
        acc1 = __builtin_elementwise_fma(d1, d1, acc1);
      }
      const float d = (acc0.x + acc0.y) + (acc1.x + acc1.y);
      // strict comparisons: on equal d2 the lower train index stays, as nearest and as second nearest (the index
      // tests: a d2 that overflowed to +inf still names a train keypoint)
      if (d < best || bi < 0) {
        second = best; si = bi;
        best = d; bi = j0 + j;
      } else if (d < second || si < 0) {
        second = d; si = j0 + j;
      }
    }
  }
  // the ratio, border and skew tests of the lane's query, and its vote
  bool ratio_ok = false, filters_ok = false;
  if (active) {
    const size_t o = (size_t)A.qptr[t.pair] + q;
    A.best_idx[o] = bi; A.best_d2[o] = best;
    A.second_idx[o] = si; A.second_d2[o] = second;
    ratio_ok = true;
    if (A.use_ratio) {
      const float d1 = sqrt_rn(best), d2 = sqrt_rn(second);
      ratio_ok = nt >= 2 && ((d1 == 0.f && d2 > 0.f) || (double)(d2 / d1) > A.ratio);
    }
    const float2 p0 = A.kp[q_lo + q], p1 = A.kp[t_lo + bi];
    const double x0 = p0.x, y0 = p0.y, x1 = p1.x, y1 = p1.y;
    const bool border = x0 >= A.x_lo && y0 >= A.y_lo && x0 <= A.x_hi && y0 <= A.y_hi && x1 >= A.x_lo && y1 >= A.y_lo &&
                        x1 <= A.x_hi && y1 <= A.y_hi;
    const bool skew = fabs(y1 - y0) < A.skew_y && fabs(x1 - x0) < A.skew_x;
    filters_ok = ratio_ok && border && skew;
    A.pass[o] = (uint8_t)((ratio_ok ? PASS_RATIO : 0) | (filters_ok ? PASS_FILTERS : 0));
    if (filters_ok) atomicMin(A.vote + (size_t)A.tptr[t.pair] + bi, vote_key(best, q));
  }
  // the stage counts of the pair: one atomic per wavefront and stage (integer sums: any order gives the same)
  const int n_ratio = __popcll(__ballot(ratio_ok)), n_filters = __popcll(__ballot(filters_ok));
  const int n_active = __popcll(__ballot(active));
  if ((threadIdx.x & (WAVE - 1)) == 0 && n_active) {
    atomicAdd(A.counts + 4 * (size_t)t.pair, n_active);
    if (n_ratio) atomicAdd(A.counts + 4 * (size_t)t.pair + 1, n_ratio);
    if (n_filters) atomicAdd(A.counts + 4 * (size_t)t.pair + 2, n_filters);
  }
}

// query q of pair p (its slot o of the per-query arrays) passed the filters and won the vote at its train keypoint
__device__ inline bool survives(const MatchArgs& A, int32_t p, int32_t q, size_t o) {
  if (!(A.pass[o] & PASS_FILTERS)) return false;
  return A.vote[(size_t)A.tptr[p] + A.best_idx[o]] == vote_key(A.best_d2[o], q);
}

// exclusive prefix sum of v over the workgroup's lanes; total = the sum.  s holds WG ints.
__device__ inline int block_excl_scan(int v, int* s, int& total) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < WG; off <<= 1) {
    const int x = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += x;
    __syncthreads();
  }
  const int incl = s[tid];
  total = s[WG - 1];
  __syncthreads();  // s may be written again
  return incl - v;
}

__global__ __launch_bounds__(WG) void k_match_count(MatchArgs A) {
  __shared__ int s[WG];
  const int32_t p = blockIdx.x;
  const int32_t lo = A.qptr[p], nq = A.qptr[p + 1] - lo;
  int mine = 0;
  for (int32_t q = threadIdx.x; q < nq; q += WG) mine += survives(A, p, q, (size_t)lo + q);
  int total;
  block_excl_scan(mine, s, total);
  if (threadIdx.x == 0) A.counts[4 * (size_t)p + 3] = total;
}

__global__ __launch_bounds__(WG) void k_match_scan(MatchArgs A) {
  __shared__ int s[WG];
  int run = 0;
  for (int32_t p0 = 0; p0 < A.n_pairs; p0 += WG) {
    const int32_t p = p0 + (int32_t)threadIdx.x;
    const int v = p < A.n_pairs ? A.counts[4 * (size_t)p + 3] : 0;
    int total;
    const int ex = block_excl_scan(v, s, total);
    if (p < A.n_pairs) A.match_ptr[p] = run + ex;
    run += total;
  }
  if (threadIdx.x == 0) A.match_ptr[A.n_pairs] = run;
}

__global__ __launch_bounds__(WG) void k_match_compact(MatchArgs A) {
  __shared__ int s[WG];
  const int32_t p = blockIdx.x;
  const int32_t lo = A.qptr[p], nq = A.qptr[p + 1] - lo;
  if (nq == 0) return;
  const int32_t f0 = A.pairs[2 * p], f1 = A.pairs[2 * p + 1];
  const int32_t q_lo = A.kp_ptr[f0], t_lo = A.kp_ptr[f1];
  int run = A.match_ptr[p];
  for (int32_t q0 = 0; q0 < nq; q0 += WG) {
    const int32_t q = q0 + (int32_t)threadIdx.x;
    const size_t o = (size_t)lo + q;
    const bool keep = q < nq && survives(A, p, q, o);
    int total;
    const int ex = block_excl_scan(keep ? 1 : 0, s, total);
    if (keep) {
      const size_t m = (size_t)(run + ex);
      const int32_t tr = A.best_idx[o];
      const float2 p0 = A.kp[q_lo + q], p1 = A.kp[t_lo + tr];
      A.m_query[m] = q;
      A.m_train[m] = tr;
      A.m_dist[m] = sqrt_rn(A.best_d2[o]);
      A.m_uv0[2 * m] = p0.x; A.m_uv0[2 * m + 1] = p0.y;
      A.m_uv1[2 * m] = p1.x; A.m_uv1[2 * m + 1] = p1.y;
    }
    run += total;
  }
}

// The K-nearest regression of cv::ml::KNearest for one pixel per lane on n_obs >= 1 observations, all lanes of the
// workgroup on the same observations (every lane calls; `active` says whether it has a pixel).  Returns the depth;
// nb (when given: K entries of the lane) receives the chosen observations in (distance, index) order, -1 padded.
__device__ inline float knn_depth(float u, float v, bool active, const float2* ouv, const float* od, int32_t n_obs,
                                  int K, float2* stage, int32_t* nb) {
  // Contraction is off for the distance below.  (__fmul_rn and __fadd_rn would not do: here they are the plain operators
  // inside inline functions, and the compiler fused them into fl(dx dx + fl(dy dy)), which orders near ties otherwise.)
#pragma clang fp contract(off)
  float dk[MAX_K];
  int32_t ik[MAX_K];
#pragma unroll
  for (int j = 0; j < MAX_K; ++j) { dk[j] = INFINITY; ik[j] = -1; }
  int cnt = 0;
  float worst = INFINITY;  // dk[K - 1] once the list is full
  for (int32_t c0 = 0; c0 < n_obs; c0 += OBS_CHUNK) {
    const int32_t m = min(OBS_CHUNK, n_obs - c0);
    __syncthreads();
    for (int32_t i = threadIdx.x; i < m; i += WG) stage[i] = ouv[c0 + i];
    __syncthreads();
    if (!active) continue;
    for (int32_t i = 0; i < m; ++i) {
      const float2 o = stage[i];
      // fl(fl(dx dx) + fl(dy dy)): no fused multiply-add, so a restatement gets the same bits
      const float dx = o.x - u, dy = o.y - v;
      const float xx = dx * dx, yy = dy * dy;
      const float d = xx + yy;
      if (cnt < K || d < worst) {  // (strict: on equal distance the earlier, lower index stays)
        const int pos = cnt < K ? cnt : K - 1;
        if (cnt < K) ++cnt;
#pragma unroll
        for (int j = 0; j < MAX_K; ++j)
          if (j == pos) { dk[j] = d; ik[j] = c0 + i; }
#pragma unroll
        for (int j = MAX_K - 1; j >= 1; --j)
          if (j <= pos && dk[j] < dk[j - 1]) {
            const float td = dk[j]; dk[j] = dk[j - 1]; dk[j - 1] = td;
            const int32_t ti = ik[j]; ik[j] = ik[j - 1]; ik[j - 1] = ti;
          }
        if (cnt == K) {
#pragma unroll
          for (int j = 0; j < MAX_K; ++j)
            if (j == K - 1) worst = dk[j];
        }
      }
    }
  }
  if (!active) return 0.f;
  double sum = 0;
#pragma unroll
  for (int j = 0; j < MAX_K; ++j)
    if (j < cnt) sum += (double)od[ik[j]];
  if (nb) {
#pragma unroll
    for (int j = 0; j < MAX_K; ++j)
      if (j < K) nb[j] = ik[j];
  }
  return (float)(sum / (double)cnt);
}

__global__ __launch_bounds__(WG) void k_match_depth(MatchArgs A) {
  __shared__ float2 stage[OBS_CHUNK];
  const Tile t = A.tiles[blockIdx.x];
  const int side = blockIdx.y;
  const int32_t m_lo = A.match_ptr[t.pair], nm = A.match_ptr[t.pair + 1] - m_lo;
  if (t.q0 >= nm) return;  // (the whole workgroup: the table is the queries', a pair has no more matches than those)
  const int32_t frame = A.pairs[2 * t.pair + side];
  const int32_t o_lo = A.obs_ptr[frame], n_obs = A.obs_ptr[frame + 1] - o_lo;
  const int32_t i = t.q0 + (int32_t)threadIdx.x;
  const bool active = i < nm;
  const size_t m = (size_t)m_lo + (active ? i : nm - 1);
  const int32_t key = side ? A.m_train[m] : A.m_query[m];
  const float2 px = A.kp[A.kp_ptr[frame] + key];
  const float depth = knn_depth(px.x, px.y, active, A.obs_uv + o_lo, A.obs_depth + o_lo, n_obs, A.K, stage, nullptr);
  if (!active) return;
  const double z = depth;
  if (side) {
    A.m_depth1[m] = z;
  } else {
    A.m_depth0[m] = z;
    A.m_pts[3 * m] = z * (((double)px.x - A.cx) / A.f);
    A.m_pts[3 * m + 1] = z * (((double)px.y - A.cy) / A.f);
    A.m_pts[3 * m + 2] = z;
  }
}

__global__ __launch_bounds__(WG) void k_match_depth_probe(const float2* ouv, const float* od, int32_t n_obs, int K,
                                                          const float2* uv, int32_t n, double* depth, int32_t* nb) {
  __shared__ float2 stage[OBS_CHUNK];
  const int32_t i = (int32_t)(blockIdx.x * WG + threadIdx.x);
  const bool active = i < n;
  const float2 px = uv[active ? i : n - 1];
  const float z = knn_depth(px.x, px.y, active, ouv, od, n_obs, K, stage, active ? nb + (size_t)K * i : nullptr);
  if (active) depth[i] = z;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Batch : sim3opt::BatchHandle {
  sim3opt_match_batch_options opt;
  // the frames and pairs, as set
  std::vector<int32_t> kp_ptr, obs_ptr, pairs;
  std::vector<float> kp, desc, obs_uv, obs_depth;
  double f = 0, cx = 0, cy = 0;
  int32_t width = 0, height = 0;
  Plan plan;
  // the last solve
  std::vector<int32_t> match_ptr, counts, m_query, m_train;
  std::vector<float> m_dist;
  std::vector<double> m_uv0, m_uv1, m_depth0, m_depth1, m_pts;
  // device
  sim3opt::DevArena frame_mem, pair_mem;  // the blocks of devf; of devp
  sim3opt_fstore::SnapshotRef snap;       // set_frames_from: kp_ptr / kp / desc of devf are the snapshot's, not frame_mem's
  struct DevFrames {  // the frames, as set
    float *kp, *desc, *obs_uv, *obs_depth;
    int32_t *kp_ptr, *obs_ptr;
    bool up;
  } devf{};
  struct DevPairs {  // the pairs' plan and the blocks of a solve
    int32_t *pairs, *qptr, *tptr;
    Tile* tiles;
    int32_t *best_idx, *second_idx, *counts, *match_ptr;
    float *best_d2, *second_d2, *m_dist;
    uint8_t* pass;
    unsigned long long* vote;
    int32_t *m_query, *m_train;
    double* m_dbl;  // uv0 (2), uv1 (2), depth0, depth1, points0 (3): nine blocks of Q doubles
    bool up;
  } devp{};

  ~Batch() { release(); }
  int32_t n_frames() const { return kp_ptr.empty() ? 0 : (int32_t)kp_ptr.size() - 1; }
  int32_t n_pairs() const { return (int32_t)(pairs.size() / 2); }
  size_t Q() const { return plan.qptr.empty() ? 0 : (size_t)plan.qptr.back(); }
  size_t T() const { return plan.tptr.empty() ? 0 : (size_t)plan.tptr.back(); }

  // the pairs' blocks alone: the frames stay on the device when only the candidate list changes
  void release_pairs() {
    wait();
    pair_mem.release();
    devp = DevPairs{};
  }

  void release() {
    close_stream(pair_mem, frame_mem);
    devp = DevPairs{};
    devf = DevFrames{};
  }

  // the device and the frames on it (need_pairs: and the pairs, their plan and the blocks of a solve)
  int ensure_device(const char* who, bool need_pairs) {
    if (n_frames() < 1) { err = std::string(who) + ": no frames set"; return SIM3OPT_ERR_STATE; }
    if (need_pairs && n_pairs() < 1) { err = std::string(who) + ": no pairs set"; return SIM3OPT_ERR_STATE; }
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    if (snap)
      if (int rc = sim3opt_fstore::check_snapshot_device(*snap, who, opt.device, err)) return rc;
    if (!devf.up) {
      release();
      if (int rc = open_stream()) return rc;
      if (snap) {  // read in place: nothing of the keypoints is uploaded
        devf.kp_ptr = snap->d_kp_ptr; devf.kp = snap->d_kp; devf.desc = snap->d_desc;
        HIPCHK(frame_mem.upload(devf.obs_ptr, obs_ptr, stream, nullptr));
      } else {
        HIPCHK(frame_mem.upload(devf.kp_ptr, kp_ptr, stream, nullptr));
        HIPCHK(frame_mem.upload(devf.obs_ptr, obs_ptr, stream, nullptr));
        HIPCHK(frame_mem.upload(devf.kp, kp, stream, nullptr));
        HIPCHK(frame_mem.upload(devf.desc, desc, stream, nullptr));
      }
      HIPCHK(frame_mem.upload(devf.obs_uv, obs_uv, stream, nullptr));
      HIPCHK(frame_mem.upload(devf.obs_depth, obs_depth, stream, nullptr));
      HIPCHK(hipStreamSynchronize(stream));
      devf.up = true;
    }
    if (need_pairs && !devp.up) {
      release_pairs();
      const size_t N = (size_t)n_pairs(), q = Q();
      HIPCHK(pair_mem.upload(devp.pairs, pairs, stream, nullptr));
      HIPCHK(pair_mem.upload(devp.qptr, plan.qptr, stream, nullptr));
      HIPCHK(pair_mem.upload(devp.tptr, plan.tptr, stream, nullptr));
      HIPCHK(pair_mem.upload(devp.tiles, plan.tiles, stream, nullptr));
      HIPCHK(pair_mem.raw(devp.best_idx, q));
      HIPCHK(pair_mem.raw(devp.second_idx, q));
      HIPCHK(pair_mem.raw(devp.best_d2, q));
      HIPCHK(pair_mem.raw(devp.second_d2, q));
      HIPCHK(pair_mem.raw(devp.pass, q));
      HIPCHK(pair_mem.raw(devp.vote, T()));
      HIPCHK(pair_mem.raw(devp.counts, 4 * N));
      HIPCHK(pair_mem.raw(devp.match_ptr, N + 1));
      HIPCHK(pair_mem.raw(devp.m_query, q));
      HIPCHK(pair_mem.raw(devp.m_train, q));
      HIPCHK(pair_mem.raw(devp.m_dist, q));
      HIPCHK(pair_mem.raw(devp.m_dbl, 9 * q));
      HIPCHK(hipStreamSynchronize(stream));
      devp.up = true;
    }
    return SIM3OPT_OK;
  }

  MatchArgs args() const {
    MatchArgs A{};
    const size_t q = Q();
    A.kp = reinterpret_cast<const float2*>(devf.kp); A.desc = devf.desc;
    A.obs_uv = reinterpret_cast<const float2*>(devf.obs_uv); A.obs_depth = devf.obs_depth;
    A.kp_ptr = devf.kp_ptr; A.obs_ptr = devf.obs_ptr;
    A.pairs = devp.pairs; A.qptr = devp.qptr; A.tptr = devp.tptr; A.tiles = devp.tiles;
    A.best_idx = devp.best_idx; A.second_idx = devp.second_idx; A.best_d2 = devp.best_d2; A.second_d2 = devp.second_d2;
    A.pass = devp.pass; A.vote = devp.vote; A.counts = devp.counts; A.match_ptr = devp.match_ptr;
    A.m_query = devp.m_query; A.m_train = devp.m_train; A.m_dist = devp.m_dist;
    if (devp.m_dbl) {
      A.m_uv0 = devp.m_dbl; A.m_uv1 = devp.m_dbl + 2 * q; A.m_depth0 = devp.m_dbl + 4 * q; A.m_depth1 = devp.m_dbl + 5 * q;
      A.m_pts = devp.m_dbl + 6 * q;
    }
    A.ratio = opt.ratio; A.use_ratio = opt.ratio > 0;
    A.x_lo = opt.border_ratio * width; A.x_hi = (1 - opt.border_ratio) * width;
    A.y_lo = opt.border_ratio * height; A.y_hi = (1 - opt.border_ratio) * height;
    A.skew_x = opt.skew_x * width; A.skew_y = opt.skew_y * height;
    A.f = f; A.cx = cx; A.cy = cy;
    A.n_pairs = n_pairs(); A.K = opt.knn_k;
    return A;
  }

  int solve() {
    err.clear();
    const int rc = ensure_device("match_batch_solve", true);
    if (rc != SIM3OPT_OK) return rc;
    const size_t N = (size_t)n_pairs(), n_tiles = plan.tiles.size();
    const MatchArgs A = args();
    HIPCHK(hipMemsetAsync(devp.vote, 0xFF, sizeof(unsigned long long) * std::max<size_t>(T(), 1), stream));
    HIPCHK(hipMemsetAsync(devp.counts, 0, sizeof(int32_t) * 4 * N, stream));
    if (n_tiles) hipLaunchKernelGGL(k_match_nn, dim3((unsigned)n_tiles), dim3(WG), 0, stream, A);
    hipLaunchKernelGGL(k_match_count, dim3((unsigned)N), dim3(WG), 0, stream, A);
    hipLaunchKernelGGL(k_match_scan, dim3(1), dim3(WG), 0, stream, A);
    hipLaunchKernelGGL(k_match_compact, dim3((unsigned)N), dim3(WG), 0, stream, A);
    if (n_tiles) hipLaunchKernelGGL(k_match_depth, dim3((unsigned)n_tiles, 2), dim3(WG), 0, stream, A);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> mp, cn;
    HIPCHK(sim3opt::read_back(mp, devp.match_ptr, N + 1, stream));
    HIPCHK(sim3opt::read_back(cn, devp.counts, 4 * N, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const size_t M = (size_t)mp[N];
    if (M > Q()) { err = "match_batch_solve: internal error (more matches than queries)"; return SIM3OPT_ERR_HIP; }
    std::vector<int32_t> mq, mt;
    std::vector<float> md;
    std::vector<double> u0, u1, z0, z1, pt;
    HIPCHK(sim3opt::read_back(mq, A.m_query, M, stream));
    HIPCHK(sim3opt::read_back(mt, A.m_train, M, stream));
    HIPCHK(sim3opt::read_back(md, A.m_dist, M, stream));
    HIPCHK(sim3opt::read_back(u0, A.m_uv0, 2 * M, stream));
    HIPCHK(sim3opt::read_back(u1, A.m_uv1, 2 * M, stream));
    HIPCHK(sim3opt::read_back(z0, A.m_depth0, M, stream));
    HIPCHK(sim3opt::read_back(z1, A.m_depth1, M, stream));
    HIPCHK(sim3opt::read_back(pt, A.m_pts, 3 * M, stream));
    if (M) HIPCHK(hipStreamSynchronize(stream));  // (no match: nothing was enqueued)
    match_ptr.swap(mp); counts.swap(cn); m_query.swap(mq); m_train.swap(mt); m_dist.swap(md);
    m_uv0.swap(u0); m_uv1.swap(u1); m_depth0.swap(z0); m_depth1.swap(z1); m_pts.swap(pt);
    have_run = true;
    int ok = 0;
    for (size_t k = 0; k < N; ++k) ok += plan.status[k] == SIM3OPT_MATCH_OK;
    return ok;
  }

  int debug_nn(int32_t pair, int32_t* best_idx, float* best_d2, int32_t* second_idx, float* second_d2) {
    err.clear();
    if (!have_run) { err = "match_batch_debug_nn: no solve yet"; return SIM3OPT_ERR_STATE; }
    if (!devp.up) {  // (options.device changed: the getters still hold the last results, the device holds nothing)
      err = "match_batch_debug_nn: the device blocks of the last solve were released; solve again";
      return SIM3OPT_ERR_STATE;
    }
    if (pair < 0 || pair >= n_pairs()) { err = "match_batch_debug_nn: no such pair"; return SIM3OPT_ERR_ARG; }
    if (plan.status[pair] != SIM3OPT_MATCH_OK) {
      err = "match_batch_debug_nn: nothing was computed for a pair of status " + std::to_string(plan.status[pair]);
      return SIM3OPT_ERR_STATE;
    }
    const size_t lo = (size_t)plan.qptr[pair], n = (size_t)plan.qptr[pair + 1] - lo;
    std::vector<int32_t> bi, si;
    std::vector<float> bd, sd;
    HIPCHK(sim3opt::read_back(bi, devp.best_idx + lo, n, stream));
    HIPCHK(sim3opt::read_back(si, devp.second_idx + lo, n, stream));
    HIPCHK(sim3opt::read_back(bd, devp.best_d2 + lo, n, stream));
    HIPCHK(sim3opt::read_back(sd, devp.second_d2 + lo, n, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (best_idx) std::memcpy(best_idx, bi.data(), sizeof(int32_t) * n);
    if (second_idx) std::memcpy(second_idx, si.data(), sizeof(int32_t) * n);
    if (best_d2) std::memcpy(best_d2, bd.data(), sizeof(float) * n);
    if (second_d2) std::memcpy(second_d2, sd.data(), sizeof(float) * n);
    return SIM3OPT_OK;
  }

  int debug_depth(int32_t n, int32_t frame, const float* uv, double* depth, int32_t* neighbours) {
    err.clear();
    if (n_frames() < 1) { err = "match_batch_debug_depth: no frames set"; return SIM3OPT_ERR_STATE; }
    if (frame < 0 || frame >= n_frames()) { err = "match_batch_debug_depth: no such frame"; return SIM3OPT_ERR_ARG; }
    const int32_t o_lo = obs_ptr[frame], n_obs = obs_ptr[frame + 1] - o_lo;
    if (n_obs < 1) { err = "match_batch_debug_depth: the frame has no observation"; return SIM3OPT_ERR_ARG; }
    const int rc = ensure_device("match_batch_debug_depth", false);
    if (rc != SIM3OPT_OK) return rc;
    const size_t K = (size_t)opt.knn_k;
    sim3opt::DevBuf<float> duv;
    sim3opt::DevBuf<double> dz;
    sim3opt::DevBuf<int32_t> dnb;
    HIPCHK(duv.alloc(2 * (size_t)n));
    HIPCHK(dz.alloc((size_t)n));
    HIPCHK(dnb.alloc(K * n));
    HIPCHK(hipMemcpyAsync(duv.get(), uv, sizeof(float) * 2 * n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_match_depth_probe, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, stream,
                       reinterpret_cast<const float2*>(devf.obs_uv) + o_lo, devf.obs_depth + o_lo, n_obs, opt.knn_k,
                       reinterpret_cast<const float2*>(duv.get()), n, dz.get(), dnb.get());
    HIPCHK(hipGetLastError());
    std::vector<double> hz;
    std::vector<int32_t> hn;
    HIPCHK(sim3opt::read_back(hz, dz.get(), (size_t)n, stream));
    HIPCHK(sim3opt::read_back(hn, dnb.get(), K * n, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (depth) std::memcpy(depth, hz.data(), sizeof(double) * n);
    if (neighbours) std::memcpy(neighbours, hn.data(), sizeof(int32_t) * K * n);
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_match

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched descriptor matching")
// ------------------------------------------------------------------------------------------
struct sim3opt_match_batch : sim3opt_match::Batch {};

extern "C" {

void sim3opt_match_batch_options_default(sim3opt_match_batch_options* o) {
  if (!o) return;
  o->ratio = 0.0;            // USE_KNN_MATCH is off in the reference's build
  o->border_ratio = 0.1;     // boundaryRatio
  o->skew_x = 1.0 / 3.0;     // skewThreshX
  o->skew_y = 1.0 / 4.0;     // skewThreshY
  o->knn_k = 6;              // K
  o->device = -1;
}

sim3opt_match_batch* sim3opt_match_batch_create(void) {
  return sim3opt::handle_create<sim3opt_match_batch>(sim3opt_match_batch_options_default);
}

void sim3opt_match_batch_destroy(sim3opt_match_batch* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_match_batch_last_error(const sim3opt_match_batch* b) { return b ? b->err.c_str() : "null batch"; }

int sim3opt_match_batch_set_options(sim3opt_match_batch* b, const sim3opt_match_batch_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  const std::string e = sim3opt_match::validate_options(*o);
  if (!e.empty()) { b->err = "match_batch_set_options: " + e; return SIM3OPT_ERR_ARG; }
  if (o->device != b->opt.device && b->snap) {
    b->err = "match_batch_set_options: the frames are a store's snapshot on its device; options.device cannot change";
    return SIM3OPT_ERR_ARG;
  }
  if (o->device != b->opt.device) b->release();  // the device is chosen at the next solve
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_match_batch_set_frames(sim3opt_match_batch* b, int32_t n_frames, const int32_t* kp_ptr,
                                   const int32_t* obs_ptr, const float* kp, const float* desc, const float* obs_uv,
                                   const float* obs_depth, double focal, double cx, double cy, int32_t image_width,
                                   int32_t image_height) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "match_batch_set_frames", sim3opt::NO_MEMORY, [&]() -> int {
    const std::string e = sim3opt_match::validate_frames(n_frames, kp_ptr, obs_ptr, kp, desc, obs_uv, obs_depth, focal,
                                                         cx, cy, image_width, image_height);
    if (!e.empty()) { b->err = "match_batch_set_frames: " + e; return SIM3OPT_ERR_ARG; }
    const size_t nk = (size_t)kp_ptr[n_frames], no = (size_t)obs_ptr[n_frames];
    std::vector<int32_t> kpp(kp_ptr, kp_ptr + n_frames + 1), obp(obs_ptr, obs_ptr + n_frames + 1);
    std::vector<float> k(kp, kp + 2 * nk), d(desc, desc + sim3opt_match::DESC * nk), ou(obs_uv, obs_uv + 2 * no),
        od(obs_depth, obs_depth + no);
    // nothing failed: the handle changes now
    b->kp_ptr.swap(kpp); b->obs_ptr.swap(obp); b->kp.swap(k); b->desc.swap(d); b->obs_uv.swap(ou); b->obs_depth.swap(od);
    b->f = focal; b->cx = cx; b->cy = cy; b->width = image_width; b->height = image_height;
    b->pairs.clear();
    b->plan = sim3opt_match::Plan();
    b->have_run = false;
    b->devf.up = b->devp.up = false;
    b->snap.reset();
    return SIM3OPT_OK;
  });
}

int sim3opt_match_batch_set_frames_from(sim3opt_match_batch* b, const sim3opt_frames* store, int32_t n_frames,
                                        const int32_t* obs_ptr, const float* obs_uv, const float* obs_depth, double focal,
                                        double cx, double cy, int32_t image_width, int32_t image_height) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "match_batch_set_frames_from", sim3opt::NO_MEMORY, [&]() -> int {
    sim3opt_fstore::SnapshotRef s;
    if (int rc = sim3opt_fstore::take_snapshot(store, "match_batch_set_frames_from", b->opt.device, s, b->err)) return rc;
    std::string e = sim3opt_match::validate_observations(n_frames, obs_ptr, obs_uv, obs_depth, focal, cx, cy, image_width,
                                                         image_height);
    if (e.empty() && n_frames != s->n_frames())
      e = "obs_ptr is of " + std::to_string(n_frames) + " frames, the store holds " + std::to_string(s->n_frames());
    if (!e.empty()) { b->err = "match_batch_set_frames_from: " + e; return SIM3OPT_ERR_ARG; }
    const size_t no = (size_t)obs_ptr[n_frames];
    std::vector<int32_t> kpp(s->kp_ptr), obp(obs_ptr, obs_ptr + n_frames + 1);
    std::vector<float> ou(obs_uv, obs_uv + 2 * no), od(obs_depth, obs_depth + no);
    // nothing failed: the handle changes now
    b->wait();
    b->kp_ptr.swap(kpp); b->obs_ptr.swap(obp); b->obs_uv.swap(ou); b->obs_depth.swap(od);
    std::vector<float>().swap(b->kp); std::vector<float>().swap(b->desc);
    b->f = focal; b->cx = cx; b->cy = cy; b->width = image_width; b->height = image_height;
    b->pairs.clear();
    b->plan = sim3opt_match::Plan();
    b->have_run = false;
    b->devf.up = b->devp.up = false;
    b->snap = std::move(s);
    return SIM3OPT_OK;
  });
}

int sim3opt_match_batch_set_pairs(sim3opt_match_batch* b, int32_t n_pairs, const int32_t* pairs) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (b->n_frames() < 1) { b->err = "match_batch_set_pairs: no frames set"; return SIM3OPT_ERR_STATE; }
  return sim3opt::guarded(b, "match_batch_set_pairs", sim3opt::NO_MEMORY, [&]() -> int {
    std::string e = sim3opt_match::validate_pairs(b->n_frames(), n_pairs, pairs);
    sim3opt_match::Plan plan;
    if (e.empty()) e = sim3opt_match::build_plan(b->kp_ptr.data(), b->obs_ptr.data(), n_pairs, pairs, plan);
    if (!e.empty()) { b->err = "match_batch_set_pairs: " + e; return SIM3OPT_ERR_ARG; }
    std::vector<int32_t> p(pairs, pairs + 2 * (size_t)n_pairs);
    b->pairs.swap(p);
    b->plan = std::move(plan);
    b->have_run = false;
    b->devp.up = false;  // (the frames stay where they are)
    return SIM3OPT_OK;
  });
}

int sim3opt_match_batch_dims(const sim3opt_match_batch* b, int32_t* n_frames, int32_t* n_pairs,
                             int32_t* total_keypoints, int32_t* total_observations, int32_t tiles[4]) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (n_frames) *n_frames = b->n_frames();
  if (n_pairs) *n_pairs = b->n_pairs();
  if (total_keypoints) *total_keypoints = b->kp_ptr.empty() ? 0 : b->kp_ptr.back();
  if (total_observations) *total_observations = b->obs_ptr.empty() ? 0 : b->obs_ptr.back();
  if (tiles) {
    tiles[0] = sim3opt_match::WAVE; tiles[1] = sim3opt_match::QUERY_TILE; tiles[2] = sim3opt_match::TRAIN_TILE;
    tiles[3] = sim3opt_match::OBS_CHUNK;
  }
  return SIM3OPT_OK;
}

int sim3opt_match_batch_solve(sim3opt_match_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "match_batch_solve", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve(); });
}

int sim3opt_match_batch_get_match_ptr(const sim3opt_match_batch* b, int32_t* match_ptr) {
  if (!b || !match_ptr) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  std::memcpy(match_ptr, b->match_ptr.data(), sizeof(int32_t) * b->match_ptr.size());
  return SIM3OPT_OK;
}

int sim3opt_match_batch_get_matches(const sim3opt_match_batch* b, int32_t* query_idx, int32_t* train_idx,
                                    float* distance, double* uv0, double* uv1, double* depth0, double* depth1,
                                    double* points0) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  const size_t M = b->m_query.size();
  if (!M) return SIM3OPT_OK;
  if (query_idx) std::memcpy(query_idx, b->m_query.data(), sizeof(int32_t) * M);
  if (train_idx) std::memcpy(train_idx, b->m_train.data(), sizeof(int32_t) * M);
  if (distance) std::memcpy(distance, b->m_dist.data(), sizeof(float) * M);
  if (uv0) std::memcpy(uv0, b->m_uv0.data(), sizeof(double) * 2 * M);
  if (uv1) std::memcpy(uv1, b->m_uv1.data(), sizeof(double) * 2 * M);
  if (depth0) std::memcpy(depth0, b->m_depth0.data(), sizeof(double) * M);
  if (depth1) std::memcpy(depth1, b->m_depth1.data(), sizeof(double) * M);
  if (points0) std::memcpy(points0, b->m_pts.data(), sizeof(double) * 3 * M);
  return SIM3OPT_OK;
}

int sim3opt_match_batch_get_summary(const sim3opt_match_batch* b, int32_t* status, int32_t* n_nearest,
                                    int32_t* n_after_ratio, int32_t* n_after_filters, int32_t* n_after_unique) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  for (int32_t k = 0; k < b->n_pairs(); ++k) {
    const int32_t* c = b->counts.data() + 4 * (size_t)k;
    if (status) status[k] = b->plan.status[k];
    if (n_nearest) n_nearest[k] = c[0];
    if (n_after_ratio) n_after_ratio[k] = c[1];
    if (n_after_filters) n_after_filters[k] = c[2];
    if (n_after_unique) n_after_unique[k] = c[3];
  }
  return SIM3OPT_OK;
}

int sim3opt_match_batch_debug_nn(sim3opt_match_batch* b, int32_t pair, int32_t* best_idx, float* best_d2,
                                 int32_t* second_idx, float* second_d2) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "match_batch_debug_nn", sim3opt::NO_MEMORY,
                          [&] { return b->debug_nn(pair, best_idx, best_d2, second_idx, second_d2); });
}

int sim3opt_match_batch_debug_depth(sim3opt_match_batch* b, int32_t n, int32_t frame, const float* uv, double* depth,
                                    int32_t* neighbours) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (n < 1 || !uv || (!depth && !neighbours) || !sim3opt::all_finite(uv, 2 * (size_t)n)) {
    b->err = "match_batch_debug_depth: bad argument"; return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "match_batch_debug_depth", sim3opt::NO_MEMORY,
                          [&] { return b->debug_depth(n, frame, uv, depth, neighbours); });
}

}  // extern "C"
