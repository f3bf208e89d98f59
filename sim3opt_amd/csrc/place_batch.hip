// place_batch.hip -- the loop detector's place recognition for a whole sequence of keyframes: the bag-of-words vector
// of every frame, the score of every pair of frames and, per query, DLoopDetector's tests up to the chosen island
// (detector.detectLoop, kittiDetector.h:1663).  include/sim3opt.h ("batched bag-of-words place recognition") holds the
// definition the kernels follow, and says what of it is the reference's and what is recalled from upstream.
//
// A solve is four launches, whatever the number of frames:
//   k_place_words   one lane per descriptor, its 64 floats in registers, descending the tree.  The tree is numbered
//                   breadth first (place_host.hpp), so a node's children are consecutive and the first LDS_NODES nodes
//                   -- the levels every descriptor passes -- have their centres in LDS; deeper nodes are read from
//                   memory by the lane that reached them.  d2 is the definition's: FP32 difference and square, not
//                   fused, 64 double additions in ascending k, so the mapping cannot change a result.
//   k_place_bow     one workgroup per frame.  A lane ranks its descriptor's word among the frame's (the words pass
//                   through LDS BOW_CHUNK at a time) and counts its equals, and scatters (word, count) to its rank: the
//                   words sorted, without a sort whose size would bound the frame.  A prefix scan over the heads of the
//                   runs of positive weight writes the vector by ascending word id; one lane adds the values in that
//                   order; all divide.
//   k_place_score   one workgroup per (query i, SCORE_JB database frames j <= i), a wavefront per database frame at a
//                   time.  The query's words are in LDS (up to SCORE_LDS of them; a longer vector is searched in
//                   memory); a lane looks one entry of the database frame up by bisection, and the wavefront adds the
//                   terms of the common words one after the other in ascending word id.  That order is a function of
//                   the two vectors alone, and the term is symmetric in them, so s(a, b) has one value bit for bit.
//                   No atomics.  The scores fill a triangle in device memory: row i holds j = 0..i.
//   k_place_select  one workgroup per query: up to max_db_results rounds of "the best result after the last one" over
//                   the query's row -- an arg-max under the total order (score descending, j ascending), so lane order
//                   cannot matter -- ending at the first result below alpha * ns; the kept results ordered by j; one
//                   lane forms the islands and adds their scores in ascending j.
// The temporal window is place_host.hpp's, on the read-back (status, first, last).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "frames_host.hpp"
#include "handle_device.hpp"
#include "place_host.hpp"

// the definition's arithmetic is written out operation by operation: nothing is contracted into a fused multiply-add
#pragma clang fp contract(off)

namespace sim3opt_place {

static_assert(WG % WAVE == 0 && SCORE_JB % (WG / WAVE) == 0 && BOW_CHUNK % WG == 0, "tile sizes");

struct PlaceArgs {
  // the vocabulary, breadth first
  const float* centre;
  const int32_t *first_child, *n_child, *node_word;
  const double* word_weight;
  int32_t n_nodes, depth;
  // the frames
  const float* desc;
  const int32_t* kp_ptr;
  int32_t n_frames, n_desc;
  // per descriptor: its word; the frame's words sorted, with their counts; the vectors (room for one entry each)
  int32_t *word, *sorted_word, *sorted_cnt, *bow_word;
  double* bow_val;
  int32_t* bow_n;  // per frame: the entries of its vector
  double* tri;     // s(i, j) at i (i + 1) / 2 + j, j <= i
  // per query
  int32_t *q_status, *q_match, *q_island;
  double *q_score, *q_ns;
  // the diagnostics of one query (k_place_select with one workgroup): query < 0 in a solve
  int32_t query;
  int32_t *dbg_count, *dbg_kept_j, *dbg_island;
  double *dbg_kept_score, *dbg_island_score;
  // options
  double alpha, min_nss;
  int32_t use_nss, dislocal, max_db, gap, min_group, accumulate;
};

__device__ inline size_t tri_at(int32_t i, int32_t j) { return (size_t)i * ((size_t)i + 1) / 2 + (size_t)j; }

// FSurf64::distance: b is a centre in LDS or in memory
__device__ inline double d2_of(const float (&a)[DESC], const float* b) {
  const float4* b4 = reinterpret_cast<const float4*>(b);
  double acc = 0;
#pragma unroll
  for (int k = 0; k < DESC / 4; ++k) {
    const float4 v = b4[k];
    const float d0 = a[4 * k] - v.x, d1 = a[4 * k + 1] - v.y, d2 = a[4 * k + 2] - v.z, d3 = a[4 * k + 3] - v.w;
    const float s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2, s3 = d3 * d3;
    acc += (double)s0; acc += (double)s1; acc += (double)s2; acc += (double)s3;
  }
  return acc;
}

// the centres of the first LDS_NODES nodes; every lane of the workgroup calls
__device__ inline void stage_top(const PlaceArgs& A, float* top) {
  const int32_t m = min(A.n_nodes, LDS_NODES) * (DESC / 4);
  for (int32_t i = threadIdx.x; i < m; i += WG)
    reinterpret_cast<float4*>(top)[i] = reinterpret_cast<const float4*>(A.centre)[i];
  __syncthreads();
}

// the word of descriptor a; path (when given: A.depth entries) receives the winning d2 of every level, -1 past the leaf
__device__ inline int32_t descend(const PlaceArgs& A, const float* top, const float (&a)[DESC], double* path) {
  int32_t node = 0, level = 0;
  for (int32_t nc = A.n_child[0]; nc > 0; nc = A.n_child[node]) {
    const int32_t c0 = A.first_child[node];
    double best = 0;
    int32_t bc = -1;
    for (int32_t c = c0; c < c0 + nc; ++c) {
      const double d = c < LDS_NODES ? d2_of(a, top + (size_t)c * DESC) : d2_of(a, A.centre + (size_t)c * DESC);
      if (bc < 0 || d < best) { best = d; bc = c; }  // (strict: on equal d2 the lower child stays)
    }
    if (path && level < A.depth) path[level] = best;
    ++level;
    node = bc;
  }
  if (path)
    for (; level < A.depth; ++level) path[level] = -1.0;
  return A.node_word[node];
}

__device__ inline void load_descriptor(const float* src, float (&a)[DESC]) {
  const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
  for (int k = 0; k < DESC / 4; ++k) {
    const float4 v = s4[k];
    a[4 * k] = v.x; a[4 * k + 1] = v.y; a[4 * k + 2] = v.z; a[4 * k + 3] = v.w;
  }
}

__global__ __launch_bounds__(WG) void k_place_words(PlaceArgs A) {
  __shared__ __attribute__((aligned(16))) float top[LDS_NODES * DESC];
  stage_top(A, top);
  const int32_t d = (int32_t)(blockIdx.x * WG + threadIdx.x);
  if (d >= A.n_desc) return;
  float a[DESC];
  load_descriptor(A.desc + (size_t)d * DESC, a);
  A.word[d] = descend(A, top, a, nullptr);
}

__global__ __launch_bounds__(WG) void k_place_words_probe(PlaceArgs A, const float* desc, int32_t n, int32_t* word,
                                                          double* path) {
  __shared__ __attribute__((aligned(16))) float top[LDS_NODES * DESC];
  stage_top(A, top);
  const int32_t d = (int32_t)(blockIdx.x * WG + threadIdx.x);
  if (d >= n) return;
  float a[DESC];
  load_descriptor(desc + (size_t)d * DESC, a);
  word[d] = descend(A, top, a, path + (size_t)d * A.depth);
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

__global__ __launch_bounds__(WG) void k_place_bow(PlaceArgs A) {
  __shared__ int32_t sw[BOW_CHUNK];
  __shared__ int s[WG];
  __shared__ double sv[WG];
  __shared__ double s_sum;
  const int32_t f = blockIdx.x, tid = threadIdx.x;
  const int32_t lo = A.kp_ptr[f], n = A.kp_ptr[f + 1] - lo;
  // the frame's words sorted: (word, its count) at the rank of every descriptor
  for (int32_t t0 = 0; t0 < n; t0 += WG) {
    const int32_t t = t0 + tid;
    const bool active = t < n;
    const int32_t wt = active ? A.word[lo + t] : 0;
    int32_t rank = 0, cnt = 0;
    for (int32_t u0 = 0; u0 < n; u0 += BOW_CHUNK) {
      const int32_t m = min(BOW_CHUNK, n - u0);
      __syncthreads();  // the chunk before is read
      for (int32_t i = tid; i < m; i += WG) sw[i] = A.word[lo + u0 + i];
      __syncthreads();
      if (active)
        for (int32_t i = 0; i < m; ++i) {
          const int32_t wu = sw[i];
          rank += (wu < wt) || (wu == wt && u0 + i < t);
          cnt += wu == wt;
        }
    }
    if (active) { A.sorted_word[lo + rank] = wt; A.sorted_cnt[lo + rank] = cnt; }
  }
  __threadfence_block();  // the workgroup reads below what its lanes wrote to memory
  __syncthreads();
  // the heads of the runs of positive weight, in order: the vector by ascending word id
  int32_t run = 0;
  for (int32_t p0 = 0; p0 < n; p0 += WG) {
    const int32_t p = p0 + tid;
    bool head = false;
    int32_t w = 0;
    double ww = 0;
    if (p < n) {
      w = A.sorted_word[lo + p];
      ww = A.word_weight[w];
      head = (p == 0 || A.sorted_word[lo + p - 1] != w) && ww > 0;
    }
    int total;
    const int ex = block_excl_scan(head ? 1 : 0, s, total);
    if (head) {
      A.bow_word[lo + run + ex] = w;
      A.bow_val[lo + run + ex] = A.accumulate ? (double)A.sorted_cnt[lo + p] * ww : ww;
    }
    run += total;
  }
  __threadfence_block();
  __syncthreads();
  // the L1 norm: the values added in ascending word id by one lane, WG of them staged at a time
  double sum = 0;
  for (int32_t e0 = 0; e0 < run; e0 += WG) {
    __syncthreads();
    if (e0 + tid < run) sv[tid] = A.bow_val[lo + e0 + tid];
    __syncthreads();
    if (tid == 0) {
      const int32_t m = min(WG, run - e0);
      for (int32_t i = 0; i < m; ++i) sum += sv[i];
    }
  }
  if (tid == 0) { s_sum = sum; A.bow_n[f] = run; }
  __syncthreads();
  sum = s_sum;
  for (int32_t e = tid; e < run; e += WG) A.bow_val[lo + e] = A.bow_val[lo + e] / sum;
}

// the first position of the sorted words w[0..m) that is not below key
__device__ inline int32_t lower_bound(const int32_t* w, int32_t m, int32_t key) {
  int32_t lo = 0, hi = m;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (w[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ inline double read_lane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(WG) void k_place_score(PlaceArgs A) {
  __shared__ int32_t qw[SCORE_LDS];
  const int32_t i = blockIdx.y, jb = (int32_t)blockIdx.x * SCORE_JB;
  if (jb > i) return;  // (the whole workgroup)
  const int32_t lo_i = A.kp_ptr[i], m_i = A.bow_n[i];
  const bool in_lds = m_i <= SCORE_LDS;
  if (in_lds)
    for (int32_t e = threadIdx.x; e < m_i; e += WG) qw[e] = A.bow_word[lo_i + e];
  __syncthreads();
  const int32_t wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int32_t j_end = min(jb + SCORE_JB, i + 1);
  const int32_t* gw = A.bow_word + lo_i;
  for (int32_t j = jb + wave; j < j_end; j += WG / WAVE) {
    const int32_t lo_j = A.kp_ptr[j], m_j = m_i > 0 ? A.bow_n[j] : 0;
    double acc = 0;
    for (int32_t e0 = 0; e0 < m_j; e0 += WAVE) {
      const int32_t e = e0 + lane;
      bool found = false;
      double term = 0;
      if (e < m_j) {
        const int32_t w = A.bow_word[lo_j + e];
        const int32_t pos = in_lds ? lower_bound(qw, m_i, w) : lower_bound(gw, m_i, w);
        if (pos < m_i && (in_lds ? qw[pos] : gw[pos]) == w) {
          found = true;
          const double a = A.bow_val[lo_i + pos], b = A.bow_val[lo_j + e];
          term = fabs(a - b) - (fabs(a) + fabs(b));
        }
      }
      // the common words of these 64 entries, one after the other in ascending word id (the mask is the wavefront's)
      for (unsigned long long mask = __ballot(found); mask; mask &= mask - 1)
        acc += read_lane(term, __ffsll((long long)mask) - 1);
    }
    if (lane == 0) A.tri[tri_at(i, j)] = acc == 0 ? 0.0 : -0.5 * acc;
  }
}

// (s, j) comes before (s2, j2) in the order of the results; j < 0: no result
__device__ inline bool before(double s, int32_t j, double s2, int32_t j2) {
  if (j < 0) return false;
  return j2 < 0 || s > s2 || (s == s2 && j < j2);
}

__global__ __launch_bounds__(WG) void k_place_select(PlaceArgs A) {
  __shared__ int32_t kj[MAX_RESULTS], oj[MAX_RESULTS];
  __shared__ double ks[MAX_RESULTS], os[MAX_RESULTS];
  __shared__ double red_s[WG / WAVE];
  __shared__ int32_t red_j[WG / WAVE];
  const bool dbg = A.query >= 0;
  const int32_t i = dbg ? A.query : (int32_t)blockIdx.x;
  const int32_t tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  int32_t status = SIM3OPT_PLACE_CANDIDATE, match = -1, first = -1, last = -1, n_kept = 0, n_islands = 0;
  double score = 0, ns = 0;
  if (i <= A.dislocal) {
    status = SIM3OPT_PLACE_CLOSE_MATCHES_ONLY;
  } else {
    const double* row = A.tri + tri_at(i, 0);
    const int32_t hi = i - A.dislocal;
    ns = A.use_nss ? row[i - 1] : 1.0;
    const double thr = A.alpha * ns;
    const bool low_nss = A.use_nss && ns < A.min_nss;
    double prev_s = INFINITY;
    int32_t prev_j = -1;
    bool any = false;
    for (int32_t r = 0; r < A.max_db; ++r) {
      // the best result after (prev_s, prev_j)
      double bs = 0;
      int32_t bj = -1;
      for (int32_t j = tid; j <= hi; j += WG) {
        const double s = row[j];
        if (s > 0 && (s < prev_s || (s == prev_s && j > prev_j)) && before(s, j, bs, bj)) { bs = s; bj = j; }
      }
      for (int off = WAVE / 2; off; off >>= 1) {
        const double s2 = __shfl_xor(bs, off);
        const int32_t j2 = __shfl_xor(bj, off);
        if (before(s2, j2, bs, bj)) { bs = s2; bj = j2; }
      }
      __syncthreads();  // the round before is read
      if (lane == 0) { red_s[wave] = bs; red_j[wave] = bj; }
      __syncthreads();
      bs = red_s[0]; bj = red_j[0];
      for (int w = 1; w < WG / WAVE; ++w)
        if (before(red_s[w], red_j[w], bs, bj)) { bs = red_s[w]; bj = red_j[w]; }
      if (bj < 0) break;  // (uniform: every lane holds the same best)
      any = true;
      if (low_nss || !(bs >= thr)) break;  // the results come by descending score: none after this one passes
      if (tid == 0) { kj[n_kept] = bj; ks[n_kept] = bs; }
      ++n_kept;
      prev_s = bs; prev_j = bj;
    }
    __syncthreads();
    if (!any) {
      status = SIM3OPT_PLACE_NO_DB_RESULTS;
      ns = 0;
    } else if (low_nss) {
      status = SIM3OPT_PLACE_LOW_NSS_FACTOR;
    } else if (n_kept == 0) {
      status = SIM3OPT_PLACE_LOW_SCORES;
    } else {
      // the kept results by ascending j (their j differ: the rank is a count)
      for (int32_t e = tid; e < n_kept; e += WG) {
        int32_t rank = 0;
        for (int32_t u = 0; u < n_kept; ++u) rank += kj[u] < kj[e];
        oj[rank] = kj[e]; os[rank] = ks[e];
      }
      __syncthreads();
      if (tid == 0) {
        double chosen_score = 0;
        int32_t chosen_best = -1;
        double chosen_best_score = 0;
        for (int32_t p = 0; p < n_kept;) {
          const int32_t i_first = oj[p];
          int32_t i_last = i_first, best = i_first, cnt = 1, q = p + 1;
          double sum = os[p], best_s = os[p];
          for (; q < n_kept && oj[q] - i_last < A.gap; ++q) {
            sum += os[q];
            if (os[q] > best_s) { best_s = os[q]; best = oj[q]; }
            i_last = oj[q];
            ++cnt;
          }
          p = q;
          if (cnt < A.min_group) continue;
          if (dbg && A.dbg_island) {
            int32_t* o = A.dbg_island + 4 * n_islands;
            o[0] = i_first; o[1] = i_last; o[2] = best; o[3] = cnt;
            A.dbg_island_score[n_islands] = sum;
          }
          if (n_islands == 0 || sum > chosen_score) {  // (strict: on equal score the island of lower first stays)
            chosen_score = sum; chosen_best = best; chosen_best_score = best_s;
            first = i_first; last = i_last;
          }
          ++n_islands;
        }
        if (n_islands == 0) {
          status = SIM3OPT_PLACE_NO_GROUPS;
          match = kj[0]; score = ks[0];
        } else {
          match = chosen_best; score = chosen_best_score;
        }
      }
    }
  }
  if (dbg) {  // (results were kept only on the way to the islands: oj and os hold them)
    for (int32_t e = tid; e < n_kept; e += WG) { A.dbg_kept_j[e] = oj[e]; A.dbg_kept_score[e] = os[e]; }
    if (tid == 0) { A.dbg_count[0] = n_kept; A.dbg_count[1] = n_islands; }
    return;
  }
  if (tid != 0) return;
  A.q_status[i] = status; A.q_match[i] = match; A.q_score[i] = score; A.q_ns[i] = ns;
  A.q_island[2 * i] = first; A.q_island[2 * i + 1] = last;
}

// the diagnostic's row: s(query, j) for every j, from the triangle
__global__ __launch_bounds__(WG) void k_place_row(const double* tri, int32_t query, int32_t n, double* row) {
  const int32_t j = (int32_t)(blockIdx.x * WG + threadIdx.x);
  if (j < n) row[j] = j <= query ? tri[tri_at(query, j)] : tri[tri_at(j, query)];
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Batch : sim3opt::BatchHandle {
  sim3opt_place_batch_options opt;
  Vocabulary voc;
  std::vector<int32_t> kp_ptr;
  std::vector<float> desc;
  // the last solve
  sim3opt_place_batch_options run_opt;  // the options it ran with (the diagnostics repeat its steps)
  std::vector<int32_t> status, match, n_consistent, island, pairs, bow_ptr, bow_word;
  std::vector<double> score, ns, bow_val;
  // device
  sim3opt::DevArena voc_mem, frame_mem;
  sim3opt_fstore::SnapshotRef snap;  // set_frames_from: kp_ptr / desc of devf are the snapshot's, not frame_mem's
  struct DevVoc {
    float* centre;
    int32_t *first_child, *n_child, *node_word;
    double* word_weight;
    bool up;
  } devv{};
  struct DevFrames {  // the frames and the blocks of a solve
    float* desc;
    int32_t *kp_ptr, *word, *sorted_word, *sorted_cnt, *bow_word, *bow_n;
    double *bow_val, *tri;
    int32_t *q_status, *q_match, *q_island;
    double *q_score, *q_ns;
    bool up, solved;  // solved: tri and the vectors are the last solve's
  } devf{};

  ~Batch() { release(); }
  int32_t n_frames() const { return kp_ptr.empty() ? 0 : (int32_t)kp_ptr.size() - 1; }
  size_t D() const { return kp_ptr.empty() ? 0 : (size_t)kp_ptr.back(); }

  void release_frames() {
    wait();
    frame_mem.release();
    devf = DevFrames{};
  }

  void release() {
    close_stream(frame_mem, voc_mem);
    devf = DevFrames{};
    devv = DevVoc{};
  }

  // the device and the vocabulary on it (need_frames: and the frames with the blocks of a solve)
  int ensure_device(const char* who, bool need_frames) {
    if (voc.n_nodes < 2) { err = std::string(who) + ": no vocabulary set"; return SIM3OPT_ERR_STATE; }
    if (need_frames && n_frames() < 1) { err = std::string(who) + ": no frames set"; return SIM3OPT_ERR_STATE; }
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    if (need_frames && snap)
      if (int rc = sim3opt_fstore::check_snapshot_device(*snap, who, opt.device, err)) return rc;
    if (!stream) {
      release();
      if (int rc = open_stream()) return rc;
    }
    if (!devv.up) {
      wait();
      voc_mem.release();
      devv = DevVoc{};
      HIPCHK(voc_mem.upload(devv.centre, voc.centre, stream, nullptr));
      HIPCHK(voc_mem.upload(devv.first_child, voc.first_child, stream, nullptr));
      HIPCHK(voc_mem.upload(devv.n_child, voc.n_child, stream, nullptr));
      HIPCHK(voc_mem.upload(devv.node_word, voc.node_word, stream, nullptr));
      HIPCHK(voc_mem.upload(devv.word_weight, voc.word_weight, stream, nullptr));
      HIPCHK(hipStreamSynchronize(stream));
      devv.up = true;
    }
    if (need_frames && !devf.up) {
      release_frames();
      const size_t n = (size_t)n_frames(), d = D();
      if (snap) {  // read in place: nothing of the frames is uploaded
        devf.kp_ptr = snap->d_kp_ptr; devf.desc = snap->d_desc;
      } else {
        HIPCHK(frame_mem.upload(devf.kp_ptr, kp_ptr, stream, nullptr));
        HIPCHK(frame_mem.upload(devf.desc, desc, stream, nullptr));
      }
      HIPCHK(frame_mem.raw(devf.word, d));
      HIPCHK(frame_mem.raw(devf.sorted_word, d));
      HIPCHK(frame_mem.raw(devf.sorted_cnt, d));
      HIPCHK(frame_mem.raw(devf.bow_word, d));
      HIPCHK(frame_mem.raw(devf.bow_val, d));
      HIPCHK(frame_mem.raw(devf.bow_n, n));
      HIPCHK(frame_mem.raw(devf.tri, n * (n + 1) / 2));
      HIPCHK(frame_mem.raw(devf.q_status, n));
      HIPCHK(frame_mem.raw(devf.q_match, n));
      HIPCHK(frame_mem.raw(devf.q_island, 2 * n));
      HIPCHK(frame_mem.raw(devf.q_score, n));
      HIPCHK(frame_mem.raw(devf.q_ns, n));
      HIPCHK(hipStreamSynchronize(stream));
      devf.up = true;
    }
    return SIM3OPT_OK;
  }

  PlaceArgs args(const sim3opt_place_batch_options& o) const {
    PlaceArgs A{};
    A.centre = devv.centre; A.first_child = devv.first_child; A.n_child = devv.n_child; A.node_word = devv.node_word;
    A.word_weight = devv.word_weight; A.n_nodes = voc.n_nodes; A.depth = voc.depth;
    A.desc = devf.desc; A.kp_ptr = devf.kp_ptr; A.n_frames = n_frames(); A.n_desc = (int32_t)D();
    A.word = devf.word; A.sorted_word = devf.sorted_word; A.sorted_cnt = devf.sorted_cnt; A.bow_word = devf.bow_word;
    A.bow_val = devf.bow_val; A.bow_n = devf.bow_n; A.tri = devf.tri;
    A.q_status = devf.q_status; A.q_match = devf.q_match; A.q_island = devf.q_island; A.q_score = devf.q_score;
    A.q_ns = devf.q_ns;
    A.query = -1;
    A.alpha = o.alpha; A.min_nss = o.min_nss_factor; A.use_nss = o.use_nss; A.dislocal = o.dislocal;
    A.max_db = o.max_db_results; A.gap = o.max_intragroup_gap; A.min_group = o.min_matches_per_group;
    A.accumulate = o.accumulate;
    return A;
  }

  int solve() {
    err.clear();
    const int rc = ensure_device("place_batch_solve", true);
    if (rc != SIM3OPT_OK) return rc;
    const size_t n = (size_t)n_frames(), d = D();
    const PlaceArgs A = args(opt);
    devf.solved = false;
    if (d) hipLaunchKernelGGL(k_place_words, dim3((unsigned)((d + WG - 1) / WG)), dim3(WG), 0, stream, A);
    hipLaunchKernelGGL(k_place_bow, dim3((unsigned)n), dim3(WG), 0, stream, A);
    hipLaunchKernelGGL(k_place_score, dim3((unsigned)((n + SCORE_JB - 1) / SCORE_JB), (unsigned)n), dim3(WG), 0, stream, A);
    hipLaunchKernelGGL(k_place_select, dim3((unsigned)n), dim3(WG), 0, stream, A);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> st, ma, is, bn, bw;
    std::vector<double> sc, nss, bv;
    HIPCHK(sim3opt::read_back(st, devf.q_status, n, stream));
    HIPCHK(sim3opt::read_back(ma, devf.q_match, n, stream));
    HIPCHK(sim3opt::read_back(is, devf.q_island, 2 * n, stream));
    HIPCHK(sim3opt::read_back(sc, devf.q_score, n, stream));
    HIPCHK(sim3opt::read_back(nss, devf.q_ns, n, stream));
    HIPCHK(sim3opt::read_back(bn, devf.bow_n, n, stream));
    HIPCHK(sim3opt::read_back(bw, devf.bow_word, d, stream));
    HIPCHK(sim3opt::read_back(bv, devf.bow_val, d, stream));
    HIPCHK(hipStreamSynchronize(stream));
    // the vectors, compacted: on the device frame f's starts at kp_ptr[f]
    std::vector<int32_t> bp(n + 1, 0), cw;
    std::vector<double> cv;
    for (size_t f = 0; f < n; ++f) {
      if (bn[f] < 0 || bn[f] > kp_ptr[f + 1] - kp_ptr[f]) {
        err = "place_batch_solve: internal error (a vector longer than its frame)"; return SIM3OPT_ERR_HIP;
      }
      bp[f + 1] = bp[f] + bn[f];
    }
    cw.reserve((size_t)bp[n]); cv.reserve((size_t)bp[n]);
    for (size_t f = 0; f < n; ++f) {
      cw.insert(cw.end(), bw.begin() + kp_ptr[f], bw.begin() + kp_ptr[f] + bn[f]);
      cv.insert(cv.end(), bv.begin() + kp_ptr[f], bv.begin() + kp_ptr[f] + bn[f]);
    }
    // the temporal window, and the candidates' pairs
    std::vector<int32_t> first(n), last(n), nc(n), pr;
    for (size_t f = 0; f < n; ++f) { first[f] = is[2 * f]; last[f] = is[2 * f + 1]; }
    temporal_consistency((int32_t)n, first.data(), last.data(), opt, st.data(), nc.data());
    for (size_t f = 0; f < n; ++f)
      if (st[f] == SIM3OPT_PLACE_CANDIDATE) { pr.push_back((int32_t)f); pr.push_back(ma[f]); }
    status.swap(st); match.swap(ma); island.swap(is); score.swap(sc); ns.swap(nss); n_consistent.swap(nc);
    pairs.swap(pr); bow_ptr.swap(bp); bow_word.swap(cw); bow_val.swap(cv);
    run_opt = opt;
    have_run = true;
    devf.solved = true;
    return (int)(pairs.size() / 2);
  }

  int debug_words(int32_t n, const float* d, int32_t* word, double* path_d2) {
    err.clear();
    const int rc = ensure_device("place_batch_debug_words", false);
    if (rc != SIM3OPT_OK) return rc;
    const size_t depth = (size_t)voc.depth;
    sim3opt::DevBuf<float> dd;
    sim3opt::DevBuf<int32_t> dw;
    sim3opt::DevBuf<double> dp;
    HIPCHK(dd.alloc((size_t)DESC * n));
    HIPCHK(dw.alloc((size_t)n));
    HIPCHK(dp.alloc(depth * n));
    HIPCHK(hipMemcpyAsync(dd.get(), d, sizeof(float) * DESC * n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_place_words_probe, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, stream, args(opt), dd.get(),
                       n, dw.get(), dp.get());
    HIPCHK(hipGetLastError());
    std::vector<int32_t> hw;
    std::vector<double> hp;
    HIPCHK(sim3opt::read_back(hw, dw.get(), (size_t)n, stream));
    HIPCHK(sim3opt::read_back(hp, dp.get(), depth * n, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (word) std::memcpy(word, hw.data(), sizeof(int32_t) * n);
    if (path_d2) std::memcpy(path_d2, hp.data(), sizeof(double) * depth * n);
    return SIM3OPT_OK;
  }

  // what the diagnostics of the last solve need: its blocks still on the device
  int last_solve_on_device(const char* who, int32_t query) {
    err.clear();
    if (!have_run) { err = std::string(who) + ": no solve yet"; return SIM3OPT_ERR_STATE; }
    if (!devf.up || !devf.solved) {  // (options.device changed: the getters still hold the last results)
      err = std::string(who) + ": the device blocks of the last solve were released; solve again";
      return SIM3OPT_ERR_STATE;
    }
    if (query < 0 || query >= n_frames()) { err = std::string(who) + ": no such frame"; return SIM3OPT_ERR_ARG; }
    return SIM3OPT_OK;
  }

  int debug_scores(int32_t query, double* row) {
    if (int rc = last_solve_on_device("place_batch_debug_scores", query)) return rc;
    const size_t n = (size_t)n_frames();
    sim3opt::DevBuf<double> dr;
    HIPCHK(dr.alloc(n));
    hipLaunchKernelGGL(k_place_row, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, stream, devf.tri, query, (int32_t)n,
                       dr.get());
    HIPCHK(hipGetLastError());
    std::vector<double> hr;
    HIPCHK(sim3opt::read_back(hr, dr.get(), n, stream));
    HIPCHK(hipStreamSynchronize(stream));
    std::memcpy(row, hr.data(), sizeof(double) * n);
    return SIM3OPT_OK;
  }

  int debug_islands(int32_t query, int32_t* n_kept, int32_t* kept_j, double* kept_score, int32_t* n_islands,
                    int32_t* isl, double* isl_score) {
    if (int rc = last_solve_on_device("place_batch_debug_islands", query)) return rc;
    const size_t R = (size_t)run_opt.max_db_results;
    sim3opt::DevBuf<int32_t> dc, dj, di;
    sim3opt::DevBuf<double> ds, dis;
    HIPCHK(dc.alloc(2));
    HIPCHK(dj.alloc(R));
    HIPCHK(di.alloc(4 * R));
    HIPCHK(ds.alloc(R));
    HIPCHK(dis.alloc(R));
    PlaceArgs A = args(run_opt);
    A.query = query;
    A.dbg_count = dc.get(); A.dbg_kept_j = dj.get(); A.dbg_island = di.get(); A.dbg_kept_score = ds.get();
    A.dbg_island_score = dis.get();
    hipLaunchKernelGGL(k_place_select, dim3(1), dim3(WG), 0, stream, A);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> hc, hj, hi;
    std::vector<double> hs, his;
    HIPCHK(sim3opt::read_back(hc, dc.get(), 2, stream));
    HIPCHK(sim3opt::read_back(hj, dj.get(), R, stream));
    HIPCHK(sim3opt::read_back(hi, di.get(), 4 * R, stream));
    HIPCHK(sim3opt::read_back(hs, ds.get(), R, stream));
    HIPCHK(sim3opt::read_back(his, dis.get(), R, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (hc[0] < 0 || (size_t)hc[0] > R || hc[1] < 0 || hc[1] > hc[0]) {
      err = "place_batch_debug_islands: internal error (more results than max_db_results)"; return SIM3OPT_ERR_HIP;
    }
    const size_t nk = (size_t)hc[0], ni = (size_t)hc[1];
    if (n_kept) *n_kept = hc[0];
    if (n_islands) *n_islands = hc[1];
    if (kept_j) std::memcpy(kept_j, hj.data(), sizeof(int32_t) * nk);
    if (kept_score) std::memcpy(kept_score, hs.data(), sizeof(double) * nk);
    if (isl) std::memcpy(isl, hi.data(), sizeof(int32_t) * 4 * ni);
    if (isl_score) std::memcpy(isl_score, his.data(), sizeof(double) * ni);
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_place

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched bag-of-words place recognition")
// ------------------------------------------------------------------------------------------
struct sim3opt_place_batch : sim3opt_place::Batch {};

extern "C" {

void sim3opt_place_batch_options_default(sim3opt_place_batch_options* o) {
  if (!o) return;
  o->alpha = 0.3;                        // kittiDetector.h:1549-1564
  o->min_nss_factor = 0.005;             // [upstream recall]
  o->use_nss = 1;                        // :1549-1564
  o->k = 3;                              // :1549-1564
  o->dislocal = 20;                      // [upstream recall], as every default below
  o->max_db_results = 50;
  o->max_intragroup_gap = 3;
  o->min_matches_per_group = 1;
  o->max_distance_between_queries = 2;
  o->max_distance_between_groups = 3;
  o->accumulate = 1;
  o->device = -1;
}

sim3opt_place_batch* sim3opt_place_batch_create(void) {
  return sim3opt::handle_create<sim3opt_place_batch>(sim3opt_place_batch_options_default);
}

void sim3opt_place_batch_destroy(sim3opt_place_batch* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_place_batch_last_error(const sim3opt_place_batch* b) { return b ? b->err.c_str() : "null batch"; }

int sim3opt_place_batch_set_options(sim3opt_place_batch* b, const sim3opt_place_batch_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  const std::string e = sim3opt_place::validate_options(*o);
  if (!e.empty()) { b->err = "place_batch_set_options: " + e; return SIM3OPT_ERR_ARG; }
  if (o->device != b->opt.device && b->snap) {
    b->err = "place_batch_set_options: the frames are a store's snapshot on its device; options.device cannot change";
    return SIM3OPT_ERR_ARG;
  }
  if (o->device != b->opt.device) b->release();  // the device is chosen at the next solve
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_place_batch_set_vocabulary(sim3opt_place_batch* b, int32_t n_nodes, const int32_t* parent,
                                       const float* centre, const double* weight, const int32_t* word_id) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "place_batch_set_vocabulary", sim3opt::NO_MEMORY, [&]() -> int {
    sim3opt_place::Vocabulary V;
    const std::string e = sim3opt_place::build_vocabulary(n_nodes, parent, centre, weight, word_id, V);
    if (!e.empty()) { b->err = "place_batch_set_vocabulary: " + e; return SIM3OPT_ERR_ARG; }
    // nothing failed: the handle changes now
    b->voc = std::move(V);
    b->have_run = false;
    b->devv.up = false;
    b->devf.solved = false;
    return SIM3OPT_OK;
  });
}

int sim3opt_place_batch_set_frames(sim3opt_place_batch* b, int32_t n_frames, const int32_t* kp_ptr, const float* desc) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "place_batch_set_frames", sim3opt::NO_MEMORY, [&]() -> int {
    const std::string e = sim3opt_place::validate_frames(n_frames, kp_ptr, desc);
    if (!e.empty()) { b->err = "place_batch_set_frames: " + e; return SIM3OPT_ERR_ARG; }
    std::vector<int32_t> kpp(kp_ptr, kp_ptr + n_frames + 1);
    std::vector<float> d(desc, desc + (size_t)sim3opt_place::DESC * (size_t)kp_ptr[n_frames]);
    b->kp_ptr.swap(kpp); b->desc.swap(d);
    b->have_run = false;
    b->devf.up = b->devf.solved = false;  // (the vocabulary stays where it is)
    b->snap.reset();
    return SIM3OPT_OK;
  });
}

int sim3opt_place_batch_set_frames_from(sim3opt_place_batch* b, const sim3opt_frames* store) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "place_batch_set_frames_from", sim3opt::NO_MEMORY, [&]() -> int {
    sim3opt_fstore::SnapshotRef s;
    if (int rc = sim3opt_fstore::take_snapshot(store, "place_batch_set_frames_from", b->opt.device, s, b->err)) return rc;
    if (s->n_frames() > SIM3OPT_PLACE_MAX_FRAMES) {
      b->err = "place_batch_set_frames_from: n_frames above SIM3OPT_PLACE_MAX_FRAMES"; return SIM3OPT_ERR_ARG;
    }
    std::vector<int32_t> kpp(s->kp_ptr);
    b->wait();
    b->kp_ptr.swap(kpp);
    std::vector<float>().swap(b->desc);
    b->have_run = false;
    b->devf.up = b->devf.solved = false;  // (the vocabulary stays where it is)
    b->snap = std::move(s);
    return SIM3OPT_OK;
  });
}

int sim3opt_place_batch_dims(const sim3opt_place_batch* b, int32_t* n_nodes, int32_t* n_words, int32_t* depth,
                             int32_t* n_frames, int32_t* total_descriptors, int32_t tiles[6]) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (n_nodes) *n_nodes = b->voc.n_nodes;
  if (n_words) *n_words = b->voc.n_words;
  if (depth) *depth = b->voc.depth;
  if (n_frames) *n_frames = b->n_frames();
  if (total_descriptors) *total_descriptors = (int32_t)b->D();
  if (tiles) {
    tiles[0] = sim3opt_place::WAVE; tiles[1] = sim3opt_place::WG; tiles[2] = sim3opt_place::BOW_CHUNK;
    tiles[3] = sim3opt_place::SCORE_LDS; tiles[4] = sim3opt_place::SCORE_JB; tiles[5] = sim3opt_place::LDS_NODES;
  }
  return SIM3OPT_OK;
}

int sim3opt_place_batch_solve(sim3opt_place_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "place_batch_solve", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve(); });
}

int sim3opt_place_batch_get_results(const sim3opt_place_batch* b, int32_t* status, int32_t* match, double* score,
                                    double* ns_factor, int32_t* n_consistent, int32_t* island) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  const size_t n = b->status.size();
  if (status) std::memcpy(status, b->status.data(), sizeof(int32_t) * n);
  if (match) std::memcpy(match, b->match.data(), sizeof(int32_t) * n);
  if (score) std::memcpy(score, b->score.data(), sizeof(double) * n);
  if (ns_factor) std::memcpy(ns_factor, b->ns.data(), sizeof(double) * n);
  if (n_consistent) std::memcpy(n_consistent, b->n_consistent.data(), sizeof(int32_t) * n);
  if (island) std::memcpy(island, b->island.data(), sizeof(int32_t) * 2 * n);
  return SIM3OPT_OK;
}

int sim3opt_place_batch_get_pairs(const sim3opt_place_batch* b, int32_t capacity, int32_t* n_pairs, int32_t* pairs) {
  if (!b || !n_pairs || capacity < 0 || (!pairs && capacity > 0)) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  const size_t n = b->pairs.size() / 2;
  *n_pairs = (int32_t)n;
  if (!pairs && capacity == 0) return SIM3OPT_OK;
  if ((size_t)capacity < n) return SIM3OPT_ERR_ARG;
  if (n) std::memcpy(pairs, b->pairs.data(), sizeof(int32_t) * 2 * n);
  return SIM3OPT_OK;
}

int sim3opt_place_batch_get_bow(const sim3opt_place_batch* b, int32_t* bow_ptr, int32_t* word, double* value) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  if (bow_ptr) std::memcpy(bow_ptr, b->bow_ptr.data(), sizeof(int32_t) * b->bow_ptr.size());
  const size_t m = b->bow_word.size();
  if (word && m) std::memcpy(word, b->bow_word.data(), sizeof(int32_t) * m);
  if (value && m) std::memcpy(value, b->bow_val.data(), sizeof(double) * m);
  return SIM3OPT_OK;
}

int sim3opt_place_batch_debug_words(sim3opt_place_batch* b, int32_t n, const float* desc, int32_t* word,
                                    double* path_d2) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (n < 1 || n > INT32_MAX / sim3opt_place::DESC || !desc || (!word && !path_d2) ||
      !sim3opt::all_finite(desc, (size_t)sim3opt_place::DESC * (size_t)n)) {
    b->err = "place_batch_debug_words: bad argument"; return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "place_batch_debug_words", sim3opt::NO_MEMORY,
                          [&] { return b->debug_words(n, desc, word, path_d2); });
}

int sim3opt_place_batch_debug_scores(sim3opt_place_batch* b, int32_t query, double* row) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!row) { b->err = "place_batch_debug_scores: bad argument"; return SIM3OPT_ERR_ARG; }
  return sim3opt::guarded(b, "place_batch_debug_scores", sim3opt::NO_MEMORY, [&] { return b->debug_scores(query, row); });
}

int sim3opt_place_batch_debug_islands(sim3opt_place_batch* b, int32_t query, int32_t* n_kept, int32_t* kept_j,
                                      double* kept_score, int32_t* n_islands, int32_t* island, double* island_score) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "place_batch_debug_islands", sim3opt::NO_MEMORY, [&] {
    return b->debug_islands(query, n_kept, kept_j, kept_score, n_islands, island, island_score);
  });
}

}  // extern "C"
