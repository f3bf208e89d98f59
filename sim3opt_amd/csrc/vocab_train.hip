// vocab_train.hip -- the vocabulary tree place recognition descends, trained on the descriptors of a sequence by
// hierarchical k-means (DBoW2's TemplatedVocabulary::create over FSurf64, Surf64Vocabulary at kitti_surf.cpp:1231).
// include/sim3opt.h ("batched vocabulary training") holds the definition the kernels follow and says what of it is the
// reference's (FSurf64::distance and meanValue, FSurf64.cpp:23-58) and what is recalled from upstream.
//
// The training is level-synchronous: all nodes of a level are clustered together, and the launches of a seeding round
// and of a Lloyd pass do not depend on the number of nodes or descriptors.  The descriptors stay where they were
// uploaded; perm keeps the members of every node of the level contiguous and in ascending descriptor index, and a
// stable counting partition on (node, cluster) writes the next level's.  vocab_host.hpp cuts every node into chunks of
// CHUNK members (a workgroup, a lane per member) and mean chunks of MEAN_CHUNK members (a wavefront, a lane per
// coordinate); a workgroup never sees two nodes, so the node's centres go through LDS.
//   seeding round c   k_vt_seed_w     w = min(w, d2 to centre c - 1) per member; the chunk's sum of w by a scan
//                     k_vt_seed_node  per node: the chunks' sums one after the other (the chunks' prefixes and W), r
//                     k_vt_seed_pick  the scan again plus the chunk's prefix; the first member above r (an integer min)
//                     k_vt_seed_commit
//   Lloyd pass        k_vt_assign     the hot one: a lane holds its descriptor's 64 floats in registers, the node's
//                                     centres are in LDS; counts the members whose cluster changed
//                     k_vt_mean_part  per mean chunk: a lane adds its coordinate of the members in ascending member
//                                     order into the cluster's double in LDS; a node of one mean chunk divides at once
//                     k_vt_mean_join  per node of several mean chunks: the partial sums in ascending chunk order
//                     k_vt_pass_end   a node without a change is done and does no work in later passes; the host reads
//                                     the number of nodes that changed
//   partition         k_vt_hist, k_vt_offsets, k_vt_scatter
// Every loop has a bound known at launch, no kernel waits for another workgroup, and there is no floating-point atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "frames_host.hpp"
#include "handle_device.hpp"
#include "ransac_sample.hpp"
#include "vocab_host.hpp"

// the definition's arithmetic is written out operation by operation: nothing is contracted into a fused multiply-add
#pragma clang fp contract(off)

namespace sim3opt_vocab {

static_assert(MEAN_CHUNK % CHUNK == 0 && CHUNK % 64 == 0, "tile sizes");

struct LevelDev {
  int32_t *start, *count, *kind, *chunk_node, *chunk_start, *chunk_len, *node_chunk0, *node_nchunks;
  int32_t *mchunk_node, *mchunk_start, *mchunk_len, *mchunk_slot, *node_mchunk0, *node_nmchunks, *multi;
  int32_t *chosen, *ncent, *sdone, *done, *changed, *pick, *chunk_cnt, *chunk_off, *child_cnt, *child_start, *part_cnt;
  int32_t* n_changed;
  float* cw;  // the centres being worked on: (node, cluster) x DESC
  double *csum, *cpre, *seedW, *seedR, *part;
};

struct Args {
  LevelDev V;
  const float* desc;
  const int32_t* perm;
  int32_t* perm_next;
  double* w;        // per position of perm
  int32_t* cl;      // per position of perm: the member's cluster
  int32_t* assign;  // per descriptor: the leaf it ended in
  int32_t k, T, first_node, round, n_chunks, n_mchunks;
  uint64_t seed;
};

// FSurf64::distance, as place_batch.hip's d2_of: b is a centre in LDS
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

__device__ inline void load_descriptor(const float* src, float (&a)[DESC]) {
  const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
  for (int k = 0; k < DESC / 4; ++k) {
    const float4 v = s4[k];
    a[4 * k] = v.x; a[4 * k + 1] = v.y; a[4 * k + 2] = v.z; a[4 * k + 3] = v.w;
  }
}

// inclusive prefix sum of v over the workgroup's CHUNK lanes, in an order that depends on the lane alone.  s: CHUNK doubles.
__device__ inline double block_incl_scan(double v, double* s) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < CHUNK; off <<= 1) {
    const double x = tid >= off ? s[tid - off] : 0.0;
    __syncthreads();
    s[tid] += x;
    __syncthreads();
  }
  const double incl = s[tid];
  __syncthreads();  // s may be written again
  return incl;
}

__global__ __launch_bounds__(CHUNK) void k_vt_iota(int32_t* perm, int32_t n) {
  const int32_t i = (int32_t)(blockIdx.x * CHUNK + threadIdx.x);
  if (i < n) perm[i] = i;
}

// centre 0 of a node that runs k-means; every member of a node of at most k
__global__ __launch_bounds__(CHUNK) void k_vt_seed0(Args A) {
  const int32_t t = (int32_t)(blockIdx.x * CHUNK + threadIdx.x);
  if (t >= A.T) return;
  const LevelDev& V = A.V;
  const int32_t kind = V.kind[t], n = V.count[t], lo = V.start[t];
  V.ncent[t] = 0; V.sdone[t] = 1;
  for (int32_t c = 0; c < A.k; ++c) {
    V.chosen[(size_t)t * A.k + c] = -1; V.seedW[(size_t)t * A.k + c] = 0; V.seedR[(size_t)t * A.k + c] = 0;
  }
  if (kind == SMALL) {
    for (int32_t c = 0; c < A.k; ++c)
      if (c < n) V.chosen[(size_t)t * A.k + c] = A.perm[lo + c];
    V.ncent[t] = n;
  } else if (kind == BIG) {
    const uint64_t z = sim3opt_ransac::splitmix64(seed_key(A.seed, A.first_node + t, 0));
    V.chosen[(size_t)t * A.k] = A.perm[lo + (int32_t)(z % (uint64_t)n)];
    V.ncent[t] = 1; V.sdone[t] = 0;
  }
}

__global__ __launch_bounds__(CHUNK) void k_vt_seed_w(Args A) {
  __shared__ __attribute__((aligned(16))) float cen[DESC];
  __shared__ double s[CHUNK];
  const LevelDev& V = A.V;
  const int32_t chunk = blockIdx.x, t = V.chunk_node[chunk], tid = threadIdx.x;
  if (V.kind[t] != BIG || V.sdone[t]) return;  // (the whole workgroup)
  const int32_t last = V.chosen[(size_t)t * A.k + A.round - 1];
  if (tid < DESC / 4)
    reinterpret_cast<float4*>(cen)[tid] = reinterpret_cast<const float4*>(A.desc + (size_t)last * DESC)[tid];
  __syncthreads();
  const int32_t p = V.chunk_start[chunk] + tid;
  double wv = 0;
  if (tid < V.chunk_len[chunk]) {
    float a[DESC];
    load_descriptor(A.desc + (size_t)A.perm[p] * DESC, a);
    const double d = d2_of(a, cen);
    wv = d;
    if (A.round > 1) { const double old = A.w[p]; wv = d < old ? d : old; }
    A.w[p] = wv;
  }
  const double incl = block_incl_scan(wv, s);
  if (tid == CHUNK - 1) V.csum[chunk] = incl;
}

__global__ __launch_bounds__(CHUNK) void k_vt_seed_node(Args A) {
  const int32_t t = (int32_t)(blockIdx.x * CHUNK + threadIdx.x);
  if (t >= A.T) return;
  const LevelDev& V = A.V;
  if (V.kind[t] != BIG || V.sdone[t]) return;
  const int32_t c0 = V.node_chunk0[t], nch = V.node_nchunks[t];
  const double* __restrict__ csum = V.csum;
  double* __restrict__ cpre = V.cpre;
  double W = 0;
  for (int32_t j = 0; j < nch; ++j) { cpre[c0 + j] = W; W += csum[c0 + j]; }
  const size_t at = (size_t)t * A.k + A.round;
  if (W == 0) {  // every member equals a centre: the seeding ends with `round` centres
    V.sdone[t] = 1;
    return;
  }
  const uint64_t z = sim3opt_ransac::splitmix64(seed_key(A.seed, A.first_node + t, A.round));
  const double u = (double)(z >> 11) * 0x1.0p-53;
  V.seedW[at] = W; V.seedR[at] = u * W;
  V.pick[t] = INT_MAX;
}

__global__ __launch_bounds__(CHUNK) void k_vt_seed_pick(Args A) {
  __shared__ double s[CHUNK];
  __shared__ int32_t first;
  const LevelDev& V = A.V;
  const int32_t chunk = blockIdx.x, t = V.chunk_node[chunk], tid = threadIdx.x;
  if (V.kind[t] != BIG || V.sdone[t]) return;
  if (tid == 0) first = INT_MAX;
  const int32_t p = V.chunk_start[chunk] + tid;
  const bool active = tid < V.chunk_len[chunk];
  const double incl = block_incl_scan(active ? A.w[p] : 0.0, s) + V.cpre[chunk];  // (the scan's barriers order `first`)
  if (active && incl > V.seedR[(size_t)t * A.k + A.round]) atomicMin(&first, p);
  __syncthreads();
  if (tid == 0 && first != INT_MAX) atomicMin(&V.pick[t], first);
}

__global__ __launch_bounds__(CHUNK) void k_vt_seed_commit(Args A) {
  const int32_t t = (int32_t)(blockIdx.x * CHUNK + threadIdx.x);
  if (t >= A.T) return;
  const LevelDev& V = A.V;
  if (V.kind[t] != BIG || V.sdone[t]) return;
  const int32_t last = V.start[t] + V.count[t] - 1;
  int32_t p = V.pick[t];
  if (p < V.start[t] || p > last) p = last;  // (no prefix above r: r < W, so only a rounding of the last prefix)
  V.chosen[(size_t)t * A.k + A.round] = A.perm[p];
  V.ncent[t] = A.round + 1;
}

// a node whose seeding ended with one centre is a leaf; the flags of the Lloyd passes
__global__ __launch_bounds__(CHUNK) void k_vt_seed_end(Args A) {
  const int32_t t = (int32_t)(blockIdx.x * CHUNK + threadIdx.x);
  if (t >= A.T) return;
  const LevelDev& V = A.V;
  if (V.kind[t] == BIG && V.ncent[t] == 1) V.kind[t] = LEAF;
  V.done[t] = V.kind[t] != BIG;
  V.changed[t] = 0;
}

// the chosen members' descriptors as the first centres (float4 q of centre s), zero where there is none
__global__ __launch_bounds__(CHUNK) void k_vt_init_centres(Args A) {
  const size_t i = (size_t)blockIdx.x * CHUNK + threadIdx.x;
  if (i >= (size_t)A.T * A.k * (DESC / 4)) return;
  const size_t s = i / (DESC / 4), q = i % (DESC / 4);
  const int32_t t = (int32_t)(s / A.k), c = (int32_t)(s % A.k);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (A.V.kind[t] != LEAF && c < A.V.ncent[t])
    v = reinterpret_cast<const float4*>(A.desc + (size_t)A.V.chosen[s] * DESC)[q];
  reinterpret_cast<float4*>(A.V.cw)[i] = v;
}

// before the first pass: no cluster (k-means), the member's rank (a node of at most k); a leaf's members end here
__global__ __launch_bounds__(CHUNK) void k_vt_init_cl(Args A) {
  const LevelDev& V = A.V;
  const int32_t chunk = blockIdx.x, t = V.chunk_node[chunk], tid = threadIdx.x;
  if (tid >= V.chunk_len[chunk]) return;
  const int32_t p = V.chunk_start[chunk] + tid, kind = V.kind[t];
  if (kind == LEAF) { A.assign[A.perm[p]] = A.first_node + t; A.cl[p] = -1; }
  else A.cl[p] = kind == SMALL ? p - V.start[t] : -1;
}

__global__ __launch_bounds__(CHUNK) void k_vt_assign(Args A) {
  __shared__ __attribute__((aligned(16))) float cen[MAX_K * DESC];
  const LevelDev& V = A.V;
  const int32_t chunk = blockIdx.x, t = V.chunk_node[chunk], tid = threadIdx.x;
  if (V.kind[t] != BIG || V.done[t]) return;  // (the whole workgroup)
  const int32_t nc = V.ncent[t];
  const float4* src = reinterpret_cast<const float4*>(V.cw + (size_t)t * A.k * DESC);
  for (int32_t i = tid; i < nc * (DESC / 4); i += CHUNK) reinterpret_cast<float4*>(cen)[i] = src[i];
  __syncthreads();
  int moved = 0;
  if (tid < V.chunk_len[chunk]) {
    const int32_t p = V.chunk_start[chunk] + tid;
    float a[DESC];
    load_descriptor(A.desc + (size_t)A.perm[p] * DESC, a);
    double best = d2_of(a, cen);
    int32_t bc = 0;
    for (int32_t c = 1; c < nc; ++c) {
      const double d = d2_of(a, cen + (size_t)c * DESC);
      if (d < best) { best = d; bc = c; }  // (strict: on equal d2 the lower cluster stays)
    }
    moved = bc != A.cl[p];
    A.cl[p] = bc;
  }
  const int n = __syncthreads_count(moved);
  if (tid == 0 && n) atomicAdd(&V.changed[t], n);
}

__global__ __launch_bounds__(64) void k_vt_mean_part(Args A) {
  __shared__ double acc[MAX_K * DESC];
  __shared__ int32_t cnt[MAX_K], scl[MEAN_CHUNK], sperm[MEAN_CHUNK];
  const LevelDev& V = A.V;
  const int32_t m = blockIdx.x, t = V.mchunk_node[m], j = threadIdx.x;
  if (V.kind[t] != BIG || V.done[t] || V.changed[t] == 0) return;
  const int32_t nc = V.ncent[t], lo = V.mchunk_start[m], len = V.mchunk_len[m];
  for (int32_t c = 0; c < nc; ++c) acc[c * DESC + j] = 0;
  if (j < nc) cnt[j] = 0;
  for (int32_t i = j; i < len; i += 64) { scl[i] = A.cl[lo + i]; sperm[i] = A.perm[lo + i]; }
  __syncthreads();
  for (int32_t i = 0; i < len; ++i) {  // ascending member order: the sum's order
    const int32_t c = scl[i];
    acc[c * DESC + j] += (double)A.desc[(size_t)sperm[i] * DESC + j];
    if (j == 0) ++cnt[c];
  }
  __syncthreads();
  const int32_t slot = V.mchunk_slot[m];
  for (int32_t c = 0; c < nc; ++c) {
    if (slot < 0) {
      if (cnt[c] > 0) V.cw[((size_t)t * A.k + c) * DESC + j] = (float)(acc[c * DESC + j] / (double)cnt[c]);
    } else {
      V.part[((size_t)slot * A.k + c) * DESC + j] = acc[c * DESC + j];
      if (j == 0) V.part_cnt[(size_t)slot * A.k + c] = cnt[c];
    }
  }
}

__global__ __launch_bounds__(64) void k_vt_mean_join(Args A) {
  const LevelDev& V = A.V;
  const int32_t t = V.multi[blockIdx.x], j = threadIdx.x;
  if (V.kind[t] != BIG || V.done[t] || V.changed[t] == 0) return;
  const int32_t nc = V.ncent[t], nm = V.node_nmchunks[t], slot0 = V.mchunk_slot[V.node_mchunk0[t]];
  for (int32_t c = 0; c < nc; ++c) {
    double sum = 0;
    int32_t n = 0;
    for (int32_t q = 0; q < nm; ++q) {  // ascending chunk order
      sum += V.part[((size_t)(slot0 + q) * A.k + c) * DESC + j];
      n += V.part_cnt[(size_t)(slot0 + q) * A.k + c];
    }
    if (n > 0) V.cw[((size_t)t * A.k + c) * DESC + j] = (float)(sum / (double)n);  // (an empty cluster keeps its centre)
  }
}

__global__ __launch_bounds__(CHUNK) void k_vt_pass_end(Args A) {
  const int32_t t = (int32_t)(blockIdx.x * CHUNK + threadIdx.x);
  if (t >= A.T) return;
  const LevelDev& V = A.V;
  if (V.kind[t] != BIG || V.done[t]) return;
  if (V.changed[t] == 0) V.done[t] = 1;
  else atomicAdd(V.n_changed, 1);
  V.changed[t] = 0;
}

// ---- the stable counting partition on (node, cluster)
__global__ __launch_bounds__(CHUNK) void k_vt_hist(Args A) {
  __shared__ int32_t h[MAX_K];
  const LevelDev& V = A.V;
  const int32_t chunk = blockIdx.x, t = V.chunk_node[chunk], tid = threadIdx.x;
  if (V.kind[t] == LEAF) return;
  if (tid < A.k) h[tid] = 0;
  __syncthreads();
  if (tid < V.chunk_len[chunk]) atomicAdd(&h[A.cl[V.chunk_start[chunk] + tid]], 1);
  __syncthreads();
  if (tid < A.k) V.chunk_cnt[(size_t)chunk * A.k + tid] = h[tid];
}

__global__ __launch_bounds__(CHUNK) void k_vt_offsets(Args A) {
  const size_t s = (size_t)blockIdx.x * CHUNK + threadIdx.x;
  if (s >= (size_t)A.T * A.k) return;
  const LevelDev& V = A.V;
  const int32_t t = (int32_t)(s / A.k), c = (int32_t)(s % A.k);
  int32_t run = 0;
  if (V.kind[t] != LEAF) {
    const int32_t c0 = V.node_chunk0[t], nch = V.node_nchunks[t];
    const int32_t* __restrict__ cnt = V.chunk_cnt;
    int32_t* __restrict__ off = V.chunk_off;
    for (int32_t q = 0; q < nch; ++q) {
      off[(size_t)(c0 + q) * A.k + c] = run;
      run += cnt[(size_t)(c0 + q) * A.k + c];
    }
  }
  V.child_cnt[s] = run;
}

__global__ __launch_bounds__(CHUNK) void k_vt_scatter(Args A) {
  __shared__ int32_t sc[CHUNK];
  const LevelDev& V = A.V;
  const int32_t chunk = blockIdx.x, t = V.chunk_node[chunk], tid = threadIdx.x;
  if (V.kind[t] == LEAF) return;
  const int32_t len = V.chunk_len[chunk], p = V.chunk_start[chunk] + tid;
  const int32_t c = tid < len ? A.cl[p] : -1;
  sc[tid] = c;
  __syncthreads();
  if (tid >= len) return;
  int32_t rank = 0;
  for (int32_t i = 0; i < CHUNK; ++i) rank += (i < tid) && sc[i] == c;
  A.perm_next[V.child_start[(size_t)t * A.k + c] + V.chunk_off[(size_t)chunk * A.k + c] + rank] = A.perm[p];
}

// the descent rule of place recognition on the finished tree (breadth first: a node's children are consecutive): the
// node every descriptor's descent ends in.  depth bounds the loop.
__global__ __launch_bounds__(CHUNK) void k_vt_descend(const float* centre, const int32_t* first_child, const int32_t* n_child,
                                                      int32_t depth, const float* desc, int32_t n_desc, int32_t* out) {
  const int32_t d = (int32_t)(blockIdx.x * CHUNK + threadIdx.x);
  if (d >= n_desc) return;
  float a[DESC];
  load_descriptor(desc + (size_t)d * DESC, a);
  int32_t node = 0;
  for (int32_t level = 0; level < depth; ++level) {
    const int32_t nc = n_child[node];
    if (nc == 0) break;
    const int32_t c0 = first_child[node];
    double best = d2_of(a, centre + (size_t)c0 * DESC);
    int32_t bc = c0;
    for (int32_t c = c0 + 1; c < c0 + nc; ++c) {
      const double dd = d2_of(a, centre + (size_t)c * DESC);
      if (dd < best) { best = dd; bc = c; }
    }
    node = bc;
  }
  out[d] = node;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct StoredLevel {  // the start of a level, for the read-outs
  Level V;            // (kind as after the seeding)
  std::vector<int32_t> chosen, ncent;
  std::vector<double> seedW, seedR;
  int32_t passes = 0;
};

inline unsigned blocks(size_t n) { return (unsigned)((n + CHUNK - 1) / CHUNK); }

struct Trainer : sim3opt::BatchHandle {
  sim3opt_vocabulary_options opt;
  std::vector<int32_t> kp_ptr;
  std::vector<float> desc;
  // the last training
  sim3opt_vocabulary_options run_opt;
  Tree tree;
  std::vector<StoredLevel> stored;
  std::vector<int32_t> assignment, descent;
  int32_t n_words = 0, depth = 0, n_unconverged = 0;
  // device
  sim3opt::DevArena frame_mem, level_mem;
  sim3opt_fstore::SnapshotRef snap;  // set_frames_from: dev.desc is the snapshot's, not frame_mem's
  struct Dev {
    float* desc;
    int32_t *perm;  // (levels + 1) x D: the members of every level's nodes
    int32_t *cl, *assign, *descent;
    double* w;
    int32_t levels;  // what perm has room for
    bool up, trained;
  } dev{};

  ~Trainer() { release(); }
  int32_t n_frames() const { return kp_ptr.empty() ? 0 : (int32_t)kp_ptr.size() - 1; }
  size_t D() const { return kp_ptr.empty() ? 0 : (size_t)kp_ptr.back(); }

  void release() {
    close_stream(level_mem, frame_mem);
    dev = Dev{};
  }

  int ensure_device(const char* who) {
    if (n_frames() < 1) { err = std::string(who) + ": no frames set"; return SIM3OPT_ERR_STATE; }
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    if (snap)
      if (int rc = sim3opt_fstore::check_snapshot_device(*snap, who, opt.device, err)) return rc;
    if (!stream) {
      release();
      if (int rc = open_stream()) return rc;
    }
    if (!dev.up || dev.levels != opt.levels) {
      wait();
      level_mem.release(); frame_mem.release();
      dev = Dev{};
      const size_t d = D();
      if (snap) dev.desc = snap->d_desc;  // read in place: nothing of the frames is uploaded
      else HIPCHK(frame_mem.upload(dev.desc, desc, stream, nullptr));
      HIPCHK(frame_mem.raw(dev.perm, d * (size_t)(opt.levels + 1)));
      HIPCHK(frame_mem.raw(dev.cl, d));
      HIPCHK(frame_mem.raw(dev.assign, d));
      HIPCHK(frame_mem.raw(dev.descent, d));
      HIPCHK(frame_mem.raw(dev.w, d));
      HIPCHK(hipStreamSynchronize(stream));
      dev.levels = opt.levels;
      dev.up = true;
    }
    return SIM3OPT_OK;
  }

  // the tables of a level on the device, in level_mem (whatever it held goes first)
  int upload_level(const Level& V, int32_t k, LevelDev& L) {
    wait();
    level_mem.release();
    L = LevelDev{};
    const size_t T = (size_t)V.T(), nch = V.chunk_node.size(), tk = T * (size_t)k;
    HIPCHK(level_mem.upload(L.start, V.start, stream, nullptr));
    HIPCHK(level_mem.upload(L.count, V.count, stream, nullptr));
    HIPCHK(level_mem.upload(L.kind, V.kind, stream, nullptr));
    HIPCHK(level_mem.upload(L.chunk_node, V.chunk_node, stream, nullptr));
    HIPCHK(level_mem.upload(L.chunk_start, V.chunk_start, stream, nullptr));
    HIPCHK(level_mem.upload(L.chunk_len, V.chunk_len, stream, nullptr));
    HIPCHK(level_mem.upload(L.node_chunk0, V.node_chunk0, stream, nullptr));
    HIPCHK(level_mem.upload(L.node_nchunks, V.node_nchunks, stream, nullptr));
    HIPCHK(level_mem.upload(L.mchunk_node, V.mchunk_node, stream, nullptr));
    HIPCHK(level_mem.upload(L.mchunk_start, V.mchunk_start, stream, nullptr));
    HIPCHK(level_mem.upload(L.mchunk_len, V.mchunk_len, stream, nullptr));
    HIPCHK(level_mem.upload(L.mchunk_slot, V.mchunk_slot, stream, nullptr));
    HIPCHK(level_mem.upload(L.node_mchunk0, V.node_mchunk0, stream, nullptr));
    HIPCHK(level_mem.upload(L.node_nmchunks, V.node_nmchunks, stream, nullptr));
    HIPCHK(level_mem.upload(L.multi, V.multi, stream, nullptr));
    HIPCHK(level_mem.raw(L.chosen, tk));
    HIPCHK(level_mem.raw(L.ncent, T));
    HIPCHK(level_mem.raw(L.sdone, T));
    HIPCHK(level_mem.raw(L.done, T));
    HIPCHK(level_mem.raw(L.changed, T));
    HIPCHK(level_mem.raw(L.pick, T));
    HIPCHK(level_mem.raw(L.chunk_cnt, nch * (size_t)k));
    HIPCHK(level_mem.raw(L.chunk_off, nch * (size_t)k));
    HIPCHK(level_mem.raw(L.child_cnt, tk));
    HIPCHK(level_mem.raw(L.child_start, tk));
    HIPCHK(level_mem.raw(L.part_cnt, (size_t)V.n_slots * (size_t)k));
    HIPCHK(level_mem.alloc(L.n_changed, 1, stream));
    HIPCHK(level_mem.raw(L.cw, tk * DESC));
    HIPCHK(level_mem.raw(L.csum, nch));
    HIPCHK(level_mem.raw(L.cpre, nch));
    HIPCHK(level_mem.raw(L.seedW, tk));
    HIPCHK(level_mem.raw(L.seedR, tk));
    HIPCHK(level_mem.raw(L.part, (size_t)V.n_slots * (size_t)k * DESC));
    return SIM3OPT_OK;
  }

  Args args(const sim3opt_vocabulary_options& o, const Level& V, const LevelDev& L, int32_t level) const {
    Args A{};
    A.V = L;
    A.desc = dev.desc;
    A.perm = dev.perm + (size_t)level * D();
    A.perm_next = level < dev.levels ? dev.perm + (size_t)(level + 1) * D() : nullptr;
    A.w = dev.w; A.cl = dev.cl; A.assign = dev.assign;
    A.k = o.k; A.T = V.T(); A.first_node = V.first_node; A.round = 0;
    A.n_chunks = (int32_t)V.chunk_node.size(); A.n_mchunks = (int32_t)V.mchunk_node.size();
    A.seed = o.seed;
    return A;
  }

  // what precedes the first pass of a level, from the seeding's outcome on the device: the flags, the first centres,
  // the clusters; the leaves' members receive their node
  void launch_start(const Args& A) {
    hipLaunchKernelGGL(k_vt_seed_end, dim3(blocks((size_t)A.T)), dim3(CHUNK), 0, stream, A);
    hipLaunchKernelGGL(k_vt_init_centres, dim3(blocks((size_t)A.T * A.k * (DESC / 4))), dim3(CHUNK), 0, stream, A);
    hipLaunchKernelGGL(k_vt_init_cl, dim3((unsigned)A.n_chunks), dim3(CHUNK), 0, stream, A);
  }

  void launch_pass(const Args& A, const Level& V) {
    hipLaunchKernelGGL(k_vt_assign, dim3((unsigned)A.n_chunks), dim3(CHUNK), 0, stream, A);
    if (A.n_mchunks) hipLaunchKernelGGL(k_vt_mean_part, dim3((unsigned)A.n_mchunks), dim3(64), 0, stream, A);
    if (!V.multi.empty()) hipLaunchKernelGGL(k_vt_mean_join, dim3((unsigned)V.multi.size()), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k_vt_pass_end, dim3(blocks((size_t)A.T)), dim3(CHUNK), 0, stream, A);
  }

  int train() {
    err.clear();
    if (int rc = ensure_device("vocabulary_train")) return rc;
    const sim3opt_vocabulary_options o = opt;
    const size_t d = D();
    const int32_t k = o.k;
    dev.trained = false;
    Tree R;
    R.start();
    std::vector<StoredLevel> st;
    int32_t unconverged = 0;
    Level V;
    V.first_node = 0;
    V.count.assign(1, (int32_t)d);
    hipLaunchKernelGGL(k_vt_iota, dim3(blocks(d)), dim3(CHUNK), 0, stream, dev.perm, (int32_t)d);
    for (int32_t level = 0; level <= o.levels; ++level) {
      plan_level(V, level, o.levels, k);
      LevelDev L;
      if (int rc = upload_level(V, k, L)) return rc;
      Args A = args(o, V, L, level);
      const size_t T = (size_t)V.T(), tk = T * (size_t)k;
      bool any_big = false;
      for (int32_t kd : V.kind) any_big = any_big || kd == BIG;
      hipLaunchKernelGGL(k_vt_seed0, dim3(blocks(T)), dim3(CHUNK), 0, stream, A);
      if (any_big)
        for (int32_t c = 1; c < k; ++c) {
          A.round = c;
          hipLaunchKernelGGL(k_vt_seed_w, dim3((unsigned)A.n_chunks), dim3(CHUNK), 0, stream, A);
          hipLaunchKernelGGL(k_vt_seed_node, dim3(blocks(T)), dim3(CHUNK), 0, stream, A);
          hipLaunchKernelGGL(k_vt_seed_pick, dim3((unsigned)A.n_chunks), dim3(CHUNK), 0, stream, A);
          hipLaunchKernelGGL(k_vt_seed_commit, dim3(blocks(T)), dim3(CHUNK), 0, stream, A);
        }
      A.round = 0;
      launch_start(A);
      HIPCHK(hipGetLastError());
      StoredLevel S;
      HIPCHK(sim3opt::read_back(V.kind, L.kind, T, stream));
      HIPCHK(sim3opt::read_back(S.chosen, L.chosen, tk, stream));
      HIPCHK(sim3opt::read_back(S.ncent, L.ncent, T, stream));
      HIPCHK(sim3opt::read_back(S.seedW, L.seedW, tk, stream));
      HIPCHK(sim3opt::read_back(S.seedR, L.seedR, tk, stream));
      HIPCHK(hipStreamSynchronize(stream));
      bool any_split = false;
      any_big = false;
      for (int32_t kd : V.kind) { any_split = any_split || kd != LEAF; any_big = any_big || kd == BIG; }
      if (any_big) {
        std::vector<int32_t> nchg;
        for (int32_t p = 1; p <= o.max_iters; ++p) {
          HIPCHK(hipMemsetAsync(L.n_changed, 0, sizeof(int32_t), stream));
          launch_pass(A, V);
          HIPCHK(hipGetLastError());
          HIPCHK(sim3opt::read_back(nchg, L.n_changed, 1, stream));
          HIPCHK(hipStreamSynchronize(stream));
          S.passes = p;
          if (nchg[0] == 0) break;
        }
        std::vector<int32_t> done;
        HIPCHK(sim3opt::read_back(done, L.done, T, stream));
        HIPCHK(hipStreamSynchronize(stream));
        for (size_t t = 0; t < T; ++t) unconverged += V.kind[t] == BIG && !done[t];
      }
      S.V = V;
      if (any_split) {
        hipLaunchKernelGGL(k_vt_hist, dim3((unsigned)A.n_chunks), dim3(CHUNK), 0, stream, A);
        hipLaunchKernelGGL(k_vt_offsets, dim3(blocks(tk)), dim3(CHUNK), 0, stream, A);
        HIPCHK(hipGetLastError());
        std::vector<int32_t> child_cnt, child_start;
        std::vector<float> cw;
        HIPCHK(sim3opt::read_back(child_cnt, L.child_cnt, tk, stream));
        HIPCHK(sim3opt::read_back(cw, L.cw, tk * DESC, stream));
        HIPCHK(hipStreamSynchronize(stream));
        Level N;
        N.first_node = R.n_nodes();
        std::string e;
        N.count = append_children(R, V, level, k, child_cnt, cw, child_start, e);
        if (!e.empty()) { err = "vocabulary_train: " + e; return SIM3OPT_ERR_ARG; }
        size_t members = 0;
        for (int32_t n : N.count) members += (size_t)n;
        if (N.count.empty() || members > d || !A.perm_next) {
          err = "vocabulary_train: internal error (the partition's counts)"; return SIM3OPT_ERR_HIP;
        }
        HIPCHK(hipMemcpyAsync(L.child_start, child_start.data(), sizeof(int32_t) * tk, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_vt_scatter, dim3((unsigned)A.n_chunks), dim3(CHUNK), 0, stream, A);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));  // (child_start is read from this frame)
        V = std::move(N);
      }
      st.push_back(std::move(S));
      if (!any_split) break;
    }
    // the words, the descent of every training descriptor on the finished tree, the weights
    std::vector<int32_t> first_child, n_child, asg, dsc;
    int32_t dep = 0;
    const int32_t words = finish_tree(R, first_child, n_child, dep);
    {
      wait();
      level_mem.release();
      float* dc = nullptr;
      int32_t *dfc = nullptr, *dnc = nullptr;
      HIPCHK(level_mem.upload(dc, R.centre, stream, nullptr));
      HIPCHK(level_mem.upload(dfc, first_child, stream, nullptr));
      HIPCHK(level_mem.upload(dnc, n_child, stream, nullptr));
      hipLaunchKernelGGL(k_vt_descend, dim3(blocks(d)), dim3(CHUNK), 0, stream, dc, dfc, dnc, dep, dev.desc, (int32_t)d,
                         dev.descent);
      HIPCHK(hipGetLastError());
      HIPCHK(sim3opt::read_back(asg, dev.assign, d, stream));
      HIPCHK(sim3opt::read_back(dsc, dev.descent, d, stream));
      HIPCHK(hipStreamSynchronize(stream));
      level_mem.release();
    }
    for (size_t i = 0; i < d; ++i)
      if (asg[i] < 0 || asg[i] >= R.n_nodes() || dsc[i] < 0 || dsc[i] >= R.n_nodes() || n_child[(size_t)asg[i]] ||
          n_child[(size_t)dsc[i]]) {
        err = "vocabulary_train: internal error (a descriptor outside the leaves)"; return SIM3OPT_ERR_HIP;
      }
    idf_weights(R, n_frames(), kp_ptr.data(), dsc.data(), o.idf);
    tree = std::move(R);
    stored.swap(st); assignment.swap(asg); descent.swap(dsc);
    n_words = words; depth = dep; n_unconverged = unconverged;
    run_opt = o;
    have_run = true;
    dev.trained = true;
    return tree.n_nodes();
  }

  int trained_on_device(const char* who) {
    err.clear();
    if (!have_run) { err = std::string(who) + ": no training yet"; return SIM3OPT_ERR_STATE; }
    if (!dev.up || !dev.trained) {
      err = std::string(who) + ": the device blocks of the last training were released; train again";
      return SIM3OPT_ERR_STATE;
    }
    return SIM3OPT_OK;
  }

  // the level of an output node (levels are consecutive runs of the numbering): -1 when there is none
  int32_t level_of(int32_t node) const {
    for (size_t l = 0; l < stored.size(); ++l)
      if (node >= stored[l].V.first_node && node < stored[l].V.first_node + stored[l].V.T()) return (int32_t)l;
    return -1;
  }

  int debug_seeding(int32_t node, int32_t* n_chosen, int32_t* member, int32_t* n_rounds, double* W, double* r) {
    err.clear();
    if (!have_run) { err = "vocabulary_debug_seeding: no training yet"; return SIM3OPT_ERR_STATE; }
    const int32_t l = level_of(node);
    if (l < 0) { err = "vocabulary_debug_seeding: no such node"; return SIM3OPT_ERR_ARG; }
    const StoredLevel& S = stored[(size_t)l];
    const size_t t = (size_t)(node - S.V.first_node), k = (size_t)run_opt.k;
    const bool seeded = S.V.count[t] > run_opt.k && l < run_opt.levels;
    const int32_t nc = seeded ? S.ncent[t] : 0;
    const int32_t rounds = !seeded ? 0 : nc < run_opt.k ? nc : run_opt.k - 1;
    if (n_chosen) *n_chosen = nc;
    if (n_rounds) *n_rounds = rounds;
    for (int32_t c = 0; c < nc; ++c)
      if (member) member[c] = S.chosen[t * k + (size_t)c];
    for (int32_t c = 1; c <= rounds; ++c) {
      if (W) W[c - 1] = S.seedW[t * k + (size_t)c];
      if (r) r[c - 1] = S.seedR[t * k + (size_t)c];
    }
    return SIM3OPT_OK;
  }

  int debug_lloyd(int32_t level, int32_t pass, int32_t* first_node, int32_t* n_level_nodes, int32_t* cluster,
                  float* centre) {
    if (int rc = trained_on_device("vocabulary_debug_lloyd")) return rc;
    if (level < 0 || (size_t)level >= stored.size()) { err = "vocabulary_debug_lloyd: no such level"; return SIM3OPT_ERR_ARG; }
    const StoredLevel& S = stored[(size_t)level];
    if (pass < 0 || pass > S.passes) { err = "vocabulary_debug_lloyd: no such pass"; return SIM3OPT_ERR_ARG; }
    if (first_node) *first_node = S.V.first_node;
    if (n_level_nodes) *n_level_nodes = S.V.T();
    if (!cluster && !centre) return SIM3OPT_OK;
    const size_t T = (size_t)S.V.T(), tk = T * (size_t)run_opt.k, d = D(), m = (size_t)S.V.n_members;
    LevelDev L;
    if (int rc = upload_level(S.V, run_opt.k, L)) return rc;
    const Args A = args(run_opt, S.V, L, level);
    HIPCHK(hipMemcpyAsync(L.chosen, S.chosen.data(), sizeof(int32_t) * tk, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(L.ncent, S.ncent.data(), sizeof(int32_t) * T, hipMemcpyHostToDevice, stream));
    launch_start(A);
    for (int32_t p = 1; p <= pass; ++p) launch_pass(A, S.V);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> cl, perm;
    std::vector<float> cw;
    HIPCHK(sim3opt::read_back(cl, dev.cl, m, stream));
    HIPCHK(sim3opt::read_back(perm, A.perm, m, stream));
    HIPCHK(sim3opt::read_back(cw, L.cw, tk * DESC, stream));
    HIPCHK(hipStreamSynchronize(stream));
    level_mem.release();
    if (cluster) {
      for (size_t i = 0; i < d; ++i) cluster[i] = -1;
      for (size_t p = 0; p < m; ++p) {
        if (perm[p] < 0 || (size_t)perm[p] >= d) { err = "vocabulary_debug_lloyd: internal error (perm)"; return SIM3OPT_ERR_HIP; }
        cluster[perm[p]] = cl[p];
      }
    }
    if (centre) std::memcpy(centre, cw.data(), sizeof(float) * tk * DESC);
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_vocab

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched vocabulary training")
// ------------------------------------------------------------------------------------------
struct sim3opt_vocabulary : sim3opt_vocab::Trainer {};

extern "C" {

void sim3opt_vocabulary_options_default(sim3opt_vocabulary_options* o) {
  if (!o) return;
  o->seed = 0;
  o->k = 10;           // [upstream recall] DBoW2's default branching
  o->levels = 5;       // [upstream recall] DBoW2's default depth
  o->max_iters = 100;  // ours: DBoW2 iterates until nothing changes
  o->idf = 1;          // [upstream recall] TF_IDF is DBoW2's default weighting
  o->device = -1;
}

sim3opt_vocabulary* sim3opt_vocabulary_create(void) {
  return sim3opt::handle_create<sim3opt_vocabulary>(sim3opt_vocabulary_options_default);
}

void sim3opt_vocabulary_destroy(sim3opt_vocabulary* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_vocabulary_last_error(const sim3opt_vocabulary* b) { return b ? b->err.c_str() : "null trainer"; }

int sim3opt_vocabulary_set_options(sim3opt_vocabulary* b, const sim3opt_vocabulary_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  const std::string e = sim3opt_vocab::validate_options(*o);
  if (!e.empty()) { b->err = "vocabulary_set_options: " + e; return SIM3OPT_ERR_ARG; }
  if (o->device != b->opt.device && b->snap) {
    b->err = "vocabulary_set_options: the frames are a store's snapshot on its device; options.device cannot change";
    return SIM3OPT_ERR_ARG;
  }
  if (o->device != b->opt.device) b->release();  // the device is chosen at the next training
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_vocabulary_set_frames(sim3opt_vocabulary* b, int32_t n_frames, const int32_t* kp_ptr, const float* desc) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "vocabulary_set_frames", sim3opt::NO_MEMORY, [&]() -> int {
    const std::string e = sim3opt_vocab::validate_frames(n_frames, kp_ptr, desc);
    if (!e.empty()) { b->err = "vocabulary_set_frames: " + e; return SIM3OPT_ERR_ARG; }
    std::vector<int32_t> kpp(kp_ptr, kp_ptr + n_frames + 1);
    std::vector<float> d(desc, desc + (size_t)sim3opt_vocab::DESC * (size_t)kp_ptr[n_frames]);
    b->kp_ptr.swap(kpp); b->desc.swap(d);
    b->have_run = false;
    b->dev.up = b->dev.trained = false;
    b->snap.reset();
    return SIM3OPT_OK;
  });
}

int sim3opt_vocabulary_set_frames_from(sim3opt_vocabulary* b, const sim3opt_frames* store) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "vocabulary_set_frames_from", sim3opt::NO_MEMORY, [&]() -> int {
    sim3opt_fstore::SnapshotRef s;
    if (int rc = sim3opt_fstore::take_snapshot(store, "vocabulary_set_frames_from", b->opt.device, s, b->err)) return rc;
    std::string e;
    if (s->n_frames() > SIM3OPT_PLACE_MAX_FRAMES) e = "n_frames above SIM3OPT_PLACE_MAX_FRAMES";
    else if (!s->distinct) e = sim3opt_vocab::MSG_DISTINCT;  // (the fill looked on the device)
    if (!e.empty()) { b->err = "vocabulary_set_frames_from: " + e; return SIM3OPT_ERR_ARG; }
    std::vector<int32_t> kpp(s->kp_ptr);
    b->wait();
    b->kp_ptr.swap(kpp);
    std::vector<float>().swap(b->desc);
    b->have_run = false;
    b->dev.up = b->dev.trained = false;
    b->snap = std::move(s);
    return SIM3OPT_OK;
  });
}

int sim3opt_vocabulary_train(sim3opt_vocabulary* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "vocabulary_train", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->train(); });
}

int sim3opt_vocabulary_dims(const sim3opt_vocabulary* b, int32_t* n_nodes, int32_t* n_words, int32_t* depth,
                            int32_t* n_unconverged, int32_t* n_frames, int32_t* total_descriptors, int32_t passes[8],
                            int32_t tiles[2]) {
  if (!b) return SIM3OPT_ERR_ARG;
  const bool run = b->have_run;
  if (n_nodes) *n_nodes = run ? b->tree.n_nodes() : 0;
  if (n_words) *n_words = run ? b->n_words : 0;
  if (depth) *depth = run ? b->depth : 0;
  if (n_unconverged) *n_unconverged = run ? b->n_unconverged : 0;
  if (n_frames) *n_frames = b->n_frames();
  if (total_descriptors) *total_descriptors = (int32_t)b->D();
  if (passes)
    for (size_t l = 0; l < (size_t)sim3opt_vocab::MAX_LEVELS; ++l)
      passes[l] = run && l < b->stored.size() ? b->stored[l].passes : 0;
  if (tiles) { tiles[0] = sim3opt_vocab::CHUNK; tiles[1] = sim3opt_vocab::MEAN_CHUNK; }
  return SIM3OPT_OK;
}

int sim3opt_vocabulary_get_vocabulary(const sim3opt_vocabulary* b, int32_t* parent, float* centre, double* weight,
                                      int32_t* word_id) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  const size_t n = (size_t)b->tree.n_nodes();
  if (parent) std::memcpy(parent, b->tree.parent.data(), sizeof(int32_t) * n);
  if (centre) std::memcpy(centre, b->tree.centre.data(), sizeof(float) * n * sim3opt_vocab::DESC);
  if (weight) std::memcpy(weight, b->tree.weight.data(), sizeof(double) * n);
  if (word_id) std::memcpy(word_id, b->tree.word_id.data(), sizeof(int32_t) * n);
  return SIM3OPT_OK;
}

int sim3opt_vocabulary_get_assignment(const sim3opt_vocabulary* b, int32_t* node_of_descriptor, int32_t* descent_node) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  const size_t d = b->assignment.size();
  if (node_of_descriptor && d) std::memcpy(node_of_descriptor, b->assignment.data(), sizeof(int32_t) * d);
  if (descent_node && d) std::memcpy(descent_node, b->descent.data(), sizeof(int32_t) * d);
  return SIM3OPT_OK;
}

int sim3opt_vocabulary_debug_seeding(sim3opt_vocabulary* b, int32_t node, int32_t* n_chosen, int32_t* member,
                                     int32_t* n_rounds, double* W, double* r) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "vocabulary_debug_seeding", sim3opt::NO_MEMORY,
                          [&] { return b->debug_seeding(node, n_chosen, member, n_rounds, W, r); });
}

int sim3opt_vocabulary_debug_lloyd(sim3opt_vocabulary* b, int32_t level, int32_t pass, int32_t* first_node,
                                   int32_t* n_level_nodes, int32_t* cluster, float* centre) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "vocabulary_debug_lloyd", sim3opt::NO_MEMORY,
                          [&] { return b->debug_lloyd(level, pass, first_node, n_level_nodes, cluster, centre); });
}

int sim3opt_vocabulary_save(const char* path, int32_t n_nodes, const int32_t* parent, const float* centre,
                            const double* weight, const int32_t* word_id) {
  try {
    const std::string e = sim3opt_vocab::save_file(path, n_nodes, parent, centre, weight, word_id);
    if (e.empty()) return SIM3OPT_OK;
    return e == sim3opt_vocab::MSG_FILE_OPEN || e == sim3opt_vocab::MSG_FILE_WRITE ? SIM3OPT_ERR_IO : SIM3OPT_ERR_ARG;
  } catch (...) {
    return SIM3OPT_ERR_ARG;
  }
}

int sim3opt_vocabulary_load(const char* path, int32_t* n_nodes, int32_t** parent, float** centre, double** weight,
                            int32_t** word_id) {
  if (!path || !n_nodes || !parent || !centre || !weight || !word_id) return SIM3OPT_ERR_ARG;
  try {
    std::vector<int32_t> p, w;
    std::vector<float> c;
    std::vector<double> g;
    if (!sim3opt_vocab::load_file(path, p, c, g, w).empty()) return SIM3OPT_ERR_IO;
    const size_t n = p.size();
    int32_t* op = (int32_t*)std::malloc(sizeof(int32_t) * n);
    int32_t* ow = (int32_t*)std::malloc(sizeof(int32_t) * n);
    float* oc = (float*)std::malloc(sizeof(float) * c.size());
    double* og = (double*)std::malloc(sizeof(double) * n);
    if (!op || !ow || !oc || !og) { std::free(op); std::free(ow); std::free(oc); std::free(og); return SIM3OPT_ERR_ARG; }
    std::memcpy(op, p.data(), sizeof(int32_t) * n); std::memcpy(ow, w.data(), sizeof(int32_t) * n);
    std::memcpy(oc, c.data(), sizeof(float) * c.size()); std::memcpy(og, g.data(), sizeof(double) * n);
    *n_nodes = (int32_t)n; *parent = op; *centre = oc; *weight = og; *word_id = ow;
    return SIM3OPT_OK;
  } catch (...) {
    return SIM3OPT_ERR_ARG;
  }
}

void sim3opt_vocabulary_free(void* p) { std::free(p); }

}  // extern "C"
