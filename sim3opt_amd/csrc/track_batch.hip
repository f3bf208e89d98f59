// track_batch.hip -- batched loop tracks: the kept matches of all loop pairs fused into multi-view tracks, one 3-D point
// per track in the corrected world, and the obs_cam / obs_point / obs_uv rows sim3opt_ba_set_problem takes
// (SaveAsSfMInit's connection loop, kitti_surf.cpp:349-391, restated as connected components).  include/sim3opt.h
// ("batched loop tracks") is the specification; track_host.hpp holds the checks and the serial restatement,
// track_math.hpp the arithmetic both sides share.  DESIGN.md, section 5c.
//
//   k_track_init           every observation its own label; no smallest match, no depth key, no track yet
//   k_track_hook           a lane per kept match: the roots of its two sides, the larger hooked under the smaller by an
//                          integer atomicMin; a device flag says that something was hooked
//   k_track_jump           a lane per observation: its label becomes its root
//                          (the two are relaunched until the flag stays clear: the host reads one integer a round)
//   k_track_keys           per component the smallest kept match, per observation the lowest match that gives it a
//                          depth (integer atomicMin both)
//   k_track_heads          a match is its track's head when it is that smallest match
//   k_track_tile_sums / k_track_scan_tiles / k_track_scan_apply
//                          an ordered exclusive scan in tiles of SCAN_TILE with a carry across them: over the heads
//                          (the track numbers), over the tracks' lengths (track_ptr), over the kept tracks and their
//                          lengths (the bundle-adjustment rows)
//   k_track_number         the head gives its component the track number and the track its first match
//   k_track_count          the tracks' lengths (integer adds) and the track of every match
//   k_track_scatter        the observations into their segments, in arrival order
//   k_track_sort_lane / _wave / _workgroup
//                          every segment ascending in g, by rank (the keys are unique, so the bytes are a function of
//                          the inputs alone): up to LANE_MAX observations by a lane, up to WAVE_MAX by a wavefront,
//                          longer ones by a workgroup
//   k_track_points         a lane per track: track_math.hpp's point and status
//   k_track_ba             the status-0 tracks in order: their points and observation rows
// Integer atomics only; no floating-point atomic.  Within a launch nothing relies on one workgroup seeing another's
// plain stores: a label read during hooking may be an older one, which is a member of the same component and no
// smaller than the newest (labels only ever decrease towards the component's smallest g), so a round is correct
// whatever it sees, and the fixed point -- a round that hooks nothing, read after the launch has ended -- is unique.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "frames_host.hpp"
#include "handle_device.hpp"
#include "track_host.hpp"

namespace sim3opt_track {

static_assert(WORKGROUP == 256 && SCAN_TILE == WORKGROUP && WAVE_MAX == 64 && LANE_MAX < WAVE_MAX, "the kernels' tiles");
constexpr int WAVES = WORKGROUP / WAVE_MAX;

__device__ inline int32_t load_label(const int32_t* label, int32_t x) {
  return __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// label[x] <= x everywhere and always, so the walk ends
__device__ inline int32_t root_of(const int32_t* label, int32_t x) {
  for (int32_t p = load_label(label, x); p != x; p = load_label(label, x)) x = p;
  return x;
}

__global__ __launch_bounds__(WORKGROUP) void k_track_init(int32_t N, int32_t* label, int32_t* min_match, int32_t* dkey,
                                                          int32_t* track_of_root) {
  const int32_t g = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (g >= N) return;
  label[g] = g;
  min_match[g] = NONE;
  dkey[g] = NONE;
  track_of_root[g] = -1;
}

__global__ __launch_bounds__(WORKGROUP) void k_track_hook(int32_t M, const int32_t* ga, const int32_t* gb, int32_t* label,
                                                          int32_t* flag) {
  const int32_t m = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (m >= M || ga[m] < 0) return;
  const int32_t ra = root_of(label, ga[m]), rb = root_of(label, gb[m]);
  if (ra == rb) return;
  atomicMin(label + max(ra, rb), min(ra, rb));
  flag[0] = 1;  // (every writer writes the same value)
}

__global__ __launch_bounds__(WORKGROUP) void k_track_jump(int32_t N, int32_t* label) {
  const int32_t g = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (g >= N) return;
  const int32_t r = root_of(label, g);
  if (r != g) __hip_atomic_store(label + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(WORKGROUP) void k_track_keys(int32_t M, const int32_t* ga, const int32_t* gb,
                                                          const double* depth0, const double* depth1,
                                                          const int32_t* label, int32_t* min_match, int32_t* dkey) {
  const int32_t m = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (m >= M || ga[m] < 0) return;
  atomicMin(min_match + label[ga[m]], m);
  if (depth0 && depth_present(depth0[m])) atomicMin(dkey + ga[m], 2 * m);
  if (depth1 && depth_present(depth1[m])) atomicMin(dkey + gb[m], 2 * m + 1);
}

__global__ __launch_bounds__(WORKGROUP) void k_track_heads(int32_t M, const int32_t* ga, const int32_t* label,
                                                           const int32_t* min_match, int32_t* head) {
  const int32_t m = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (m >= M) return;
  head[m] = ga[m] >= 0 && min_match[label[ga[m]]] == m;
}

// exclusive prefix sum of v over the workgroup's lanes; total: the sum.  s: SCAN_TILE ints.
__device__ inline int32_t tile_excl_scan(int32_t v, int32_t* s, int32_t& total) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < SCAN_TILE; off <<= 1) {
    const int32_t x = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += x;
    __syncthreads();
  }
  const int32_t incl = s[tid];
  total = s[SCAN_TILE - 1];
  __syncthreads();  // s may be written again
  return incl - v;
}

__global__ __launch_bounds__(SCAN_TILE) void k_track_tile_sums(const int32_t* v, int32_t n, int32_t* tile_sum) {
  __shared__ int32_t sc[SCAN_TILE];
  const int32_t i = (int32_t)(blockIdx.x * SCAN_TILE + threadIdx.x);
  int32_t total;
  tile_excl_scan(i < n ? v[i] : 0, sc, total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: the tiles' exclusive offsets, SCAN_TILE of them at a time with a running carry, and the grand total
__global__ __launch_bounds__(SCAN_TILE) void k_track_scan_tiles(const int32_t* tile_sum, int32_t n_tiles, int32_t* tile_base,
                                                                int32_t* total_out) {
  __shared__ int32_t sc[SCAN_TILE];
  int32_t run = 0;
  for (int32_t i0 = 0; i0 < n_tiles; i0 += SCAN_TILE) {  // (uniform)
    const int32_t i = i0 + (int32_t)threadIdx.x;
    int32_t total;
    const int32_t excl = tile_excl_scan(i < n_tiles ? tile_sum[i] : 0, sc, total);
    if (i < n_tiles) tile_base[i] = run + excl;
    run += total;
  }
  if (threadIdx.x == 0) total_out[0] = run;
}

// excl: n + 1 entries, the last one the total
__global__ __launch_bounds__(SCAN_TILE) void k_track_scan_apply(const int32_t* v, int32_t n, const int32_t* tile_base,
                                                                const int32_t* total, int32_t* excl) {
  __shared__ int32_t sc[SCAN_TILE];
  const int32_t i = (int32_t)(blockIdx.x * SCAN_TILE + threadIdx.x);
  int32_t t;
  const int32_t e = tile_excl_scan(i < n ? v[i] : 0, sc, t);
  if (i < n) excl[i] = tile_base[blockIdx.x] + e;
  if (blockIdx.x == 0 && threadIdx.x == 0) excl[n] = total[0];
}

__global__ __launch_bounds__(WORKGROUP) void k_track_number(int32_t M, const int32_t* ga, const int32_t* label,
                                                            const int32_t* head, const int32_t* head_excl,
                                                            int32_t* track_of_root, int32_t* first_match) {
  const int32_t m = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (m >= M || !head[m]) return;
  const int32_t t = head_excl[m];  // (< the number of heads <= M)
  track_of_root[label[ga[m]]] = t;
  first_match[t] = m;
}

// a lane per observation and per match: n = max(N, M)
__global__ __launch_bounds__(WORKGROUP) void k_track_count(int32_t N, int32_t M, const int32_t* ga, const int32_t* label,
                                                           const int32_t* track_of_root, int32_t* count,
                                                           int32_t* match_track) {
  const int32_t i = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (i < N) {
    const int32_t t = track_of_root[label[i]];
    if (t >= 0) atomicAdd(count + t, 1);
  }
  if (i < M) match_track[i] = ga[i] >= 0 ? track_of_root[label[ga[i]]] : -1;
}

__global__ __launch_bounds__(WORKGROUP) void k_track_scatter(int32_t N, const int32_t* label, const int32_t* track_of_root,
                                                             const int32_t* track_ptr, int32_t* cursor, int32_t* unsorted) {
  const int32_t g = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (g >= N) return;
  const int32_t t = track_of_root[label[g]];
  if (t < 0) return;
  const int32_t at = atomicAdd(cursor + t, 1);  // (< the track's count: the same observations were counted)
  unsorted[track_ptr[t] + at] = g;
}

// The three orderings read `unsorted` and write `sorted`: the rank of a key is the number of smaller keys of its segment.
__global__ __launch_bounds__(WORKGROUP) void k_track_sort_lane(int32_t T, const int32_t* track_ptr, const int32_t* unsorted,
                                                               int32_t* sorted) {
  const int32_t t = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (t >= T) return;
  const int32_t p0 = track_ptr[t], len = track_ptr[t + 1] - p0;
  if (len > LANE_MAX) return;
  for (int32_t i = 0; i < len; ++i) {
    const int32_t key = unsorted[p0 + i];
    int32_t rank = 0;
    for (int32_t j = 0; j < len; ++j) rank += unsorted[p0 + j] < key;
    sorted[p0 + rank] = key;
  }
}

__global__ __launch_bounds__(WORKGROUP) void k_track_sort_wave(int32_t T, const int32_t* track_ptr, const int32_t* unsorted,
                                                               int32_t* sorted) {
  const int32_t t = (int32_t)(blockIdx.x * WAVES + threadIdx.x / WAVE_MAX), lane = (int32_t)(threadIdx.x % WAVE_MAX);
  if (t >= T) return;  // (the whole wavefront)
  const int32_t p0 = track_ptr[t], len = track_ptr[t + 1] - p0;
  if (len <= LANE_MAX || len > WAVE_MAX) return;  // (the whole wavefront)
  const int32_t key = lane < len ? unsorted[p0 + lane] : NONE;
  int32_t rank = 0;
  for (int32_t j = 0; j < len; ++j) rank += __shfl(key, j, WAVE_MAX) < key;
  if (lane < len) sorted[p0 + rank] = key;
}

__global__ __launch_bounds__(WORKGROUP) void k_track_sort_workgroup(int32_t T, const int32_t* track_ptr,
                                                                    const int32_t* unsorted, int32_t* sorted) {
  __shared__ int32_t s[WORKGROUP];
  const int32_t t = (int32_t)blockIdx.x, tid = (int32_t)threadIdx.x;
  if (t >= T) return;
  const int32_t p0 = track_ptr[t], len = track_ptr[t + 1] - p0;
  if (len <= WAVE_MAX) return;  // (the whole workgroup)
  for (int32_t i0 = 0; i0 < len; i0 += WORKGROUP) {  // (uniform)
    const int32_t i = i0 + tid;
    const int32_t key = i < len ? unsorted[p0 + i] : NONE;
    int32_t rank = 0;
    for (int32_t c0 = 0; c0 < len; c0 += WORKGROUP) {  // (uniform)
      __syncthreads();
      s[tid] = c0 + tid < len ? unsorted[p0 + c0 + tid] : NONE;
      __syncthreads();
      const int32_t nc = min(WORKGROUP, len - c0);
      for (int32_t j = 0; j < nc; ++j) rank += s[j] < key;
    }
    if (i < len) sorted[p0 + rank] = key;
  }
}

__global__ __launch_bounds__(WORKGROUP) void k_track_points(int32_t T, PointArgs A, const int32_t* track_ptr,
                                                            const int32_t* obs_g, double* points, int32_t* status,
                                                            int32_t* n_depths, int32_t* kept, int32_t* kept_len) {
  const int32_t t = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (t >= T) return;
  const int32_t p0 = track_ptr[t], len = track_ptr[t + 1] - p0;
  double X[3];
  int32_t nd;
  const int32_t st = track_point(A, obs_g + p0, len, X, nd);
  points[3 * (size_t)t] = X[0]; points[3 * (size_t)t + 1] = X[1]; points[3 * (size_t)t + 2] = X[2];
  status[t] = st;
  n_depths[t] = nd;
  kept[t] = st == TRACK_OK;
  kept_len[t] = st == TRACK_OK ? len : 0;
}

__global__ __launch_bounds__(WORKGROUP) void k_track_ba(int32_t T, const int32_t* kp_ptr, int32_t n_frames, const float* kp,
                                                        const int32_t* track_ptr, const int32_t* obs_g,
                                                        const double* points, const int32_t* kept, const int32_t* kept_rank,
                                                        const int32_t* ba_ptr, double* ba_points, int32_t* ba_cam,
                                                        int32_t* ba_point, double* ba_uv) {
  const int32_t t = (int32_t)(blockIdx.x * WORKGROUP + threadIdx.x);
  if (t >= T || !kept[t]) return;
  const int32_t r = kept_rank[t], p0 = track_ptr[t], len = track_ptr[t + 1] - p0, o0 = ba_ptr[t];
  for (int k = 0; k < 3; ++k) ba_points[3 * (size_t)r + k] = points[3 * (size_t)t + k];
  for (int32_t i = 0; i < len; ++i) {
    const int32_t g = obs_g[p0 + i];
    ba_cam[o0 + i] = frame_of(kp_ptr, n_frames, g);
    ba_point[o0 + i] = r;
    ba_uv[2 * (size_t)(o0 + i)] = (double)kp[2 * (size_t)g];
    ba_uv[2 * (size_t)(o0 + i) + 1] = (double)kp[2 * (size_t)g + 1];
  }
}

inline unsigned blocks(size_t n, int per = WORKGROUP) { return (unsigned)((n + per - 1) / per); }

struct Batch : sim3opt::BatchHandle {
  sim3opt_track_batch_options opt;
  // as set (the host copies a re-upload after release() reads)
  bool have_frames = false, have_matches = false, have_cams = false;
  std::vector<int32_t> kp_ptr, ga, gb;
  std::vector<float> kp;  // (empty with a snapshot)
  std::vector<double> depth0, depth1, states;
  bool has_depth0 = false, has_depth1 = false;
  int32_t n_pairs = 0;
  double focal = 0, cx = 0, cy = 0;
  sim3opt_fstore::SnapshotRef snap;  // set_frames_from: kp_ptr / kp of dev are the snapshot's, not frame_mem's
  // the last solve
  Tracks res;
  std::vector<int32_t> obs_frame, obs_keypoint, ba_cam, ba_point;
  std::vector<double> ba_points, ba_uv;
  int32_t rounds = 0, n_kept = 0, n_kept_obs = 0;
  // device
  sim3opt::DevArena frame_mem, match_mem, work;
  struct Dev {
    const int32_t* kp_ptr; const float* kp;
    double* states;
    int32_t *ga, *gb;
    double *depth0, *depth1;
    bool frames_up, cams_up, matches_up;
    size_t work_N, work_M;  // the sizes the work blocks were made for (0, 0: none)
    int32_t *label, *min_match, *dkey, *track_of_root;                        // N
    int32_t *head, *head_excl, *match_track, *first_match;                   // M (+ 1)
    int32_t *count, *track_ptr, *cursor, *status, *n_depths, *kept, *kept_rank, *kept_len, *ba_ptr;  // M (+ 1)
    int32_t *unsorted, *obs_g, *ba_cam, *ba_point;                           // O = min(N, 2 M)
    double *points, *ba_points, *ba_uv;
    int32_t *tile_sum, *tile_base, *counts;                                  // tiles of M; COUNTS
  } dev{};
  enum { C_FLAG, C_TRACKS, C_OBS, C_KEPT, C_KEPT_OBS, COUNTS };

  ~Batch() { release(); }
  void release() {
    close_stream(frame_mem, match_mem, work);
    dev = Dev{};
  }
  size_t N() const { return (size_t)kp_ptr.back(); }
  int32_t n_frames() const { return (int32_t)kp_ptr.size() - 1; }

  int ensure_device() {
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    if (!stream)
      if (int rc = open_stream()) return rc;
    return SIM3OPT_OK;
  }

  int upload() {
    const size_t n = N(), M = ga.size(), nf = (size_t)n_frames();
    if (!dev.frames_up) {
      wait();
      frame_mem.release();
      dev.cams_up = false;
      if (snap) {
        dev.kp_ptr = snap->d_kp_ptr; dev.kp = snap->d_kp;
      } else {
        HIPCHK(frame_mem.upload(dev.kp_ptr, kp_ptr, stream, nullptr));
        HIPCHK(frame_mem.upload(dev.kp, kp, stream, nullptr));
      }
      HIPCHK(frame_mem.raw(dev.states, 8 * nf));
      dev.frames_up = true;
    }
    if (!dev.cams_up) {
      HIPCHK(hipMemcpyAsync(dev.states, states.data(), sizeof(double) * 8 * nf, hipMemcpyHostToDevice, stream));
      dev.cams_up = true;
    }
    if (!dev.matches_up) {
      wait();
      match_mem.release();
      HIPCHK(match_mem.upload(dev.ga, ga, stream, nullptr));
      HIPCHK(match_mem.upload(dev.gb, gb, stream, nullptr));
      dev.depth0 = dev.depth1 = nullptr;
      if (has_depth0) HIPCHK(match_mem.upload(dev.depth0, depth0, stream, nullptr));
      if (has_depth1) HIPCHK(match_mem.upload(dev.depth1, depth1, stream, nullptr));
      dev.matches_up = true;
    }
    if (dev.work_N != n || dev.work_M != M || !dev.counts) {
      wait();
      work.release();
      const size_t O = std::min(n, 2 * M);
      HIPCHK(work.raw(dev.label, n)); HIPCHK(work.raw(dev.min_match, n)); HIPCHK(work.raw(dev.dkey, n));
      HIPCHK(work.raw(dev.track_of_root, n));
      HIPCHK(work.raw(dev.head, M)); HIPCHK(work.raw(dev.head_excl, M + 1)); HIPCHK(work.raw(dev.match_track, M));
      HIPCHK(work.raw(dev.first_match, M));
      HIPCHK(work.raw(dev.count, M)); HIPCHK(work.raw(dev.track_ptr, M + 1)); HIPCHK(work.raw(dev.cursor, M));
      HIPCHK(work.raw(dev.status, M)); HIPCHK(work.raw(dev.n_depths, M)); HIPCHK(work.raw(dev.kept, M));
      HIPCHK(work.raw(dev.kept_rank, M + 1)); HIPCHK(work.raw(dev.kept_len, M)); HIPCHK(work.raw(dev.ba_ptr, M + 1));
      HIPCHK(work.raw(dev.unsorted, O)); HIPCHK(work.raw(dev.obs_g, O)); HIPCHK(work.raw(dev.ba_cam, O));
      HIPCHK(work.raw(dev.ba_point, O));
      HIPCHK(work.raw(dev.points, 3 * M)); HIPCHK(work.raw(dev.ba_points, 3 * M)); HIPCHK(work.raw(dev.ba_uv, 2 * O));
      HIPCHK(work.raw(dev.tile_sum, (size_t)blocks(M, SCAN_TILE))); HIPCHK(work.raw(dev.tile_base, (size_t)blocks(M, SCAN_TILE)));
      HIPCHK(work.raw(dev.counts, (size_t)COUNTS));
      dev.work_N = n; dev.work_M = M;
    }
    return SIM3OPT_OK;
  }

  // excl[0 .. n] = the exclusive scan of v[0 .. n) and its total, which also goes to counts[slot]; n <= M
  int scan(const int32_t* v, int32_t n, int32_t* excl, int slot) {
    if (n == 0) {
      HIPCHK(hipMemsetAsync(excl, 0, sizeof(int32_t), stream));
      HIPCHK(hipMemsetAsync(dev.counts + slot, 0, sizeof(int32_t), stream));
      return SIM3OPT_OK;
    }
    const unsigned tiles = blocks((size_t)n, SCAN_TILE);
    hipLaunchKernelGGL(k_track_tile_sums, dim3(tiles), dim3(SCAN_TILE), 0, stream, v, n, dev.tile_sum);
    hipLaunchKernelGGL(k_track_scan_tiles, dim3(1), dim3(SCAN_TILE), 0, stream, dev.tile_sum, (int32_t)tiles, dev.tile_base,
                       dev.counts + slot);
    hipLaunchKernelGGL(k_track_scan_apply, dim3(tiles), dim3(SCAN_TILE), 0, stream, v, n, dev.tile_base, dev.counts + slot,
                       excl);
    HIPCHK(hipGetLastError());
    return SIM3OPT_OK;
  }

  int solve() {
    const int rc = solve_body();
    wait();
    if (rc < 0) have_run = false;
    return rc;
  }

  int solve_body() {
    err.clear();
    if (!have_frames || !have_matches || !have_cams) {
      err = std::string("track_batch_solve: ") + (!have_frames ? "no frames" : !have_matches ? "no matches" : "no cameras") + " set";
      return SIM3OPT_ERR_STATE;
    }
    if (int rc = ensure_device()) return rc;
    if (snap)
      if (int rc = sim3opt_fstore::check_snapshot_device(*snap, "track_batch_solve", opt.device, err)) return rc;
    if (int rc = upload()) return rc;
    const int32_t n = (int32_t)N(), M = (int32_t)ga.size(), nf = n_frames();
    Tracks out;
    int32_t T = 0, n_obs = 0, used = 0;
    std::vector<int32_t> og, bc, bp, counts;
    std::vector<double> bpts, buv;
    if (n && M) {
      hipLaunchKernelGGL(k_track_init, dim3(blocks(n)), dim3(WORKGROUP), 0, stream, n, dev.label, dev.min_match, dev.dkey,
                         dev.track_of_root);
      for (;;) {  // a round: hook, jump, one integer read
        if (used == opt.max_rounds) {
          err = "track_batch_solve: the components did not settle in max_rounds = " + std::to_string(opt.max_rounds) + " rounds";
          return SIM3OPT_ERR_ARG;
        }
        int32_t flag = 0;
        HIPCHK(hipMemsetAsync(dev.counts + C_FLAG, 0, sizeof(int32_t), stream));
        hipLaunchKernelGGL(k_track_hook, dim3(blocks(M)), dim3(WORKGROUP), 0, stream, M, dev.ga, dev.gb, dev.label,
                           dev.counts + C_FLAG);
        hipLaunchKernelGGL(k_track_jump, dim3(blocks(n)), dim3(WORKGROUP), 0, stream, n, dev.label);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&flag, dev.counts + C_FLAG, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        ++used;
        if (!flag) break;
      }
      hipLaunchKernelGGL(k_track_keys, dim3(blocks(M)), dim3(WORKGROUP), 0, stream, M, dev.ga, dev.gb, dev.depth0, dev.depth1,
                         dev.label, dev.min_match, dev.dkey);
      hipLaunchKernelGGL(k_track_heads, dim3(blocks(M)), dim3(WORKGROUP), 0, stream, M, dev.ga, dev.label, dev.min_match,
                         dev.head);
      if (int rc = scan(dev.head, M, dev.head_excl, C_TRACKS)) return rc;
      hipLaunchKernelGGL(k_track_number, dim3(blocks(M)), dim3(WORKGROUP), 0, stream, M, dev.ga, dev.label, dev.head,
                         dev.head_excl, dev.track_of_root, dev.first_match);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(&T, dev.counts + C_TRACKS, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      if (T < 0 || T > M) { err = "track_batch_solve: internal error (the track count)"; return SIM3OPT_ERR_HIP; }
      HIPCHK(hipMemsetAsync(dev.count, 0, sizeof(int32_t) * (size_t)std::max(T, 1), stream));
      HIPCHK(hipMemsetAsync(dev.cursor, 0, sizeof(int32_t) * (size_t)std::max(T, 1), stream));
      hipLaunchKernelGGL(k_track_count, dim3(blocks((size_t)std::max(n, M))), dim3(WORKGROUP), 0, stream, n, M, dev.ga,
                         dev.label, dev.track_of_root, dev.count, dev.match_track);
      if (int rc = scan(dev.count, T, dev.track_ptr, C_OBS)) return rc;
      if (T) {
        hipLaunchKernelGGL(k_track_scatter, dim3(blocks(n)), dim3(WORKGROUP), 0, stream, n, dev.label, dev.track_of_root,
                           dev.track_ptr, dev.cursor, dev.unsorted);
        hipLaunchKernelGGL(k_track_sort_lane, dim3(blocks(T)), dim3(WORKGROUP), 0, stream, T, dev.track_ptr, dev.unsorted,
                           dev.obs_g);
        hipLaunchKernelGGL(k_track_sort_wave, dim3(blocks(T, WAVES)), dim3(WORKGROUP), 0, stream, T, dev.track_ptr,
                           dev.unsorted, dev.obs_g);
        hipLaunchKernelGGL(k_track_sort_workgroup, dim3((unsigned)T), dim3(WORKGROUP), 0, stream, T, dev.track_ptr,
                           dev.unsorted, dev.obs_g);
        const PointArgs A{dev.kp_ptr, nf, dev.kp, dev.dkey, dev.depth0, dev.depth1, dev.states, focal, cx, cy,
                          opt.max_reproj_px};
        hipLaunchKernelGGL(k_track_points, dim3(blocks(T)), dim3(WORKGROUP), 0, stream, T, A, dev.track_ptr, dev.obs_g,
                           dev.points, dev.status, dev.n_depths, dev.kept, dev.kept_len);
      }
      if (int rc = scan(dev.kept, T, dev.kept_rank, C_KEPT)) return rc;
      if (int rc = scan(dev.kept_len, T, dev.ba_ptr, C_KEPT_OBS)) return rc;
      if (T)
        hipLaunchKernelGGL(k_track_ba, dim3(blocks(T)), dim3(WORKGROUP), 0, stream, T, dev.kp_ptr, nf, dev.kp, dev.track_ptr,
                           dev.obs_g, dev.points, dev.kept, dev.kept_rank, dev.ba_ptr, dev.ba_points, dev.ba_cam,
                           dev.ba_point, dev.ba_uv);
      HIPCHK(hipGetLastError());
      HIPCHK(sim3opt::read_back(counts, dev.counts, (size_t)COUNTS, stream));
      HIPCHK(sim3opt::read_back(out.track_ptr, dev.track_ptr, (size_t)T + 1, stream));
      HIPCHK(sim3opt::read_back(out.status, dev.status, (size_t)T, stream));
      HIPCHK(sim3opt::read_back(out.first_match, dev.first_match, (size_t)T, stream));
      HIPCHK(sim3opt::read_back(out.n_depths, dev.n_depths, (size_t)T, stream));
      HIPCHK(sim3opt::read_back(out.points, dev.points, 3 * (size_t)T, stream));
      HIPCHK(sim3opt::read_back(out.match_track, dev.match_track, (size_t)M, stream));
      HIPCHK(hipStreamSynchronize(stream));
      n_obs = counts[C_OBS];
      const size_t O = std::min((size_t)n, 2 * (size_t)M);
      if (n_obs < 0 || (size_t)n_obs > O || counts[C_KEPT] < 0 || counts[C_KEPT] > T || counts[C_KEPT_OBS] < 0 ||
          counts[C_KEPT_OBS] > n_obs || out.track_ptr[T] != n_obs) {
        err = "track_batch_solve: internal error (the observation counts)";
        return SIM3OPT_ERR_HIP;
      }
      HIPCHK(sim3opt::read_back(out.obs_g, dev.obs_g, (size_t)n_obs, stream));
      HIPCHK(sim3opt::read_back(bc, dev.ba_cam, (size_t)counts[C_KEPT_OBS], stream));
      HIPCHK(sim3opt::read_back(bp, dev.ba_point, (size_t)counts[C_KEPT_OBS], stream));
      HIPCHK(sim3opt::read_back(buv, dev.ba_uv, 2 * (size_t)counts[C_KEPT_OBS], stream));
      HIPCHK(sim3opt::read_back(bpts, dev.ba_points, 3 * (size_t)counts[C_KEPT], stream));
      HIPCHK(hipStreamSynchronize(stream));
    } else {
      out.track_ptr.assign(1, 0);
      out.match_track.assign((size_t)M, -1);
      counts.assign((size_t)COUNTS, 0);
    }
    std::vector<int32_t> of((size_t)n_obs), ok((size_t)n_obs);
    split_observations(nf, kp_ptr.data(), out.obs_g.data(), (size_t)n_obs, of.data(), ok.data());
    // nothing failed: the handle changes now
    res = std::move(out);
    obs_frame.swap(of); obs_keypoint.swap(ok);
    ba_cam.swap(bc); ba_point.swap(bp); ba_uv.swap(buv); ba_points.swap(bpts);
    rounds = used; n_kept = counts[C_KEPT]; n_kept_obs = counts[C_KEPT_OBS];
    have_run = true;
    return n_kept;
  }
};

}  // namespace sim3opt_track

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched loop tracks")
// ------------------------------------------------------------------------------------------
struct sim3opt_track_batch : sim3opt_track::Batch {};

namespace {

template <class T>
void copy_out(T* dst, const std::vector<T>& src) {
  if (dst && !src.empty()) std::memcpy(dst, src.data(), sizeof(T) * src.size());
}

int need_run(sim3opt_track_batch* b, const char* who) {
  if (b->have_run) return SIM3OPT_OK;
  b->err = std::string(who) + ": no solve yet";
  return SIM3OPT_ERR_STATE;
}

}  // namespace

extern "C" {

void sim3opt_track_batch_options_default(sim3opt_track_batch_options* o) {
  if (!o) return;
  o->max_reproj_px = 0.0;
  o->max_rounds = 64;
  o->device = -1;
}

sim3opt_track_batch* sim3opt_track_batch_create(void) {
  return sim3opt::handle_create<sim3opt_track_batch>(sim3opt_track_batch_options_default);
}

void sim3opt_track_batch_destroy(sim3opt_track_batch* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_track_batch_last_error(const sim3opt_track_batch* b) { return b ? b->err.c_str() : "null batch"; }

int sim3opt_track_batch_set_options(sim3opt_track_batch* b, const sim3opt_track_batch_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  if (!(o->max_reproj_px >= 0.0) || !std::isfinite(o->max_reproj_px)) {
    b->err = "track_batch_set_options: max_reproj_px must be finite and >= 0";
    return SIM3OPT_ERR_ARG;
  }
  if (o->max_rounds < 1) { b->err = "track_batch_set_options: max_rounds < 1"; return SIM3OPT_ERR_ARG; }
  if (o->device < -1) { b->err = "track_batch_set_options: device below -1"; return SIM3OPT_ERR_ARG; }
  if (o->device != b->opt.device) {  // the device is chosen at the next solve; a snapshot stays on its own
    if (b->snap) { b->err = "track_batch_set_options: another device while a store's snapshot is held"; return SIM3OPT_ERR_ARG; }
    b->release();
  }
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_track_batch_set_frames(sim3opt_track_batch* b, int32_t n_frames, const int32_t* kp_ptr, const float* kp) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "track_batch_set_frames", sim3opt::NO_MEMORY, [&]() -> int {
    const std::string e = sim3opt_track::validate_frames(n_frames, kp_ptr, kp);
    if (!e.empty()) { b->err = "track_batch_set_frames: " + e; return SIM3OPT_ERR_ARG; }
    std::vector<int32_t> kpp(kp_ptr, kp_ptr + n_frames + 1);
    std::vector<float> k(kp, kp + 2 * (size_t)kp_ptr[n_frames]);
    // nothing failed: the handle changes now
    b->wait();
    b->kp_ptr.swap(kpp); b->kp.swap(k);
    b->snap.reset();
    b->have_frames = true;
    b->have_matches = b->have_cams = b->have_run = false;
    b->dev.frames_up = b->dev.matches_up = b->dev.cams_up = false;
    return SIM3OPT_OK;
  });
}

int sim3opt_track_batch_set_frames_from(sim3opt_track_batch* b, const sim3opt_frames* store) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "track_batch_set_frames_from", sim3opt::NO_MEMORY, [&]() -> int {
    sim3opt_fstore::SnapshotRef s;
    if (int rc = sim3opt_fstore::take_snapshot(store, "track_batch_set_frames_from", b->opt.device, s, b->err)) return rc;
    std::vector<int32_t> kpp(s->kp_ptr);
    b->wait();
    b->kp_ptr.swap(kpp);
    std::vector<float>().swap(b->kp);
    b->snap = std::move(s);
    b->have_frames = true;
    b->have_matches = b->have_cams = b->have_run = false;
    b->dev.frames_up = b->dev.matches_up = b->dev.cams_up = false;
    return SIM3OPT_OK;
  });
}

int sim3opt_track_batch_set_matches(sim3opt_track_batch* b, int32_t n_pairs, const int32_t* pairs, const int32_t* match_ptr,
                                    const int32_t* query_idx, const int32_t* train_idx, const uint8_t* mask,
                                    const double* depth0, const double* depth1) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "track_batch_set_matches", sim3opt::NO_MEMORY, [&]() -> int {
    if (!b->have_frames) { b->err = "track_batch_set_matches: no frames set"; return SIM3OPT_ERR_STATE; }
    std::vector<int32_t> ga, gb;
    const std::string e = sim3opt_track::validate_matches(b->n_frames(), b->kp_ptr.data(), n_pairs, pairs, match_ptr,
                                                          query_idx, train_idx, mask, ga, gb);
    if (!e.empty()) { b->err = "track_batch_set_matches: " + e; return SIM3OPT_ERR_ARG; }
    const size_t M = ga.size();
    std::vector<double> d0, d1;
    if (depth0) d0.assign(depth0, depth0 + M);
    if (depth1) d1.assign(depth1, depth1 + M);
    b->wait();
    b->ga.swap(ga); b->gb.swap(gb); b->depth0.swap(d0); b->depth1.swap(d1);
    b->has_depth0 = depth0 != nullptr; b->has_depth1 = depth1 != nullptr;
    b->n_pairs = n_pairs;
    b->have_matches = true;
    b->have_run = false;
    b->dev.matches_up = false;
    return SIM3OPT_OK;
  });
}

int sim3opt_track_batch_set_cameras(sim3opt_track_batch* b, int32_t n_frames, const double* states, double focal, double cx,
                                    double cy) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "track_batch_set_cameras", sim3opt::NO_MEMORY, [&]() -> int {
    if (!b->have_frames) { b->err = "track_batch_set_cameras: no frames set"; return SIM3OPT_ERR_STATE; }
    const std::string e = sim3opt_track::validate_cameras(n_frames, b->n_frames(), states, focal, cx, cy);
    if (!e.empty()) { b->err = "track_batch_set_cameras: " + e; return SIM3OPT_ERR_ARG; }
    std::vector<double> st(states, states + 8 * (size_t)n_frames);
    b->wait();
    b->states.swap(st);
    b->focal = focal; b->cx = cx; b->cy = cy;
    b->have_cams = true;
    b->have_run = false;
    b->dev.cams_up = false;
    return SIM3OPT_OK;
  });
}

int sim3opt_track_batch_solve(sim3opt_track_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "track_batch_solve", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve(); });
}

int sim3opt_track_batch_dims(const sim3opt_track_batch* b, int32_t* n_frames, int32_t* n_pairs, int32_t* total_matches,
                             int32_t* n_tracks, int32_t* n_observations, int32_t* n_kept_tracks,
                             int32_t* n_kept_observations, int32_t* rounds, int32_t tiles[4]) {
  if (!b) return SIM3OPT_ERR_ARG;
  const bool run = b->have_run;
  if (n_frames) *n_frames = b->have_frames ? b->n_frames() : 0;
  if (n_pairs) *n_pairs = b->have_matches ? b->n_pairs : 0;
  if (total_matches) *total_matches = b->have_matches ? (int32_t)b->ga.size() : 0;
  if (n_tracks) *n_tracks = run ? b->res.n_tracks() : 0;
  if (n_observations) *n_observations = run ? (int32_t)b->res.obs_g.size() : 0;
  if (n_kept_tracks) *n_kept_tracks = run ? b->n_kept : 0;
  if (n_kept_observations) *n_kept_observations = run ? b->n_kept_obs : 0;
  if (rounds) *rounds = run ? b->rounds : 0;
  if (tiles) {
    tiles[0] = sim3opt_track::WORKGROUP; tiles[1] = sim3opt_track::SCAN_TILE;
    tiles[2] = sim3opt_track::LANE_MAX; tiles[3] = sim3opt_track::WAVE_MAX;
  }
  return SIM3OPT_OK;
}

int sim3opt_track_batch_get_tracks(sim3opt_track_batch* b, int32_t* track_ptr, int32_t* obs_frame, int32_t* obs_keypoint,
                                   int32_t* status, int32_t* first_match) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (int rc = need_run(b, "track_batch_get_tracks")) return rc;
  copy_out(track_ptr, b->res.track_ptr); copy_out(obs_frame, b->obs_frame); copy_out(obs_keypoint, b->obs_keypoint);
  copy_out(status, b->res.status); copy_out(first_match, b->res.first_match);
  return SIM3OPT_OK;
}

int sim3opt_track_batch_get_match_track(sim3opt_track_batch* b, int32_t* match_track) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (int rc = need_run(b, "track_batch_get_match_track")) return rc;
  copy_out(match_track, b->res.match_track);
  return SIM3OPT_OK;
}

int sim3opt_track_batch_get_points(sim3opt_track_batch* b, double* points, int32_t* n_depths) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (int rc = need_run(b, "track_batch_get_points")) return rc;
  copy_out(points, b->res.points); copy_out(n_depths, b->res.n_depths);
  return SIM3OPT_OK;
}

int sim3opt_track_batch_get_ba(sim3opt_track_batch* b, int32_t point_base, double* points, int32_t* obs_cam,
                               int32_t* obs_point, double* obs_uv) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (int rc = need_run(b, "track_batch_get_ba")) return rc;
  if (point_base < 0 || (int64_t)point_base + b->n_kept > INT32_MAX) {
    b->err = "track_batch_get_ba: point_base outside the int32 point indices";
    return SIM3OPT_ERR_ARG;
  }
  copy_out(points, b->ba_points); copy_out(obs_cam, b->ba_cam); copy_out(obs_uv, b->ba_uv);
  if (obs_point)
    for (size_t i = 0; i < b->ba_point.size(); ++i) obs_point[i] = point_base + b->ba_point[i];
  return SIM3OPT_OK;
}

int sim3opt_track_reference(int32_t n_frames, const int32_t* kp_ptr, const float* kp, int32_t n_pairs, const int32_t* pairs,
                            const int32_t* match_ptr, const int32_t* query_idx, const int32_t* train_idx,
                            const uint8_t* mask, const double* depth0, const double* depth1, const double* states,
                            double focal, double cx, double cy, double max_reproj_px, int32_t* n_tracks,
                            int32_t* n_observations, int32_t* track_ptr, int32_t* obs_frame, int32_t* obs_keypoint,
                            int32_t* status, int32_t* first_match, int32_t* match_track, double* points,
                            int32_t* n_depths) {
  try {
    namespace T = sim3opt_track;
    std::vector<int32_t> ga, gb;
    if (!T::validate_frames(n_frames, kp_ptr, kp).empty()) return SIM3OPT_ERR_ARG;
    if (!T::validate_matches(n_frames, kp_ptr, n_pairs, pairs, match_ptr, query_idx, train_idx, mask, ga, gb).empty())
      return SIM3OPT_ERR_ARG;
    if (!T::validate_cameras(n_frames, n_frames, states, focal, cx, cy).empty() || !(max_reproj_px >= 0.0))
      return SIM3OPT_ERR_ARG;
    T::Tracks r;
    T::reference_tracks(n_frames, kp_ptr, kp, ga, gb, depth0, depth1, states, focal, cx, cy, max_reproj_px, r);
    if (n_tracks) *n_tracks = r.n_tracks();
    if (n_observations) *n_observations = (int32_t)r.obs_g.size();
    copy_out(track_ptr, r.track_ptr); copy_out(status, r.status); copy_out(first_match, r.first_match);
    copy_out(match_track, r.match_track); copy_out(points, r.points); copy_out(n_depths, r.n_depths);
    T::split_observations(n_frames, kp_ptr, r.obs_g.data(), r.obs_g.size(), obs_frame, obs_keypoint);
    return SIM3OPT_OK;
  } catch (...) {
    return SIM3OPT_ERR_ARG;
  }
}

}  // extern "C"
