// surf_batch.hip -- the head of the detector chain: grey images in; kp_ptr, kp and the 64-float descriptors out, in the
// layout sim3opt_match_batch_set_frames, sim3opt_place_batch_set_frames and sim3opt_vocabulary_set_frames take
// (SurfExtractor::operator(), kitti_surf.cpp:501-523: cv::xfeatures2d::SURF::create(400), detect + compute).
// include/sim3opt.h ("batched SURF-64 extraction") holds the definition the kernels follow and says what of it is the
// call site's and what is recalled from upstream.  surf_host.hpp holds the per-item arithmetic, compiled here for the
// device and there for the serial restatement: one statement of every operation, so the two agree bit for bit.
//
// A pass takes up to images_per_pass images; its launches do not depend on how many:
//   k_surf_rows, k_surf_cols   the int32 integral images: a wavefront per row carrying the running total, then a lane
//                              per column
//   k_surf_detect<COUNT>       a workgroup per 32 x 32 tile of one octave's plane of one image: det of every layer for
//                              the tile and a one-sample halo into LDS, the 26-neighbour test from LDS; the tile's count
//   k_surf_scan_tiles/_images  exclusive offsets of the tiles within their image, of the images within the pass
//   k_surf_detect<EMIT>        the same, then a scan over the workgroup's lanes: every maximum is interpolated and
//                              written at its offset with its scan index.  The response planes never leave LDS.
//   k_surf_rank                the place of a kept candidate is the number of kept candidates of its image that rank
//                              before it (response descending, scan index ascending), the keys staged through LDS in
//                              tiles of 256; the scatter applies max_keypoints
//   k_surf_describe            a wavefront per keypoint: the 113 orientation samples and the 72 windows across lanes,
//                              the 441 patch cells across lanes (each lane walks its cell's window samples; the window
//                              is never stored), the 16 sub-regions in fixed order
// The host reads the candidate counts of the pass once (to size the candidate blocks: no capacity is guessed) and drops
// the keypoints the orientation step refused while it copies the results out, in order.  solve_into leaves kp and the
// descriptors on the device: the ordered compaction of frames.hip does that dropping for them, a chunk per pass, and the
// chunks are joined once into the frame store's snapshot.
// No floating-point atomic; the integer atomics count (kept, dropped) and decide no order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "frames_device.hpp"
#include "handle_device.hpp"
#include "surf_host.hpp"

#pragma clang fp contract(off)

namespace sim3opt_surf {

static_assert(TILE * TILE == 4 * DET_THREADS && RANK_TILE == DET_THREADS && KP_LANES == 64, "tile sizes");
constexpr int HALO = TILE + 2;
enum Mode : int { COUNT = 0, EMIT = 1, DUMP = 2 };

struct DetArgs {
  const int32_t* S;
  int32_t w, h, n_octaves, nl;
  float thr;
  int32_t tiles_per_image;
  int32_t oct_tile0[MAX_OCTAVES + 1], oct_tx[MAX_OCTAVES];
  int32_t* tile_count;
  const int32_t *tile_off, *cand_ptr;
  Cand* cand;
  int32_t dump_octave, dump_layer;
  float *dump_det, *dump_trace;
};

struct DescArgs {
  const uint8_t* img;
  const int32_t* S;
  int32_t w, h, upright;
  const Tables* T;
  const float *slot_kp, *slot_size;
  const int32_t* slot_img;
  int32_t* slot_state;  // 0: no keypoint, 1: ranked, 2: described, 3: dropped at the orientation step
  float *slot_angle, *slot_desc;
  int32_t* n_dropped;
  int32_t dump_slot;
  int32_t* d_valid;
  float *d_vx, *d_vy, *d_ang, *d_win, *d_patch;
};

// ---- integral images
__global__ __launch_bounds__(64) void k_surf_rows(const uint8_t* img, int32_t* S, int32_t w, int32_t h) {
  const int32_t y = blockIdx.x, lane = threadIdx.x;
  const uint8_t* row = img + ((size_t)blockIdx.y * (size_t)h + (size_t)y) * (size_t)w;
  int32_t* out = S + ((size_t)blockIdx.y * (size_t)(h + 1) + (size_t)(y + 1)) * (size_t)(w + 1);
  if (lane == 0) out[0] = 0;
  int32_t run = 0;
  for (int32_t x0 = 0; x0 < w; x0 += 64) {
    const int32_t x = x0 + lane;
    int32_t v = x < w ? (int32_t)row[x] : 0;
    for (int off = 1; off < 64; off <<= 1) {
      const int32_t t = __shfl_up(v, off, 64);
      if (lane >= off) v += t;
    }
    if (x < w) out[x + 1] = run + v;
    run += __shfl(v, 63, 64);
  }
}

__global__ __launch_bounds__(DET_THREADS) void k_surf_cols(int32_t* S, int32_t w, int32_t h) {
  const int32_t x = (int32_t)(blockIdx.x * DET_THREADS + threadIdx.x);
  if (x > w) return;
  int32_t* col = S + (size_t)blockIdx.y * (size_t)(h + 1) * (size_t)(w + 1) + (size_t)x;
  int32_t acc = 0;
  col[0] = 0;
  for (int32_t y = 1; y <= h; ++y) {
    acc += col[(size_t)y * (size_t)(w + 1)];
    col[(size_t)y * (size_t)(w + 1)] = acc;
  }
}

// exclusive prefix sum of v over the workgroup's 256 lanes; total: the sum.  s: 256 ints.
__device__ inline int32_t block_excl_scan(int32_t v, int32_t* s, int32_t& total) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < DET_THREADS; off <<= 1) {
    const int32_t x = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += x;
    __syncthreads();
  }
  const int32_t incl = s[tid];
  total = s[DET_THREADS - 1];
  __syncthreads();  // s may be written again
  return incl - v;
}

// ---- detection
__device__ inline bool tile_is_max(const float (*det)[HALO][HALO], int l, int r, int c, float thr) {
  const float v = det[l][r][c];
  if (!(v > thr)) return false;
#pragma unroll
  for (int q = -1; q <= 1; ++q)
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj)
        if ((q != 0 || di != 0 || dj != 0) && !(v > det[l + q][r + di][c + dj])) return false;
  return true;
}

template <int MODE>
__global__ __launch_bounds__(DET_THREADS) void k_surf_detect(DetArgs A) {
  __shared__ float det[MAX_LAYERS][HALO][HALO];
  __shared__ Box bx[MAX_LAYERS][N_BOXES];
  __shared__ int32_t sc[DET_THREADS];
  const int tid = threadIdx.x;
  const int32_t image = (int32_t)(blockIdx.x / (unsigned)A.tiles_per_image), t = (int32_t)(blockIdx.x % (unsigned)A.tiles_per_image);
  int o = 0;
  while (o + 1 < A.n_octaves && t >= A.oct_tile0[o + 1]) ++o;
  const int32_t tl = t - A.oct_tile0[o], ti = tl / A.oct_tx[o], tj = tl % A.oct_tx[o];
  const int step = 1 << o, rows = A.h >> o, cols = A.w >> o, nl2 = A.nl + 2;
  const int32_t* S = A.S + (size_t)image * (size_t)(A.h + 1) * (size_t)(A.w + 1);
  if (tid < nl2 * N_BOXES) {
    int src[5];
    hessian_pattern(tid % N_BOXES, src);
    bx[tid / N_BOXES][tid % N_BOXES] = resize_box(src, 9, layer_size(o, tid / N_BOXES));
  }
  __syncthreads();
  for (int idx = tid; idx < nl2 * HALO * HALO; idx += DET_THREADS) {
    const int l = idx / (HALO * HALO), rem = idx % (HALO * HALO), r = rem / HALO, c = rem % HALO;
    const int i = ti * TILE - 1 + r, j = tj * TILE - 1 + c;
    float d = 0.f, tr = 0.f;
    int y, x;
    if (i >= 0 && j >= 0 && i < rows && j < cols && plane_sample(A.w, A.h, layer_size(o, l), step, i, j, y, x))
      hessian_at(S, A.w + 1, y, x, bx[l], d, tr);
    det[l][r][c] = d;
  }
  __syncthreads();
  if (MODE == DUMP) {
    if (o == A.dump_octave && A.dump_layer >= 0 && A.dump_layer < nl2)
      for (int p = tid; p < TILE * TILE; p += DET_THREADS) {
        const int r = p / TILE + 1, c = p % TILE + 1, i = ti * TILE + r - 1, j = tj * TILE + c - 1;
        if (i >= rows || j >= cols) continue;
        float d = 0.f, tr = 0.f;
        int y, x;
        if (plane_sample(A.w, A.h, layer_size(o, A.dump_layer), step, i, j, y, x)) hessian_at(S, A.w + 1, y, x, bx[A.dump_layer], d, tr);
        A.dump_det[(size_t)i * (size_t)cols + (size_t)j] = det[A.dump_layer][r][c];
        A.dump_trace[(size_t)i * (size_t)cols + (size_t)j] = tr;
      }
  }
  int32_t cnt = 0;
  for (int l = 1; l <= A.nl; ++l) {
    const int margin = (layer_size(o, l + 1) / 2) / step + 1;
    for (int k = 0; k < 4; ++k) {
      const int p = tid + DET_THREADS * k, r = p / TILE + 1, c = p % TILE + 1, i = ti * TILE + r - 1, j = tj * TILE + c - 1;
      if (i >= margin && i < rows - margin && j >= margin && j < cols - margin && tile_is_max(det, l, r, c, A.thr)) ++cnt;
    }
  }
  int32_t total;
  const int32_t excl = block_excl_scan(cnt, sc, total);
  if (MODE != EMIT) {
    if (tid == 0) A.tile_count[blockIdx.x] = total;
    return;
  }
  Cand* out = A.cand + (size_t)A.cand_ptr[image] + (size_t)A.tile_off[blockIdx.x] + (size_t)excl;
  for (int l = 1; l <= A.nl; ++l) {
    const int margin = (layer_size(o, l + 1) / 2) / step + 1;
    for (int k = 0; k < 4; ++k) {
      const int p = tid + DET_THREADS * k, r = p / TILE + 1, c = p % TILE + 1, i = ti * TILE + r - 1, j = tj * TILE + c - 1;
      if (!(i >= margin && i < rows - margin && j >= margin && j < cols - margin && tile_is_max(det, l, r, c, A.thr))) continue;
      float N[3][9];
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int di = 0; di < 3; ++di)
#pragma unroll
          for (int dj = 0; dj < 3; ++dj) N[q][3 * di + dj] = det[l - 1 + q][r - 1 + di][c - 1 + dj];
      float d = 0.f, tr = 0.f;
      int y, x;
      if (plane_sample(A.w, A.h, layer_size(o, l), step, i, j, y, x)) hessian_at(S, A.w + 1, y, x, bx[l], d, tr);
      *out++ = make_candidate(N, tr, o, l, A.nl, i, j, A.w, A.h);
    }
  }
}

// per image: the exclusive offsets of its tiles in scan order, and its total
__global__ __launch_bounds__(DET_THREADS) void k_surf_scan_tiles(const int32_t* tile_count, int32_t* tile_off, int32_t* img_total,
                                                                 int32_t tiles_per_image) {
  __shared__ int32_t sc[DET_THREADS];
  const size_t base = (size_t)blockIdx.x * (size_t)tiles_per_image;
  int32_t run = 0;
  for (int32_t t0 = 0; t0 < tiles_per_image; t0 += DET_THREADS) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    const int32_t v = t < tiles_per_image ? tile_count[base + (size_t)t] : 0;
    int32_t total;
    const int32_t excl = block_excl_scan(v, sc, total);
    if (t < tiles_per_image) tile_off[base + (size_t)t] = run + excl;
    run += total;
  }
  if (threadIdx.x == 0) img_total[blockIdx.x] = run;
}

__global__ __launch_bounds__(DET_THREADS) void k_surf_scan_images(const int32_t* img_total, int32_t* cand_ptr, int32_t n) {
  __shared__ int32_t sc[DET_THREADS];
  int32_t run = 0;
  for (int32_t i0 = 0; i0 < n; i0 += DET_THREADS) {
    const int32_t i = i0 + (int32_t)threadIdx.x;
    const int32_t v = i < n ? img_total[i] : 0;
    int32_t total;
    const int32_t excl = block_excl_scan(v, sc, total);
    if (i < n) cand_ptr[i] = run + excl;
    run += total;
  }
  if (threadIdx.x == 0) cand_ptr[n] = run;
}

// ---- ranking: slot cand_ptr[image] + rank receives the kept candidate of that rank
__global__ __launch_bounds__(RANK_TILE) void k_surf_rank(const Cand* cand, const int32_t* cand_ptr, int32_t max_kp, float* slot_kp,
                                                         float* slot_size, float* slot_resp, int32_t* slot_oct, int32_t* slot_lap,
                                                         int32_t* slot_img, int32_t* slot_state, int32_t* n_kept) {
  __shared__ float sr[RANK_TILE];
  __shared__ int32_t sk[RANK_TILE];
  const int32_t image = blockIdx.y, lo = cand_ptr[image], hi = cand_ptr[image + 1], tid = threadIdx.x;
  const int32_t first = lo + (int32_t)blockIdx.x * RANK_TILE;
  if (first >= hi) return;  // (the whole workgroup)
  const int32_t idx = first + tid;
  Cand mine{};
  bool kept = false;
  if (idx < hi) { mine = cand[idx]; kept = mine.kept != 0; }
  int32_t rank = 0;
  for (int32_t base = lo; base < hi; base += RANK_TILE) {
    const int32_t e = base + tid;
    int32_t key = -1;
    float resp = 0.f;
    if (e < hi) { const Cand c = cand[e]; resp = c.response; key = c.kept ? c.key : -1; }
    sr[tid] = resp; sk[tid] = key;
    __syncthreads();
    const int32_t m = hi - base < RANK_TILE ? hi - base : RANK_TILE;
    if (kept)
      for (int32_t u = 0; u < m; ++u) rank += sk[u] >= 0 && ranks_before(sr[u], sk[u], mine.response, mine.key);
    __syncthreads();
  }
  const int nk = __syncthreads_count(kept);
  if (tid == 0 && nk) atomicAdd(&n_kept[image], nk);
  if (!kept || (max_kp > 0 && rank >= max_kp)) return;
  const size_t s = (size_t)lo + (size_t)rank;
  slot_kp[2 * s] = mine.x; slot_kp[2 * s + 1] = mine.y;
  slot_size[s] = mine.size; slot_resp[s] = mine.response;
  slot_oct[s] = mine.octave; slot_lap[s] = mine.laplacian;
  slot_img[s] = image; slot_state[s] = 1;
}

// ---- orientation and descriptor: one wavefront per slot
template <bool DUMPING>
__global__ __launch_bounds__(KP_LANES) void k_surf_describe(DescArgs A) {
  __shared__ KpGeometry G;
  __shared__ float vx[ORI_N], vy[ORI_N], ang[ORI_N];
  __shared__ int32_t ok[ORI_N];
  __shared__ float wm[ORI_WINDOWS], wsx[ORI_WINDOWS], wsy[ORI_WINDOWS];
  __shared__ float patch[PATCH * PATCH];
  __shared__ float d[DESC];
  const int lane = threadIdx.x;
  const size_t slot = DUMPING ? (size_t)A.dump_slot : (size_t)blockIdx.x;
  const int32_t state = A.slot_state[slot];
  if (DUMPING ? state == 0 : state != 1) return;  // (the whole workgroup)
  const int32_t image = A.slot_img[slot], w = A.w, h = A.h;
  const int32_t* S = A.S + (size_t)image * (size_t)(h + 1) * (size_t)(w + 1);
  const uint8_t* img = A.img + (size_t)image * (size_t)h * (size_t)w;
  const Tables& T = *A.T;
  const float cx = A.slot_kp[2 * slot], cy = A.slot_kp[2 * slot + 1];
  if (lane == 0) G = kp_geometry(A.slot_size[slot]);
  __syncthreads();
  float angle = 270.f;
  bool drop = false;
  if (!A.upright) {
    for (int k = lane; k < ORI_N; k += KP_LANES) {
      float x = 0.f, y = 0.f, a = 0.f;
      const bool v = ori_sample(S, w, h, cx, cy, G, T, k, x, y);
      if (v) a = fast_atan2(y, x);
      vx[k] = x; vy[k] = y; ang[k] = a; ok[k] = v;
      if (DUMPING) { A.d_valid[k] = v; A.d_vx[k] = x; A.d_vy[k] = y; A.d_ang[k] = a; }
    }
    __syncthreads();
    int n = 0;
    for (int k = 0; k < ORI_N; ++k) n += ok[k];
    drop = n == 0;
    if (!drop) {
      for (int c = lane; c < ORI_WINDOWS; c += KP_LANES) {
        float sx = 0.f, sy = 0.f;
        for (int k = 0; k < ORI_N; ++k)
          if (ok[k] && in_window(ang[k], 5 * c)) { sx = sx + vx[k]; sy = sy + vy[k]; }
        wsx[c] = sx; wsy[c] = sy; wm[c] = sx * sx + sy * sy;
        if (DUMPING) A.d_win[c] = wm[c];
      }
      __syncthreads();
      float best = 0.f, bx = 0.f, by = 0.f;
      for (int c = 0; c < ORI_WINDOWS; ++c)
        if (wm[c] > best) { best = wm[c]; bx = wsx[c]; by = wsy[c]; }
      angle = fast_atan2(-by, bx);
    }
  } else if (G.g > h + 1 || G.g > w + 1) {
    drop = true;
  }
  if (G.win < 1) drop = true;
  if (drop) {  // (uniform)
    if (!DUMPING && lane == 0) { A.slot_state[slot] = 3; atomicAdd(&A.n_dropped[image], 1); }
    return;
  }
  float sn, cs;
  sincos_deg(angle, sn, cs);
  for (int p = lane; p < PATCH * PATCH; p += KP_LANES) {
    patch[p] = patch_cell(img, w, h, cx, cy, -sn, cs, G.win, p / PATCH, p % PATCH);
    if (DUMPING) A.d_patch[p] = patch[p];
  }
  __syncthreads();
  if (DUMPING) return;
  if (lane < 16) {
    float o4[4];
    subregion_sums(patch, T, lane, o4);
    d[4 * lane] = o4[0]; d[4 * lane + 1] = o4[1]; d[4 * lane + 2] = o4[2]; d[4 * lane + 3] = o4[3];
  }
  __syncthreads();
  const float scale = descriptor_scale(d);
  A.slot_desc[slot * DESC + (size_t)lane] = d[lane] * scale;
  if (lane == 0) { A.slot_angle[slot] = angle; A.slot_state[slot] = 2; }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct PassOut {  // per image of a pass, appended in image order
  std::vector<int32_t> kp_ptr{0}, octave, laplacian, rank, status, n_cand, n_interp, n_dropped;
  std::vector<float> kp, desc, size, angle, response;
};

struct Fill {  // solve_into: the compacted kp / desc of the passes so far, on the device
  struct Chunk { float *kp, *desc; size_t rows; };
  std::vector<Chunk> chunks;
  size_t rows = 0;
};

struct Debug {  // what a read-out asks of a one-image pass
  std::vector<int32_t>* S = nullptr;
  int32_t resp_octave = -1, resp_layer = -1;
  std::vector<float>*det = nullptr, *trace = nullptr;
  std::vector<Cand>* cand = nullptr;
  int32_t ori_rank = -1;
  OrientationTrace* ori = nullptr;
  float* patch = nullptr;
};

inline unsigned blocks(size_t n) { return (unsigned)((n + DET_THREADS - 1) / DET_THREADS); }
constexpr int32_t MAX_PASS = 32768;  // images of a pass at most: a grid dimension of the ranking

struct Batch : sim3opt::BatchHandle {
  sim3opt_surf_batch_options opt;
  int32_t n_img = 0, w = 0, h = 0;
  std::vector<uint8_t> pixels;  // rows of w bytes
  // the last solve
  sim3opt_surf_batch_options run_opt;
  PassOut res;
  bool desc_in_store = false;  // the last solve was a solve_into: res.desc is empty, the store has the descriptors
  // device
  sim3opt::DevArena table_mem, pass_mem, cand_mem, chunk_mem;  // chunk_mem: a solve_into's chunks until they are joined
  struct Dev {
    Tables* tables;
    bool up;
  } dev{};

  ~Batch() { release(); }

  void release() {
    close_stream(chunk_mem, cand_mem, pass_mem, table_mem);
    dev = Dev{};
  }

  int ensure_device(const char* who) {
    if (n_img < 1) { err = std::string(who) + ": no images set"; return SIM3OPT_ERR_STATE; }
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    if (!stream) {
      release();
      if (int rc = open_stream()) return rc;
    }
    if (!dev.up) {
      wait();
      table_mem.release();
      dev = Dev{};
      std::vector<Tables> t(1);
      make_tables(t[0]);
      HIPCHK(table_mem.upload(dev.tables, t, stream, nullptr));
      HIPCHK(hipStreamSynchronize(stream));  // (t goes out of scope)
      dev.up = true;
    }
    return SIM3OPT_OK;
  }

  // Images [img0, img0 + n) through every stage; appended to `out`.  Every block of the pass is handed back.
  int run_pass(const sim3opt_surf_batch_options& o, int32_t img0, int32_t n, PassOut& out, const Debug* dbg,
               Fill* fill = nullptr) {
    const int rc = pass_body(o, img0, n, out, dbg, fill);
    wait();
    cand_mem.release(); pass_mem.release();
    return rc;
  }

  int pass_body(const sim3opt_surf_batch_options& o, int32_t img0, int32_t n, PassOut& out, const Debug* dbg, Fill* fill) {
    wait();
    cand_mem.release(); pass_mem.release();
    const size_t npix = (size_t)w * (size_t)h, nS = (size_t)(w + 1) * (size_t)(h + 1);
    uint8_t* d_img = nullptr;
    int32_t *d_S = nullptr, *tile_count = nullptr, *tile_off = nullptr, *img_total = nullptr, *cand_ptr = nullptr,
            *n_kept = nullptr, *n_drop = nullptr;
    HIPCHK(pass_mem.raw(d_img, npix * (size_t)n));
    HIPCHK(hipMemcpyAsync(d_img, pixels.data() + npix * (size_t)img0, npix * (size_t)n, hipMemcpyHostToDevice, stream));
    HIPCHK(pass_mem.raw(d_S, nS * (size_t)n));
    hipLaunchKernelGGL(k_surf_rows, dim3((unsigned)h, (unsigned)n), dim3(64), 0, stream, d_img, d_S, w, h);
    hipLaunchKernelGGL(k_surf_cols, dim3(blocks((size_t)w + 1), (unsigned)n), dim3(DET_THREADS), 0, stream, d_S, w, h);
    DetArgs A{};
    A.S = d_S; A.w = w; A.h = h; A.n_octaves = o.n_octaves; A.nl = o.n_octave_layers; A.thr = (float)o.hessian_threshold;
    int32_t tpi = 0;
    for (int oc = 0; oc < MAX_OCTAVES; ++oc) {
      A.oct_tile0[oc] = tpi;
      const int32_t rows = h >> oc, cols = w >> oc;
      A.oct_tx[oc] = oc < o.n_octaves && rows > 0 && cols > 0 ? (cols + TILE - 1) / TILE : 0;
      if (A.oct_tx[oc]) tpi += A.oct_tx[oc] * ((rows + TILE - 1) / TILE);
      else A.oct_tx[oc] = 1;  // (a divisor only: the octave owns no tile)
    }
    A.oct_tile0[MAX_OCTAVES] = tpi;  // (an octave without tiles starts at the end: the kernel's search stops before it)
    A.tiles_per_image = tpi;
    const size_t n_tiles = (size_t)tpi * (size_t)n;
    if (n_tiles > (size_t)0x7fffffff) { err = "surf_batch_solve: too many tiles in a pass; lower images_per_pass"; return SIM3OPT_ERR_ARG; }
    // the candidate offsets are int32: two strict maxima of a layer are never neighbours, so a layer of rows x cols holds
    // at most one per 2 x 2 block, and the pass at most n times the sum of that over the middle layers
    size_t most = 0;
    for (int oc = 0; oc < o.n_octaves; ++oc)
      most += (size_t)o.n_octave_layers * (size_t)(((h >> oc) + 1) / 2) * (size_t)(((w >> oc) + 1) / 2);
    if (most * (size_t)n > (size_t)0x7fffffff) {
      err = "surf_batch_solve: a pass could hold more candidates than an int32 offset counts; lower images_per_pass";
      return SIM3OPT_ERR_ARG;
    }
    HIPCHK(pass_mem.raw(tile_count, n_tiles));
    HIPCHK(pass_mem.raw(tile_off, n_tiles));
    HIPCHK(pass_mem.raw(img_total, (size_t)n));
    HIPCHK(pass_mem.raw(cand_ptr, (size_t)n + 1));
    HIPCHK(pass_mem.alloc(n_kept, (size_t)n, stream));
    HIPCHK(pass_mem.alloc(n_drop, (size_t)n, stream));
    A.tile_count = tile_count; A.tile_off = tile_off; A.cand_ptr = cand_ptr;
    A.dump_octave = A.dump_layer = -1;
    std::vector<float> h_det, h_trace;
    if (dbg && dbg->det) {
      const size_t cells = (size_t)(h >> dbg->resp_octave) * (size_t)(w >> dbg->resp_octave);
      A.dump_octave = dbg->resp_octave; A.dump_layer = dbg->resp_layer;
      HIPCHK(pass_mem.alloc(A.dump_det, cells, stream));
      HIPCHK(pass_mem.alloc(A.dump_trace, cells, stream));
      hipLaunchKernelGGL(k_surf_detect<DUMP>, dim3((unsigned)n_tiles), dim3(DET_THREADS), 0, stream, A);
      HIPCHK(sim3opt::read_back(*dbg->det, A.dump_det, cells, stream));
      HIPCHK(sim3opt::read_back(*dbg->trace, A.dump_trace, cells, stream));
    } else {
      hipLaunchKernelGGL(k_surf_detect<COUNT>, dim3((unsigned)n_tiles), dim3(DET_THREADS), 0, stream, A);
    }
    hipLaunchKernelGGL(k_surf_scan_tiles, dim3((unsigned)n), dim3(DET_THREADS), 0, stream, tile_count, tile_off, img_total, tpi);
    hipLaunchKernelGGL(k_surf_scan_images, dim3(1), dim3(DET_THREADS), 0, stream, img_total, cand_ptr, n);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> cptr;
    HIPCHK(sim3opt::read_back(cptr, cand_ptr, (size_t)n + 1, stream));
    if (dbg && dbg->S) HIPCHK(sim3opt::read_back(*dbg->S, d_S, nS, stream));
    HIPCHK(hipStreamSynchronize(stream));
    int32_t max_n = 0;
    for (int32_t i = 0; i < n; ++i) {
      if (cptr[(size_t)i + 1] < cptr[(size_t)i]) { err = "surf_batch_solve: internal error (the candidate counts)"; return SIM3OPT_ERR_HIP; }
      max_n = std::max(max_n, cptr[(size_t)i + 1] - cptr[(size_t)i]);
    }
    const size_t total = (size_t)cptr[(size_t)n];
    std::vector<float> s_kp, s_size, s_resp, s_angle, s_desc;
    std::vector<int32_t> s_oct, s_lap, s_state, h_kept, h_drop, h_cnt;
    if (total) {
      Cand* cand = nullptr;
      float *slot_kp = nullptr, *slot_size = nullptr, *slot_resp = nullptr, *slot_angle = nullptr, *slot_desc = nullptr;
      int32_t *slot_oct = nullptr, *slot_lap = nullptr, *slot_img = nullptr, *slot_state = nullptr;
      HIPCHK(cand_mem.raw(cand, total));
      HIPCHK(cand_mem.raw(slot_kp, 2 * total));
      HIPCHK(cand_mem.raw(slot_size, total));
      HIPCHK(cand_mem.raw(slot_resp, total));
      HIPCHK(cand_mem.raw(slot_angle, total));
      HIPCHK(cand_mem.raw(slot_desc, total * DESC));
      HIPCHK(cand_mem.raw(slot_oct, total));
      HIPCHK(cand_mem.raw(slot_lap, total));
      HIPCHK(cand_mem.raw(slot_img, total));
      HIPCHK(cand_mem.alloc(slot_state, total, stream));
      A.cand = cand;
      hipLaunchKernelGGL(k_surf_detect<EMIT>, dim3((unsigned)n_tiles), dim3(DET_THREADS), 0, stream, A);
      hipLaunchKernelGGL(k_surf_rank, dim3((unsigned)((max_n + RANK_TILE - 1) / RANK_TILE), (unsigned)n), dim3(RANK_TILE), 0, stream,
                         cand, cand_ptr, o.max_keypoints, slot_kp, slot_size, slot_resp, slot_oct, slot_lap, slot_img, slot_state,
                         n_kept);
      DescArgs D{};
      D.img = d_img; D.S = d_S; D.w = w; D.h = h; D.upright = o.upright; D.T = dev.tables;
      D.slot_kp = slot_kp; D.slot_size = slot_size; D.slot_img = slot_img; D.slot_state = slot_state;
      D.slot_angle = slot_angle; D.slot_desc = slot_desc; D.n_dropped = n_drop;
      hipLaunchKernelGGL(k_surf_describe<false>, dim3((unsigned)total), dim3(KP_LANES), 0, stream, D);
      HIPCHK(hipGetLastError());
      if (dbg && dbg->cand) HIPCHK(sim3opt::read_back(*dbg->cand, cand, total, stream));
      if (dbg && dbg->ori_rank >= 0) {
        if ((size_t)dbg->ori_rank >= total) { err = "surf_batch_debug: internal error (the keypoint's rank)"; return SIM3OPT_ERR_HIP; }
        D.dump_slot = dbg->ori_rank;
        HIPCHK(cand_mem.alloc(D.d_valid, (size_t)ORI_N, stream));
        HIPCHK(cand_mem.alloc(D.d_vx, (size_t)ORI_N, stream));
        HIPCHK(cand_mem.alloc(D.d_vy, (size_t)ORI_N, stream));
        HIPCHK(cand_mem.alloc(D.d_ang, (size_t)ORI_N, stream));
        HIPCHK(cand_mem.alloc(D.d_win, (size_t)ORI_WINDOWS, stream));
        HIPCHK(cand_mem.alloc(D.d_patch, (size_t)(PATCH * PATCH), stream));
        hipLaunchKernelGGL(k_surf_describe<true>, dim3(1), dim3(KP_LANES), 0, stream, D);
        HIPCHK(hipGetLastError());
        if (dbg->ori) {
          HIPCHK(hipMemcpyAsync(dbg->ori->valid, D.d_valid, sizeof(int32_t) * ORI_N, hipMemcpyDeviceToHost, stream));
          HIPCHK(hipMemcpyAsync(dbg->ori->vx, D.d_vx, sizeof(float) * ORI_N, hipMemcpyDeviceToHost, stream));
          HIPCHK(hipMemcpyAsync(dbg->ori->vy, D.d_vy, sizeof(float) * ORI_N, hipMemcpyDeviceToHost, stream));
          HIPCHK(hipMemcpyAsync(dbg->ori->angle, D.d_ang, sizeof(float) * ORI_N, hipMemcpyDeviceToHost, stream));
          HIPCHK(hipMemcpyAsync(dbg->ori->window, D.d_win, sizeof(float) * ORI_WINDOWS, hipMemcpyDeviceToHost, stream));
        }
        if (dbg->patch)
          HIPCHK(hipMemcpyAsync(dbg->patch, D.d_patch, sizeof(float) * PATCH * PATCH, hipMemcpyDeviceToHost, stream));
      }
      HIPCHK(sim3opt::read_back(s_kp, slot_kp, 2 * total, stream));
      HIPCHK(sim3opt::read_back(s_size, slot_size, total, stream));
      HIPCHK(sim3opt::read_back(s_resp, slot_resp, total, stream));
      HIPCHK(sim3opt::read_back(s_angle, slot_angle, total, stream));
      if (!fill) {
        HIPCHK(sim3opt::read_back(s_desc, slot_desc, total * DESC, stream));
      } else {
        // the chunk of the pass: room for what the ranking can keep, known from the candidate counts
        size_t bound = 0;
        for (int32_t i = 0; i < n; ++i) {
          const int32_t c = cptr[(size_t)i + 1] - cptr[(size_t)i];
          bound += (size_t)(o.max_keypoints > 0 ? std::min(c, o.max_keypoints) : c);
        }
        Fill::Chunk ch{};
        int32_t* out_ptr = nullptr;
        HIPCHK(chunk_mem.raw(ch.kp, 2 * bound));
        HIPCHK(chunk_mem.raw(ch.desc, bound * DESC));
        HIPCHK(cand_mem.raw(out_ptr, (size_t)n + 1));
        sim3opt_fstore::CompactArgs C{};
        C.n_images = n; C.tiles = (max_n + sim3opt_fstore::COMPACT_TILE - 1) / sim3opt_fstore::COMPACT_TILE;
        C.cand_ptr = cand_ptr; C.state = slot_state; C.slot_kp = slot_kp; C.slot_desc = slot_desc;
        C.base = 0; C.kp_ptr_out = out_ptr; C.out_kp = ch.kp; C.out_desc = ch.desc;
        if (int rc = sim3opt_fstore::compact_enqueue(C, cand_mem, stream, err)) return rc;
        HIPCHK(sim3opt::read_back(h_cnt, out_ptr, (size_t)n + 1, stream));
        fill->chunks.push_back(ch);
      }
      HIPCHK(sim3opt::read_back(s_oct, slot_oct, total, stream));
      HIPCHK(sim3opt::read_back(s_lap, slot_lap, total, stream));
      HIPCHK(sim3opt::read_back(s_state, slot_state, total, stream));
    } else if (dbg && dbg->cand) {
      dbg->cand->clear();
    }
    HIPCHK(sim3opt::read_back(h_kept, n_kept, (size_t)n, stream));
    HIPCHK(sim3opt::read_back(h_drop, n_drop, (size_t)n, stream));
    HIPCHK(hipStreamSynchronize(stream));
    // the results leave in order; a keypoint the orientation step dropped is passed over
    for (int32_t i = 0; i < n; ++i) {
      int32_t kept_here = 0;
      for (int32_t s = cptr[(size_t)i]; s < cptr[(size_t)i + 1]; ++s) {
        const size_t z = (size_t)s;
        if (s_state[z] == 1) { err = "surf_batch_solve: internal error (a keypoint without a descriptor)"; return SIM3OPT_ERR_HIP; }
        if (s_state[z] != 2) continue;
        out.kp.push_back(s_kp[2 * z]); out.kp.push_back(s_kp[2 * z + 1]);
        if (!fill) out.desc.insert(out.desc.end(), s_desc.begin() + (ptrdiff_t)(z * DESC), s_desc.begin() + (ptrdiff_t)((z + 1) * DESC));
        out.size.push_back(s_size[z]); out.angle.push_back(s_angle[z]); out.response.push_back(s_resp[z]);
        out.octave.push_back(s_oct[z]); out.laplacian.push_back(s_lap[z]);
        out.rank.push_back(s - cptr[(size_t)i]);
        ++kept_here;
      }
      // (solve_into: the counts the compaction emitted are kp_ptr; the small fields above follow the same predicate)
      if (fill && total && h_cnt[(size_t)i + 1] - h_cnt[(size_t)i] != kept_here) {
        err = "surf_batch_solve_into: internal error (the compaction's counts)"; return SIM3OPT_ERR_HIP;
      }
      out.kp_ptr.push_back(out.kp_ptr.back() + kept_here);
      out.status.push_back(kept_here ? SIM3OPT_SURF_OK : SIM3OPT_SURF_NO_KEYPOINTS);
      out.n_cand.push_back(cptr[(size_t)i + 1] - cptr[(size_t)i]);
      out.n_interp.push_back(h_kept[(size_t)i]);
      out.n_dropped.push_back(h_drop[(size_t)i]);
    }
    if (fill && total) {
      fill->chunks.back().rows = (size_t)h_cnt[(size_t)n];
      fill->rows += (size_t)h_cnt[(size_t)n];
    }
    return SIM3OPT_OK;
  }

  int solve() {
    err.clear();
    if (int rc = ensure_device("surf_batch_solve")) return rc;
    const sim3opt_surf_batch_options o = opt;
    PassOut out;
    const int32_t per = std::min(o.images_per_pass, MAX_PASS);
    for (int32_t i0 = 0; i0 < n_img; i0 += per)
      if (int rc = run_pass(o, i0, std::min(per, n_img - i0), out, nullptr)) return rc;
    res = std::move(out);
    run_opt = o;
    have_run = true;
    desc_in_store = false;
    int32_t ok = 0;
    for (int32_t s : res.status) ok += s == SIM3OPT_SURF_OK;
    return ok;
  }

  // solve(), with kp and desc compacted on the device into a snapshot the store adopts.  Whatever happens, the chunks
  // and an unfinished snapshot go back once the stream has run dry.
  int solve_into(sim3opt_frames* store) {
    std::shared_ptr<sim3opt_fstore::Snapshot> snap;
    const int rc = solve_into_body(store, snap);
    wait();
    chunk_mem.release();
    return rc;
  }

  int solve_into_body(sim3opt_frames* store, std::shared_ptr<sim3opt_fstore::Snapshot>& snap) {
    err.clear();
    if (!store) { err = "surf_batch_solve_into: NULL store"; return SIM3OPT_ERR_ARG; }
    if (n_img < 1) { err = "surf_batch_solve_into: no images set"; return SIM3OPT_ERR_STATE; }
    int device = -1;  // (a refusal comes before anything is put on the device)
    if (int rc = sim3opt_fstore::resolve_device(opt.device, device, err)) return rc;
    if (int rc = sim3opt_fstore::check_fill_device(store, "surf_batch_solve_into", device, err)) return rc;
    if (int rc = ensure_device("surf_batch_solve_into")) return rc;
    const sim3opt_surf_batch_options o = opt;
    PassOut out;
    Fill fill;
    const int32_t per = std::min(o.images_per_pass, MAX_PASS);
    for (int32_t i0 = 0; i0 < n_img; i0 += per) {
      if (int rc = run_pass(o, i0, std::min(per, n_img - i0), out, nullptr, &fill)) return rc;
      const std::string e = sim3opt_fstore::check_total(fill.rows, 0);
      if (!e.empty()) { err = "surf_batch_solve_into: " + e; return SIM3OPT_ERR_ARG; }
    }
    if (fill.rows != (size_t)out.kp_ptr.back()) { err = "surf_batch_solve_into: internal error (the chunks' rows)"; return SIM3OPT_ERR_HIP; }
    // the chunks joined once: the store's arrays are contiguous
    if (int rc = sim3opt_fstore::new_snapshot(out.kp_ptr, snap, err)) return rc;
    size_t at = 0;
    for (const Fill::Chunk& c : fill.chunks) {
      if (!c.rows) continue;
      HIPCHK(hipMemcpyAsync(snap->d_kp + 2 * at, c.kp, sizeof(float) * 2 * c.rows, hipMemcpyDeviceToDevice, stream));
      HIPCHK(hipMemcpyAsync(snap->d_desc + DESC * at, c.desc, sizeof(float) * DESC * c.rows, hipMemcpyDeviceToDevice, stream));
      at += c.rows;
    }
    if (int rc = sim3opt_fstore::seal_snapshot(*snap, stream, err)) return rc;
    sim3opt_fstore::adopt_snapshot(store, std::move(snap));
    res = std::move(out);
    run_opt = o;
    have_run = true;
    desc_in_store = true;
    int32_t ok = 0;
    for (int32_t s : res.status) ok += s == SIM3OPT_SURF_OK;
    return ok;
  }

  // a read-out: image `image` alone through a pass of its own (its result does not depend on its company), with the
  // options of the last solve
  int debug_pass(const char* who, int32_t image, const Debug& dbg) {
    err.clear();
    if (!have_run) { err = std::string(who) + ": no solve yet"; return SIM3OPT_ERR_STATE; }
    if (image < 0 || image >= n_img) { err = std::string(who) + ": no such image"; return SIM3OPT_ERR_ARG; }
    if (int rc = ensure_device(who)) return rc;
    PassOut scratch;
    return run_pass(run_opt, image, 1, scratch, &dbg);
  }

  // the image and the rank (before the orientation step dropped any) of keypoint k of the last solve
  int locate(const char* who, int32_t k, int32_t& image, int32_t& rank) {
    if (!have_run) { err = std::string(who) + ": no solve yet"; return SIM3OPT_ERR_STATE; }
    if (k < 0 || k >= res.kp_ptr.back()) { err = std::string(who) + ": no such keypoint"; return SIM3OPT_ERR_ARG; }
    image = (int32_t)(std::upper_bound(res.kp_ptr.begin(), res.kp_ptr.end(), k) - res.kp_ptr.begin()) - 1;
    rank = res.rank[(size_t)k];
    return SIM3OPT_OK;
  }
};

// the candidates of a read-out in scan order
inline void sort_by_scan_index(std::vector<Cand>& c) {
  std::sort(c.begin(), c.end(), [](const Cand& a, const Cand& b) { return a.key < b.key; });
}

inline void copy_candidates(const std::vector<Cand>& c, int32_t* layer, float* pos0, float* response, uint8_t* kept, float* pos1) {
  for (size_t i = 0; i < c.size(); ++i) {
    if (layer) layer[i] = c[i].octave * MAX_LAYERS + c[i].layer;
    if (pos0) { pos0[3 * i] = c[i].x0; pos0[3 * i + 1] = c[i].y0; pos0[3 * i + 2] = c[i].size0; }
    if (response) response[i] = c[i].response;
    if (kept) kept[i] = (uint8_t)c[i].kept;
    if (pos1) { pos1[3 * i] = c[i].x; pos1[3 * i + 1] = c[i].y; pos1[3 * i + 2] = c[i].size; }
  }
}

}  // namespace sim3opt_surf

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "batched SURF-64 extraction")
// ------------------------------------------------------------------------------------------
struct sim3opt_surf_batch : sim3opt_surf::Batch {};

extern "C" {

void sim3opt_surf_batch_options_default(sim3opt_surf_batch_options* o) {
  if (o) sim3opt_surf::default_options(*o);
}

sim3opt_surf_batch* sim3opt_surf_batch_create(void) {
  return sim3opt::handle_create<sim3opt_surf_batch>(sim3opt_surf_batch_options_default);
}

void sim3opt_surf_batch_destroy(sim3opt_surf_batch* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_surf_batch_last_error(const sim3opt_surf_batch* b) { return b ? b->err.c_str() : "null batch"; }

int sim3opt_surf_batch_set_options(sim3opt_surf_batch* b, const sim3opt_surf_batch_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  const std::string e = sim3opt_surf::validate_options(*o);
  if (!e.empty()) { b->err = "surf_batch_set_options: " + e; return SIM3OPT_ERR_ARG; }
  if (o->device != b->opt.device) b->release();  // the device is chosen at the next solve
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_surf_batch_set_images(sim3opt_surf_batch* b, int32_t n_images, int32_t width, int32_t height, int32_t row_stride,
                                  const uint8_t* pixels) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "surf_batch_set_images", sim3opt::NO_MEMORY, [&]() -> int {
    const std::string e = sim3opt_surf::validate_images(n_images, width, height, row_stride, pixels);
    if (!e.empty()) { b->err = "surf_batch_set_images: " + e; return SIM3OPT_ERR_ARG; }
    std::vector<uint8_t> p((size_t)n_images * (size_t)width * (size_t)height);
    for (size_t r = 0; r < (size_t)n_images * (size_t)height; ++r)
      std::memcpy(p.data() + r * (size_t)width, pixels + r * (size_t)row_stride, (size_t)width);
    b->pixels.swap(p);
    b->n_img = n_images; b->w = width; b->h = height;
    b->have_run = false;
    b->desc_in_store = false;
    b->res = sim3opt_surf::PassOut{};
    return SIM3OPT_OK;
  });
}

int sim3opt_surf_batch_dims(const sim3opt_surf_batch* b, int32_t* n_images, int32_t* width, int32_t* height,
                            int32_t* total_keypoints, int32_t tiles[3]) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (n_images) *n_images = b->n_img;
  if (width) *width = b->w;
  if (height) *height = b->h;
  if (total_keypoints) *total_keypoints = b->have_run ? b->res.kp_ptr.back() : 0;
  if (tiles) { tiles[0] = sim3opt_surf::TILE; tiles[1] = sim3opt_surf::RANK_TILE; tiles[2] = sim3opt_surf::KP_LANES; }
  return SIM3OPT_OK;
}

int sim3opt_surf_batch_solve(sim3opt_surf_batch* b) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "surf_batch_solve", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve(); });
}

int sim3opt_surf_batch_solve_into(sim3opt_surf_batch* b, sim3opt_frames* store) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "surf_batch_solve_into", sim3opt::NO_MEMORY_OR_INTERNAL, [&] { return b->solve_into(store); });
}

int sim3opt_surf_batch_get_kp_ptr(const sim3opt_surf_batch* b, int32_t* kp_ptr) {
  if (!b || !kp_ptr) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  std::memcpy(kp_ptr, b->res.kp_ptr.data(), sizeof(int32_t) * b->res.kp_ptr.size());
  return SIM3OPT_OK;
}

int sim3opt_surf_batch_get_keypoints(const sim3opt_surf_batch* b, float* kp, float* desc, float* size, float* angle,
                                     float* response, int32_t* octave, int32_t* laplacian) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  if (desc && b->desc_in_store) {  // (the handle is the caller's own: only the message changes)
    const_cast<sim3opt_surf_batch*>(b)->err =
        "surf_batch_get_keypoints: the descriptors of a solve_into are in the frame store; read them with sim3opt_frames_get";
    return SIM3OPT_ERR_STATE;
  }
  const sim3opt_surf::PassOut& r = b->res;
  const size_t n = (size_t)r.kp_ptr.back();
  if (!n) return SIM3OPT_OK;
  if (kp) std::memcpy(kp, r.kp.data(), sizeof(float) * 2 * n);
  if (desc) std::memcpy(desc, r.desc.data(), sizeof(float) * sim3opt_surf::DESC * n);
  if (size) std::memcpy(size, r.size.data(), sizeof(float) * n);
  if (angle) std::memcpy(angle, r.angle.data(), sizeof(float) * n);
  if (response) std::memcpy(response, r.response.data(), sizeof(float) * n);
  if (octave) std::memcpy(octave, r.octave.data(), sizeof(int32_t) * n);
  if (laplacian) std::memcpy(laplacian, r.laplacian.data(), sizeof(int32_t) * n);
  return SIM3OPT_OK;
}

int sim3opt_surf_batch_get_summary(const sim3opt_surf_batch* b, int32_t* status, int32_t* n_candidates, int32_t* n_interpolated,
                                   int32_t* n_dropped) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (!b->have_run) return SIM3OPT_ERR_STATE;
  const size_t n = (size_t)b->n_img;
  if (status) std::memcpy(status, b->res.status.data(), sizeof(int32_t) * n);
  if (n_candidates) std::memcpy(n_candidates, b->res.n_cand.data(), sizeof(int32_t) * n);
  if (n_interpolated) std::memcpy(n_interpolated, b->res.n_interp.data(), sizeof(int32_t) * n);
  if (n_dropped) std::memcpy(n_dropped, b->res.n_dropped.data(), sizeof(int32_t) * n);
  return SIM3OPT_OK;
}

int sim3opt_surf_batch_debug_integral(sim3opt_surf_batch* b, int32_t image, int32_t* S) {
  if (!b || !S) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "surf_batch_debug_integral", sim3opt::NO_MEMORY, [&]() -> int {
    std::vector<int32_t> v;
    sim3opt_surf::Debug d;
    d.S = &v;
    if (int rc = b->debug_pass("surf_batch_debug_integral", image, d)) return rc;
    std::memcpy(S, v.data(), sizeof(int32_t) * v.size());
    return SIM3OPT_OK;
  });
}

int sim3opt_surf_batch_debug_responses(sim3opt_surf_batch* b, int32_t image, int32_t octave, int32_t layer, int32_t* rows,
                                       int32_t* cols, float* det, float* trace) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "surf_batch_debug_responses", sim3opt::NO_MEMORY, [&]() -> int {
    b->err.clear();
    if (!b->have_run) { b->err = "surf_batch_debug_responses: no solve yet"; return SIM3OPT_ERR_STATE; }
    if (octave < 0 || octave >= b->run_opt.n_octaves || layer < 0 || layer >= b->run_opt.n_octave_layers + 2) {
      b->err = "surf_batch_debug_responses: no such layer"; return SIM3OPT_ERR_ARG;
    }
    if (rows) *rows = b->h >> octave;
    if (cols) *cols = b->w >> octave;
    if (!det && !trace) return SIM3OPT_OK;
    std::vector<float> vd, vt;
    sim3opt_surf::Debug d;
    d.resp_octave = octave; d.resp_layer = layer; d.det = &vd; d.trace = &vt;
    if (int rc = b->debug_pass("surf_batch_debug_responses", image, d)) return rc;
    if (det) std::memcpy(det, vd.data(), sizeof(float) * vd.size());
    if (trace) std::memcpy(trace, vt.data(), sizeof(float) * vt.size());
    return SIM3OPT_OK;
  });
}

int sim3opt_surf_batch_debug_candidates(sim3opt_surf_batch* b, int32_t image, int32_t* n_candidates, int32_t* layer, float* pos0,
                                        float* response, uint8_t* kept, float* pos1) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "surf_batch_debug_candidates", sim3opt::NO_MEMORY, [&]() -> int {
    b->err.clear();
    if (!b->have_run) { b->err = "surf_batch_debug_candidates: no solve yet"; return SIM3OPT_ERR_STATE; }
    if (image < 0 || image >= b->n_img) { b->err = "surf_batch_debug_candidates: no such image"; return SIM3OPT_ERR_ARG; }
    if (n_candidates) *n_candidates = b->res.n_cand[(size_t)image];
    if (!layer && !pos0 && !response && !kept && !pos1) return SIM3OPT_OK;
    std::vector<sim3opt_surf::Cand> c;
    sim3opt_surf::Debug d;
    d.cand = &c;
    if (int rc = b->debug_pass("surf_batch_debug_candidates", image, d)) return rc;
    sim3opt_surf::sort_by_scan_index(c);
    sim3opt_surf::copy_candidates(c, layer, pos0, response, kept, pos1);
    return SIM3OPT_OK;
  });
}

int sim3opt_surf_batch_debug_orientation(sim3opt_surf_batch* b, int32_t keypoint, int32_t* valid, float* vx, float* vy,
                                         float* angle, float* window) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "surf_batch_debug_orientation", sim3opt::NO_MEMORY, [&]() -> int {
    b->err.clear();
    int32_t image, rank;
    if (int rc = b->locate("surf_batch_debug_orientation", keypoint, image, rank)) return rc;
    sim3opt_surf::OrientationTrace t{};
    sim3opt_surf::Debug d;
    d.ori_rank = rank; d.ori = &t;
    if (int rc = b->debug_pass("surf_batch_debug_orientation", image, d)) return rc;
    if (valid) std::memcpy(valid, t.valid, sizeof(t.valid));
    if (vx) std::memcpy(vx, t.vx, sizeof(t.vx));
    if (vy) std::memcpy(vy, t.vy, sizeof(t.vy));
    if (angle) std::memcpy(angle, t.angle, sizeof(t.angle));
    if (window) std::memcpy(window, t.window, sizeof(t.window));
    return SIM3OPT_OK;
  });
}

int sim3opt_surf_batch_debug_patch(sim3opt_surf_batch* b, int32_t keypoint, float* patch) {
  if (!b || !patch) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "surf_batch_debug_patch", sim3opt::NO_MEMORY, [&]() -> int {
    b->err.clear();
    int32_t image, rank;
    if (int rc = b->locate("surf_batch_debug_patch", keypoint, image, rank)) return rc;
    sim3opt_surf::Debug d;
    d.ori_rank = rank; d.patch = patch;
    return b->debug_pass("surf_batch_debug_patch", image, d);
  });
}

int sim3opt_surf_reference_image(const sim3opt_surf_batch_options* o, int32_t width, int32_t height, int32_t row_stride,
                                 const uint8_t* pixels, int32_t capacity, float* kp, float* desc, float* size, float* angle,
                                 float* response, int32_t* octave, int32_t* laplacian, int32_t counts[3], int32_t* S,
                                 int32_t resp_octave, int32_t resp_layer, float* det, float* trace, int32_t cand_capacity,
                                 int32_t* cand_layer, float* cand_pos0, float* cand_response, uint8_t* cand_kept, float* cand_pos1) {
  if (!o) return SIM3OPT_ERR_ARG;
  try {
    if (!sim3opt_surf::validate_options(*o).empty() || !sim3opt_surf::validate_images(1, width, height, row_stride, pixels).empty())
      return SIM3OPT_ERR_ARG;
    sim3opt_surf::Tables T;
    sim3opt_surf::make_tables(T);
    sim3opt_surf::ImageResult R;
    sim3opt_surf::reference_image(pixels, width, height, row_stride, *o, T, R);
    const size_t n = std::min(R.kp.size(), (size_t)std::max(capacity, 0));
    for (size_t i = 0; i < n; ++i) {
      const sim3opt_surf::Keypoint& k = R.kp[i];
      if (kp) { kp[2 * i] = k.x; kp[2 * i + 1] = k.y; }
      if (desc) std::memcpy(desc + i * sim3opt_surf::DESC, k.desc, sizeof(k.desc));
      if (size) size[i] = k.size;
      if (angle) angle[i] = k.angle;
      if (response) response[i] = k.response;
      if (octave) octave[i] = k.octave;
      if (laplacian) laplacian[i] = k.laplacian;
    }
    if (counts) { counts[0] = R.n_candidates; counts[1] = R.n_interpolated; counts[2] = R.n_dropped; }
    if (S) std::memcpy(S, R.S.data(), sizeof(int32_t) * R.S.size());
    if (det || trace) {
      if (resp_octave < 0 || resp_octave >= o->n_octaves || resp_layer < 0 || resp_layer >= o->n_octave_layers + 2) return SIM3OPT_ERR_ARG;
      std::vector<float> vd, vt;
      sim3opt_surf::response_plane(R.S.data(), width, height, resp_octave, resp_layer, vd, vt);
      if (det && !vd.empty()) std::memcpy(det, vd.data(), sizeof(float) * vd.size());
      if (trace && !vt.empty()) std::memcpy(trace, vt.data(), sizeof(float) * vt.size());
    }
    if (cand_capacity > 0) {
      std::vector<sim3opt_surf::Cand> c(R.cand.begin(), R.cand.begin() + (ptrdiff_t)std::min(R.cand.size(), (size_t)cand_capacity));
      sim3opt_surf::copy_candidates(c, cand_layer, cand_pos0, cand_response, cand_kept, cand_pos1);
    }
    return (int)R.kp.size();
  } catch (...) {
    return SIM3OPT_ERR_ARG;
  }
}

}  // extern "C"
