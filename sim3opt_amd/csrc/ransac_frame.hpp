// ransac_frame.hpp -- what the batched RANSAC stages (pnp_batch.hip, essential_batch.hip) are apart from their minimal
// solver: the consensus step on the device and the handle on the host.  DESIGN.md, "The RANSAC consensus frame".
//
// Device.  Workgroup = problem, WG threads.  A stage makes its hypotheses in chunks and leaves their models (DOUBLES
// doubles each) with a validity flag in LDS; score_chunk gives every valid one of a chunk to one wavefront, lanes
// over the points, and every wavefront keeps the best it has scored; best_of_waves picks among the wavefronts.  The
// order -- larger inlier count, then smaller cost, then smaller hypothesis index -- is stated in these two functions
// and nowhere else; it makes a problem's result independent of which wavefront scored what and of the batch.
// A stage supplies a scoring policy S:
//   S::DOUBLES, S::Prepared, prepare(model, Prepared&)     a model and what its scoring needs of it
//   inlier(prepared, Pts, i, e2)                           whether point i counts, and its squared error
// and, for the debug scoring kernel k_ransac_score<S>:
//   S::Args (with ptr and H), S{A}, S::CHUNK, S::LDS_POINTS, S::POINT_DOUBLES, S::Lds,
//   S::global(A, p0) and S::stage(global, n, lds)          the problem's points, where they lie and staged
// Host.  RansacBatch<T, Derived> is the handle: the problems, the last solve's results, the eight device blocks, and
// set_problems / solve / the read-outs.  T names the widths, the kernel, the prefix of the messages; Derived adds
// args() and what only its stage has.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "handle_device.hpp"

namespace sim3opt_ransac {

constexpr int WG = 256;  // threads of a workgroup (four wavefronts)
constexpr int NWAVE = WG / 64;

template <int DOUBLES>
struct Best {  // of the hypotheses a wavefront has scored: the same in all its lanes
  int count = -1, h = -1;
  double cost = 0.0;
  double model[DOUBLES] = {};
};

// One wavefront scores one model: lane l takes the points l, l + 64, ... in ascending order, then a butterfly; every
// lane ends with the same count and the same bits of cost.
template <class S, class Pts>
__device__ __forceinline__ void score_model(const S& score, const Pts& P, int n, const double* model, int& count,
                                            double& cost) {
  const int lane = threadIdx.x & 63;
  typename S::Prepared prep;
  score.prepare(model, prep);
  int c = 0;
  double s = 0.0;
  for (int i = lane; i < n; i += 64) {
    double e2;
    if (score.inlier(prep, P, i, e2)) { ++c; s += e2; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { c += __shfl_xor(c, off); s += __shfl_xor(s, off); }
  count = c;
  cost = s;
}

// The models s_model[stride k], k < m, of a chunk (s_valid[k] says which count): wavefront w scores k = w, w + 4, ...,
// writes count and cost of hypothesis `first + k` and updates its best (larger count, then smaller cost; it goes
// through its hypotheses in ascending order, so of equals the smallest index stays).
template <class S, class Pts>
__device__ __forceinline__ void score_chunk(const S& score, const Pts& P, int n, const double* s_model, int stride,
                                            const int* s_valid, int m, int first, int32_t* count_out,
                                            int count_stride, double* cost_out, Best<S::DOUBLES>& best) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < m; k += NWAVE) {
    int c = 0;
    double s = 0.0;
    if (s_valid[k] != 0) {
      score_model(score, P, n, s_model + stride * k, c, s);
      if (c > best.count || (c == best.count && s < best.cost)) {
        best.count = c; best.cost = s; best.h = first + k;
#pragma unroll
        for (int i = 0; i < S::DOUBLES; ++i) best.model[i] = s_model[stride * k + i];
      }
    }
    if (lane == 0) {
      count_out[(size_t)(first + k) * count_stride] = c;
      cost_out[first + k] = s;
    }
  }
}

// The best of the four wavefronts (count, then cost, then index) through s_best (NWAVE x (3 + DOUBLES) doubles of
// LDS): its inlier count, its index (-1: no wavefront scored a valid hypothesis, and nothing else is meaningful), its
// cost and its model, in every thread.
template <int DOUBLES>
__device__ __forceinline__ void best_of_waves(const Best<DOUBLES>& best, double* s_best, int& n_hyp, int& best_h,
                                              double& cost_hyp, double model[DOUBLES]) {
  constexpr int SLOT = 3 + DOUBLES;
  if ((threadIdx.x & 63) == 0) {
    double* b = s_best + SLOT * (threadIdx.x >> 6);
    b[0] = (double)best.count; b[1] = best.cost; b[2] = (double)best.h;
#pragma unroll
    for (int i = 0; i < DOUBLES; ++i) b[3 + i] = best.model[i];
  }
  __syncthreads();
  int bw = 0;
  for (int w = 1; w < NWAVE; ++w) {
    const double* a = s_best + SLOT * w;
    const double* b = s_best + SLOT * bw;
    if (a[2] < 0.0) continue;
    if (b[2] < 0.0 || a[0] > b[0] || (a[0] == b[0] && (a[1] < b[1] || (a[1] == b[1] && a[2] < b[2])))) bw = w;
  }
  const double* b = s_best + SLOT * bw;
  n_hyp = (int)b[0]; cost_hyp = b[1]; best_h = (int)b[2];
#pragma unroll
  for (int i = 0; i < DOUBLES; ++i) model[i] = b[3 + i];
}

// the exits without a result: no point of the problem is an inlier
__device__ __forceinline__ void clear_mask(uint8_t* mask, int64_t p0, int n) {
  for (int i = threadIdx.x; i < n; i += WG) mask[p0 + i] = 0;
}

// sim3opt_*_batch_debug_score: A.H supplied models per problem through score_chunk
template <class S>
__global__ __launch_bounds__(WG) void k_ransac_score(typename S::Args A, const double* models, int32_t* count,
                                                     double* cost) {
  __shared__ double s_pts[S::POINT_DOUBLES * S::LDS_POINTS];
  __shared__ double s_model[S::DOUBLES * S::CHUNK];
  __shared__ int s_valid[S::CHUNK];
  const int tid = threadIdx.x, prob = blockIdx.x;
  const int64_t p0 = A.ptr[prob];
  const int n = (int)(A.ptr[prob + 1] - p0);
  const auto G = S::global(A, p0);
  const bool staged = n <= S::LDS_POINTS;
  if (staged) S::stage(G, n, s_pts);
  const S score{A};
  Best<S::DOUBLES> best;
  for (int first = 0; first < A.H; first += S::CHUNK) {
    if (tid < S::CHUNK && first + tid < A.H) {
#pragma unroll
      for (int i = 0; i < S::DOUBLES; ++i)
        s_model[S::DOUBLES * tid + i] = models[((size_t)prob * A.H + first + tid) * S::DOUBLES + i];
      s_valid[tid] = 1;
    }
    __syncthreads();
    const int m = min(S::CHUNK, A.H - first);
    int32_t* const co = count + (size_t)prob * A.H;
    double* const cs = cost + (size_t)prob * A.H;
    if (staged) score_chunk(score, typename S::Lds{s_pts}, n, s_model, S::DOUBLES, s_valid, m, first, co, 1, cs, best);
    else score_chunk(score, G, n, s_model, S::DOUBLES, s_valid, m, first, co, 1, cs, best);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// host side.  T: Options, Args, Score; IN0 / IN1 (columns of the two input arrays), SAMPLE, MODEL, HYP_INTS
// (= SAMPLE + 3: the sample, solutions, valid, inlier count), OUT_DOUBLES (the pose first), OUT_INTS (the status
// first); KERNEL; PREFIX and IN0_NAME for the messages; n_inliers(o) of a problem's OUT_INTS.
// ------------------------------------------------------------------------------------------
template <class T, class Derived>
struct RansacBatch : sim3opt::BatchHandle {
  typename T::Options opt;
  // the problems, as set
  std::vector<int32_t> ptr;
  std::vector<double> in0, in1;
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
    double *in, *hyp_model, *hyp_cost, *out_d;
    int32_t *hyp_int, *out_i;
    uint8_t* mask;
    int64_t cap_n, cap_total, cap_H;  // what the blocks were sized for
    bool uploaded;
  } dev{};

  ~RansacBatch() { release(); }
  int32_t n() const { return ptr.empty() ? 0 : (int32_t)ptr.size() - 1; }
  int64_t total() const { return ptr.empty() ? 0 : ptr.back(); }
  static std::string who(const char* entry) { return std::string(T::PREFIX) + entry; }

  void release() {
    close_stream(mem);
    dev = Dev{};
  }

  // the device, the handle's blocks (sized by the problems and options.iterations) and the problems on the device
  int ensure_device(const std::string& who) {
    if (n() < 1) { err = who + ": no problems set"; return SIM3OPT_ERR_STATE; }
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    const size_t N = (size_t)n(), P = (size_t)total(), H = (size_t)opt.iterations;
    if ((int64_t)N != dev.cap_n || (int64_t)P != dev.cap_total || (int64_t)H != dev.cap_H) {
      release();
      if (int rc = open_stream()) return rc;
      HIPCHK(mem.raw(dev.ptr, N + 1));
      HIPCHK(mem.raw(dev.in, (T::IN0 + T::IN1) * P));
      HIPCHK(mem.raw(dev.hyp_model, T::MODEL * N * H));
      HIPCHK(mem.raw(dev.hyp_cost, N * H));
      HIPCHK(mem.raw(dev.hyp_int, T::HYP_INTS * N * H));
      HIPCHK(mem.raw(dev.out_d, T::OUT_DOUBLES * N));
      HIPCHK(mem.raw(dev.out_i, T::OUT_INTS * N));
      HIPCHK(mem.raw(dev.mask, P));
      dev.cap_n = (int64_t)N; dev.cap_total = (int64_t)P; dev.cap_H = (int64_t)H;
    }
    if (!dev.uploaded) {
      HIPCHK(hipMemcpyAsync(dev.ptr, ptr.data(), sizeof(int32_t) * (N + 1), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(dev.in, in0.data(), sizeof(double) * T::IN0 * P, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(dev.in + T::IN0 * P, in1.data(), sizeof(double) * T::IN1 * P, hipMemcpyHostToDevice,
                            stream));
      dev.uploaded = true;
    }
    return SIM3OPT_OK;
  }

  typename T::Args args() const { return static_cast<const Derived*>(this)->args(); }

  int set_problems(int32_t n_problems, const int32_t* point_ptr, const double* a0, const double* a1, double focal,
                   double pcx, double pcy) {
    // (the message of an exception is "<prefix>_set_problems: out of host memory"; nothing allocates outside the guard)
    return sim3opt::guarded(this, T::PREFIX, "_set_problems: out of host memory", [&]() -> int {
      const std::string w = who("_set_problems");
      if (n_problems < 1 || !point_ptr || !a0 || !a1 || !(focal > 0) || !std::isfinite(focal) ||
          !std::isfinite(pcx) || !std::isfinite(pcy)) {
        err = w + ": bad argument";
        return SIM3OPT_ERR_ARG;
      }
      const std::string e = sim3opt::check_point_ptr(n_problems, point_ptr);
      if (!e.empty()) { err = w + ": " + e; return SIM3OPT_ERR_ARG; }
      const size_t P = (size_t)point_ptr[n_problems];
      if (!sim3opt::all_finite(a0, T::IN0 * P)) { err = w + ": non-finite " + T::IN0_NAME; return SIM3OPT_ERR_ARG; }
      if (!sim3opt::all_finite(a1, T::IN1 * P)) { err = w + ": non-finite observation"; return SIM3OPT_ERR_ARG; }
      std::vector<int32_t> p(point_ptr, point_ptr + n_problems + 1);
      std::vector<double> v0(a0, a0 + T::IN0 * P), v1(a1, a1 + T::IN1 * P);
      // nothing failed: the handle changes now
      ptr.swap(p); in0.swap(v0); in1.swap(v1);
      f = focal; cx = pcx; cy = pcy;
      out_d.clear(); out_i.clear(); mask.clear();
      have_run = false;
      dev.uploaded = false;
      return SIM3OPT_OK;
    });
  }

  int dims(int32_t* n_problems, int32_t* total_points) const {
    if (n_problems) *n_problems = n();
    if (total_points) *total_points = (int32_t)total();
    return SIM3OPT_OK;
  }

  int solve() {
    err.clear();
    const int rc = ensure_device(who("_solve"));
    if (rc != SIM3OPT_OK) return rc;
    const size_t N = (size_t)n(), P = (size_t)total(), H = (size_t)opt.iterations;
    // hypotheses of a problem that runs none (status 1) read as zeros
    HIPCHK(hipMemsetAsync(dev.hyp_model, 0, sizeof(double) * T::MODEL * N * H, stream));
    HIPCHK(hipMemsetAsync(dev.hyp_cost, 0, sizeof(double) * N * H, stream));
    HIPCHK(hipMemsetAsync(dev.hyp_int, 0, sizeof(int32_t) * T::HYP_INTS * N * H, stream));
    hipLaunchKernelGGL(T::KERNEL, dim3((unsigned)N), dim3(WG), 0, stream, args());  // the one launch of the batch
    HIPCHK(hipGetLastError());
    std::vector<double> od;
    std::vector<int32_t> oi;
    std::vector<uint8_t> m;
    HIPCHK(sim3opt::read_back(od, dev.out_d, T::OUT_DOUBLES * N, stream));
    HIPCHK(sim3opt::read_back(oi, dev.out_i, T::OUT_INTS * N, stream));
    HIPCHK(sim3opt::read_back(m, dev.mask, P, stream));
    HIPCHK(hipStreamSynchronize(stream));
    out_d.swap(od); out_i.swap(oi); mask.swap(m);
    solved_H = opt.iterations;
    have_run = true;
    int ok = 0;
    for (size_t k = 0; k < N; ++k) ok += out_i[T::OUT_INTS * k] == 0;
    return ok;
  }

  int get_poses(double* poses) const {
    if (!poses) return SIM3OPT_ERR_ARG;
    if (!have_run) return SIM3OPT_ERR_STATE;
    for (int32_t k = 0; k < n(); ++k)
      std::memcpy(poses + 7 * (size_t)k, out_d.data() + (size_t)T::OUT_DOUBLES * k, sizeof(double) * 7);
    return SIM3OPT_OK;
  }

  int get_inliers(uint8_t* m, int32_t* n_inliers) const {
    if (!m && !n_inliers) return SIM3OPT_ERR_ARG;
    if (!have_run) return SIM3OPT_ERR_STATE;
    if (m && !mask.empty()) std::memcpy(m, mask.data(), mask.size());
    if (n_inliers)
      for (int32_t k = 0; k < n(); ++k) n_inliers[k] = T::n_inliers(out_i.data() + (size_t)T::OUT_INTS * k);
    return SIM3OPT_OK;
  }

  int debug_hypotheses(int32_t problem, int32_t* sample, int32_t* n_solutions, int32_t* valid, double* model,
                       int32_t* count, double* cost) {
    err.clear();
    const std::string w = who("_debug_hypotheses");
    if (!have_run) { err = w + ": no solve yet"; return SIM3OPT_ERR_STATE; }
    if (problem < 0 || problem >= n()) { err = w + ": no such problem"; return SIM3OPT_ERR_ARG; }
    if (solved_H != opt.iterations || dev.cap_H != solved_H) {
      err = w + ": options.iterations changed since the solve";
      return SIM3OPT_ERR_STATE;
    }
    const size_t H = (size_t)solved_H;
    std::vector<int32_t> hi;
    std::vector<double> hm, hc;
    HIPCHK(sim3opt::read_back(hi, dev.hyp_int + T::HYP_INTS * H * problem, T::HYP_INTS * H, stream));
    HIPCHK(sim3opt::read_back(hm, dev.hyp_model + T::MODEL * H * problem, T::MODEL * H, stream));
    HIPCHK(sim3opt::read_back(hc, dev.hyp_cost + H * problem, H, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (size_t h = 0; h < H; ++h) {
      if (sample)
        for (int k = 0; k < T::SAMPLE; ++k) sample[T::SAMPLE * h + k] = hi[T::HYP_INTS * h + k];
      if (n_solutions) n_solutions[h] = hi[T::HYP_INTS * h + T::SAMPLE];
      if (valid) valid[h] = hi[T::HYP_INTS * h + T::SAMPLE + 1];
      if (count) count[h] = hi[T::HYP_INTS * h + T::SAMPLE + 2];
    }
    if (model) std::memcpy(model, hm.data(), sizeof(double) * hm.size());
    if (cost) std::memcpy(cost, hc.data(), sizeof(double) * H);
    return SIM3OPT_OK;
  }

  int debug_score(int32_t P, const double* models, int32_t* count, double* cost) {
    err.clear();
    const int rc = ensure_device(who("_debug_score"));
    if (rc != SIM3OPT_OK) return rc;
    const size_t N = (size_t)n(), M = N * (size_t)P;
    sim3opt::DevBuf<double> dm, dc;
    sim3opt::DevBuf<int32_t> dn;
    HIPCHK(dm.alloc(T::MODEL * M));
    HIPCHK(dc.alloc(M));
    HIPCHK(dn.alloc(M));
    HIPCHK(hipMemcpyAsync(dm.get(), models, sizeof(double) * T::MODEL * M, hipMemcpyHostToDevice, stream));
    typename T::Args A = args();
    A.H = P;
    hipLaunchKernelGGL(k_ransac_score<typename T::Score>, dim3((unsigned)N), dim3(WG), 0, stream, A, dm.get(),
                       dn.get(), dc.get());
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
};

}  // namespace sim3opt_ransac
