// ba.hip -- the reference's `ba_demo` (bal_example.cpp:44-243) on the GPU: Levenberg-Marquardt bundle
// adjustment of SE(3) cameras and 3-D points over pinhole observations with a Huber kernel.
//
// What it replaces (all third-party g2o code; restated in oracle/ba_oracle.py, [upstream-recall]):
//   g2o::VertexSE3Expmap (T_w2c, update T <- exp([omega, upsilon]) T)       bal_example.cpp:112-118, :160-175
//   g2o::VertexSBAPointXYZ, setMarginalized(true)                            :120-130
//   g2o::EdgeProjectXYZ2UV + CameraParameters(f, pp, 0), information I/s^2    :90-97, :134-158
//   g2o::RobustKernelHuber(2.5)                                              :149-153
//   BlockSolver_6_3 (Schur complement on the points) + LinearSolverEigen     :76-88
//   OptimizationAlgorithmLevenberg, optimize(maxIterations)                  :86-88, :207
//
// Device pipeline of one LM iteration (all FP64, fixed summation orders, no atomics):
//   k_ba_obs      thread / observation: e = uv - K (R p + t), analytic Jacobians, Huber weight;
//                 stores A = sqrt(w) J_cam (2x6), B = sqrt(w) J_point (2x3), es = sqrt(w) e
//   k_ba_points   thread / point: H_pp = lambda I + sum B^T B over its observations (list order),
//                 b_p = -sum B^T es, H_pp^-1
//   k_ba_obs2     thread / observation: Z = (A^T B) H_pp^-1 (6x3)
//   k_ba_reduced  wavefront / block (i,j) of the reduced camera system: S_ij = [i=j](lambda I + sum
//                 A^T A) - sum over the listed observation pairs Z_o1 (A^T B)_o2^T (lane = pair, fixed-order
//                 butterfly sum); the diagonal block's wavefront also forms g_i = b_c,i - sum Z_o b_p(o)
//   k_ldl*        the reduced camera system S dx_c = g solved exactly: the level-scheduled block
//                 Cholesky of direct.hpp, run by a BlockLdl (direct_factor.hpp; written for the 7x7 blocks
//                 of the Sim(3) graphs; the 6x6 camera blocks are stored padded to 7x7 with a unit diagonal
//                 entry, which leaves the factorisation of the 6x6 part untouched)
//   k_ba_pcg      fallback when a factorisation would be too large: block-Jacobi PCG in ONE workgroup
//   k_ba_backsub  thread / point: dx_p = H_pp^-1 b_p - sum Z_o^T dx_c(cam(o))
//   k_ba_update   exp-map update of the cameras, additive update of the points (backup kept)
//   k_ba_chi2     thread / observation: robustified chi2, fixed-order block sums
// Covariances of the refined map (sim3opt_ba_covariances): the same linearisation and reduced system, a second BlockLdl
// with the selected inversion, and the kernels of ba_cov_kernels.hpp on top of S^-1 (host side: ba_cov_host.hpp).
// The host runs g2o's lambda policy on three scalars per trial: engine.hip's LmDamping (lm_damping.hpp).
// The camera / point arithmetic is ba_math.hpp's, shared with the batched two-view kernel (ba_batch.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstddef>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "ba_cov_host.hpp"
#include "ba_math.hpp"
#include "handle_device.hpp"
#include "direct_factor.hpp"
#include "lm_damping.hpp"

namespace sim3opt_bundle {

constexpr int WG = 256;

struct Cam {  // T_w2c: unit quaternion (x y z w) and translation; 8th double pads to 64 bytes
  double q[4], t[3], pad;
};
constexpr bool dev_block_is_floating(const Cam*) { return true; }  // doubles only (csrc/devmem.hpp's test mode)

struct Scal {
  double chi2, scale, maxdiag;
  int32_t pcg_iters, fail;  // fail: PCG breakdown or a non-positive pivot of the factorisation
  double pcg_rel;
};

using sim3opt::ldl_sum_over_c;
using sim3opt::LmDamping;

struct ObsArgs {
  int32_t n_obs;
  const int32_t* oc;
  const int32_t* op;
  const double* uv;
  const Cam* cams;
  const double* pts;
  double f, cx, cy, omega, huber;
};

// residual of one observation: e = uv - K (R p + t); X = camera-frame point
__device__ __forceinline__ void ba_residual(const ObsArgs& A, int o, double R[9], double X[3], double e[2]) {
  const Cam c = A.cams[A.oc[o]];
  const double* p = A.pts + (size_t)3 * A.op[o];
  ba_project_residual(c.q, c.t, p, A.uv[2 * (size_t)o], A.uv[2 * (size_t)o + 1], A.f, A.cx, A.cy, R, X, e);
}

// per observation: 20 doubles [A (2x6 row-major), B (2x3 row-major), es (2)], all scaled by sqrt(w Omega)
__global__ __launch_bounds__(WG) void k_ba_obs(ObsArgs A, double* __restrict__ lin) {
  const int o = blockIdx.x * WG + threadIdx.x;
  if (o >= A.n_obs) return;
  double R[9], X[3], e[2];
  ba_residual(A, o, R, X, e);
  double rho, w;
  ba_huber(A.omega * (e[0] * e[0] + e[1] * e[1]), A.huber, rho, w);
  const double sw = sqrt(w * A.omega);
  double Jc[12], Jp[6];
  ba_jacobians(R, X, A.f, Jc, Jp);
  double* d = lin + (size_t)20 * o;
#pragma unroll
  for (int i = 0; i < 12; ++i) d[i] = sw * Jc[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) d[12 + i] = sw * Jp[i];
  d[18] = sw * e[0];
  d[19] = sw * e[1];
}

// per point: Hinv (9, symmetric), bp (3), undamped max diagonal
__global__ __launch_bounds__(WG) void k_ba_points(int np, const int32_t* __restrict__ pptr,
                                                  const int32_t* __restrict__ pobs,
                                                  const double* __restrict__ lin, double lambda,
                                                  double* __restrict__ Hinv, double* __restrict__ bp,
                                                  double* __restrict__ pdmax) {
  const int p = blockIdx.x * WG + threadIdx.x;
  if (p >= np) return;
  double H[6] = {0, 0, 0, 0, 0, 0};  // xx xy xz yy yz zz
  double b[3] = {0, 0, 0};
  for (int k = pptr[p]; k < pptr[p + 1]; ++k) {
    const double* d = lin + (size_t)20 * pobs[k];
    const double* B = d + 12;
    H[0] += B[0] * B[0] + B[3] * B[3];
    H[1] += B[0] * B[1] + B[3] * B[4];
    H[2] += B[0] * B[2] + B[3] * B[5];
    H[3] += B[1] * B[1] + B[4] * B[4];
    H[4] += B[1] * B[2] + B[4] * B[5];
    H[5] += B[2] * B[2] + B[5] * B[5];
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] -= B[c] * d[18] + B[3 + c] * d[19];
  }
  pdmax[p] = fmax(H[0], fmax(H[3], H[5]));
  const double a = H[0] + lambda, bb = H[1], c = H[2], dd = H[3] + lambda, ee = H[4], ff = H[5] + lambda;
  ba_sym3_inverse(a, bb, c, dd, ee, ff, Hinv + (size_t)9 * p);
  bp[3 * (size_t)p] = b[0]; bp[3 * (size_t)p + 1] = b[1]; bp[3 * (size_t)p + 2] = b[2];
}

// per observation: Z = (A^T B) Hinv_p, 6x3 row-major
__global__ __launch_bounds__(WG) void k_ba_obs2(int n_obs, const int32_t* __restrict__ op,
                                                const double* __restrict__ lin,
                                                const double* __restrict__ Hinv, double* __restrict__ Z) {
  const int o = blockIdx.x * WG + threadIdx.x;
  if (o >= n_obs) return;
  const double* d = lin + (size_t)20 * o;
  const double* Hi = Hinv + (size_t)9 * op[o];
  double* z = Z + (size_t)18 * o;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double y0 = d[r] * d[12] + d[6 + r] * d[15];
    const double y1 = d[r] * d[13] + d[6 + r] * d[16];
    const double y2 = d[r] * d[14] + d[6 + r] * d[17];
#pragma unroll
    for (int c = 0; c < 3; ++c) z[3 * r + c] = y0 * Hi[c] + y1 * Hi[3 + c] + y2 * Hi[6 + c];
  }
}

// reduced camera system: one wavefront per block k = (row i, column j), stored as a 7x7 column-major
// block (entry (r, c) at r + 7c) whose 6x6 part is S_ij and whose 7th row / column is that of the
// identity; camera vectors are 7 per camera with a zero pad.  The lanes share out the block's list of
// observation pairs (lane = pair, 64 at a time, every load independent), each keeping a private 6x6
// sum; a butterfly over the wavefront adds them in a fixed order.  The diagonal block's list holds
// every observation of the camera as (o, o): H_cc, b_c and g are formed in the same pass.
__global__ __launch_bounds__(WG) void k_ba_reduced(int nblk, const int32_t* __restrict__ brow,
                                                   const int32_t* __restrict__ bcol,
                                                   const int32_t* __restrict__ sptr,
                                                   const int32_t* __restrict__ sa,
                                                   const int32_t* __restrict__ sb,
                                                   const int32_t* __restrict__ op,
                                                   const double* __restrict__ lin,
                                                   const double* __restrict__ Z,
                                                   const double* __restrict__ bp,
                                                   const uint8_t* __restrict__ fixed, double lambda,
                                                   double* __restrict__ S, double* __restrict__ g,
                                                   double* __restrict__ bc, double* __restrict__ cdmax) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= nblk) return;
  const int i = brow[k], j = bcol[k];
  const int l49 = lane < 49 ? lane : lane - 49;
  const int r = l49 % 7, c = l49 / 7;
  const bool pad = r == 6 || c == 6;
  const bool dg = i == j;
  if (fixed[i] | fixed[j]) {  // setFixed(true): the camera leaves the system (identity row, zero rhs)
    if (lane < 49) S[(size_t)49 * k + lane] = (dg && r == c) ? 1.0 : 0.0;
    if (dg && lane < 7) {
      g[7 * (size_t)i + lane] = 0.0;
      bc[7 * (size_t)i + lane] = 0.0;
      cdmax[7 * (size_t)i + lane] = 0.0;
    }
    return;
  }
  double acc[36], hd[6], bcv[6], gbv[6];
#pragma unroll
  for (int q = 0; q < 36; ++q) acc[q] = 0.0;
#pragma unroll
  for (int q = 0; q < 6; ++q) hd[q] = bcv[q] = gbv[q] = 0.0;
  for (int e = sptr[k] + lane; e < sptr[k + 1]; e += 64) {
    const int o1 = sa[e], o2 = sb[e];
    const double* z = Z + (size_t)18 * o1;
    const double* d = lin + (size_t)20 * o2;
    double zz[18], dd[20];
#pragma unroll
    for (int q = 0; q < 18; ++q) zz[q] = z[q];
#pragma unroll
    for (int q = 0; q < 20; ++q) dd[q] = d[q];
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) {  // Y_o2 row cc = (A^T B) row cc
      const double y0 = dd[cc] * dd[12] + dd[6 + cc] * dd[15];
      const double y1 = dd[cc] * dd[13] + dd[6 + cc] * dd[16];
      const double y2 = dd[cc] * dd[14] + dd[6 + cc] * dd[17];
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) acc[6 * rr + cc] -= zz[3 * rr] * y0 + zz[3 * rr + 1] * y1 + zz[3 * rr + 2] * y2;
    }
    if (dg && o1 == o2) {
      const double* b3 = bp + (size_t)3 * op[o1];
      const double b0 = b3[0], b1 = b3[1], b2 = b3[2];
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) {
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) acc[6 * rr + cc] += dd[rr] * dd[cc] + dd[6 + rr] * dd[6 + cc];
        hd[rr] += dd[rr] * dd[rr] + dd[6 + rr] * dd[6 + rr];
        bcv[rr] -= dd[rr] * dd[18] + dd[6 + rr] * dd[19];
        gbv[rr] -= zz[3 * rr] * b0 + zz[3 * rr + 1] * b1 + zz[3 * rr + 2] * b2;
      }
    }
  }
  // butterfly sums (every lane ends with the total), then lane = entry picks its value
  double mine = 0.0, vh = 0.0, vb = 0.0, vg = 0.0;
  const int idx = pad ? 0 : 6 * r + c;
#pragma unroll
  for (int q = 0; q < 36; ++q) {
    double v = acc[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    mine = idx == q ? v : mine;
  }
  if (dg) {
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      double h = hd[q], b = bcv[q], gg = gbv[q];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        h += __shfl_xor(h, off);
        b += __shfl_xor(b, off);
        gg += __shfl_xor(gg, off);
      }
      if (lane == q) { vh = h; vb = b; vg = gg; }
    }
    if (lane < 7) {
      // undamped diagonal for lambda_0 (computeLambdaInit looks at every vertex's Hessian diagonal)
      cdmax[7 * (size_t)i + lane] = lane < 6 ? vh : 0.0;
      bc[7 * (size_t)i + lane] = lane < 6 ? vb : 0.0;
      g[7 * (size_t)i + lane] = lane < 6 ? vb + vg : 0.0;
    }
    if (r == c) mine += lambda;
  }
  if (lane < 49) S[(size_t)49 * k + lane] = pad ? ((dg && r == c) ? 1.0 : 0.0) : mine;
}

// Fallback: block-Jacobi PCG on S x = g inside ONE workgroup (rows = cameras, padded 7x7 blocks,
// block-CSR with the diagonal block first in every row).  Wavefront per block row in the SpMV, thread
// per unknown in the vector steps; dot products through LDS in a fixed order.
__global__ __launch_bounds__(1024) void k_ba_pcg(int nc, const int32_t* __restrict__ rptr,
                                                 const int32_t* __restrict__ cidx,
                                                 const double* __restrict__ S,
                                                 const double* __restrict__ g, double* __restrict__ x,
                                                 double* __restrict__ rv, double* __restrict__ zv,
                                                 double* __restrict__ pv, double* __restrict__ qv,
                                                 double* __restrict__ Dinv, int max_iter, double tol2,
                                                 Scal* sc) {
  __shared__ double red[1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int n = 7 * nc;
  auto dot = [&](const double* a, const double* b) {
    double s = 0.0;
    for (int i = tid; i < n; i += blockDim.x) s += a[i] * b[i];
    red[tid] = s;
    __syncthreads();
    for (int off = blockDim.x >> 1; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    const double v = red[0];
    __syncthreads();
    return v;
  };
  // D^-1: thread per camera, Gauss-Jordan on the diagonal block (stored row-major here)
  bool spd = true;
  for (int i = tid; i < nc; i += blockDim.x) {
    double a[7][7];
    const double* blk = S + (size_t)49 * rptr[i];
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
      for (int c = 0; c < 7; ++c) a[r][c] = blk[r + 7 * c];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      if (!(a[k][k] > 0.0)) spd = false;
      const double d = 1.0 / a[k][k];
#pragma unroll
      for (int jj = 0; jj < 7; ++jj)
        if (jj != k) a[k][jj] *= d;
#pragma unroll
      for (int ii = 0; ii < 7; ++ii)
        if (ii != k) {
          const double f = a[ii][k];
#pragma unroll
          for (int jj = 0; jj < 7; ++jj)
            if (jj != k) a[ii][jj] -= f * a[k][jj];
          a[ii][k] = -f * d;
        }
      a[k][k] = d;
    }
    double* dst = Dinv + (size_t)49 * i;
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
      for (int c = 0; c < 7; ++c) dst[7 * r + c] = a[r][c];
  }
  if (!spd) sc->fail = 1;
  for (int i = tid; i < n; i += blockDim.x) {
    x[i] = 0.0;
    rv[i] = g[i];
  }
  __syncthreads();
  auto precond = [&]() {  // z = D^-1 r
    for (int i = tid; i < n; i += blockDim.x) {
      const int cam = i / 7, rr = i % 7;
      const double* d = Dinv + (size_t)49 * cam + 7 * rr;
      const double* r7 = rv + (size_t)7 * cam;
      zv[i] = d[0] * r7[0] + d[1] * r7[1] + d[2] * r7[2] + d[3] * r7[3] + d[4] * r7[4] + d[5] * r7[5] + d[6] * r7[6];
    }
    __syncthreads();
  };
  precond();
  for (int i = tid; i < n; i += blockDim.x) pv[i] = zv[i];
  __syncthreads();
  double rz = dot(rv, zv);
  const double rz0 = rz;
  int it = 0;
  bool fail = false;
  const int l49 = lane < 49 ? lane : lane - 49;
  const int r = l49 % 7, c = l49 / 7;
  while (it < max_iter && rz > tol2 * rz0 && rz > 0.0) {
    // q = S p : wavefront per block row, lane = entry (r, c) of the column-major block
    for (int row = wave; row < nc; row += nw) {
      double acc = 0.0;
      for (int k = rptr[row]; k < rptr[row + 1]; ++k)
        acc += S[(size_t)49 * k + l49] * pv[(size_t)7 * cidx[k] + c];
      const double s = ldl_sum_over_c(lane < 49 ? acc : 0.0, r);
      if (lane < 7) qv[(size_t)7 * row + lane] = s;
    }
    __syncthreads();
    const double pq = dot(pv, qv);
    if (!(pq > 0.0) || !(pq < DBL_MAX)) { fail = true; break; }
    const double alpha = rz / pq;
    for (int i = tid; i < n; i += blockDim.x) {
      x[i] += alpha * pv[i];
      rv[i] -= alpha * qv[i];
    }
    __syncthreads();
    precond();
    const double rzn = dot(rv, zv);
    const double beta = rzn / rz;
    for (int i = tid; i < n; i += blockDim.x) pv[i] = zv[i] + beta * pv[i];
    __syncthreads();
    rz = rzn;
    ++it;
  }
  if (tid == 0) {
    sc->pcg_iters = it;
    if (fail || !(rz >= 0.0)) sc->fail = 1;
    sc->pcg_rel = rz0 > 0 ? sqrt(fabs(rz) / rz0) : 0.0;
  }
}

// per point: dx_p = Hinv b_p - sum_o Z_o^T dx_c(cam(o))
__global__ __launch_bounds__(WG) void k_ba_backsub(int np, const int32_t* __restrict__ pptr,
                                                   const int32_t* __restrict__ pobs,
                                                   const int32_t* __restrict__ oc,
                                                   const double* __restrict__ Hinv,
                                                   const double* __restrict__ bp,
                                                   const double* __restrict__ Z,
                                                   const double* __restrict__ xc, double* __restrict__ xp) {
  const int p = blockIdx.x * WG + threadIdx.x;
  if (p >= np) return;
  const double* Hi = Hinv + (size_t)9 * p;
  const double* b = bp + (size_t)3 * p;
  double d[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = Hi[3 * c] * b[0] + Hi[3 * c + 1] * b[1] + Hi[3 * c + 2] * b[2];
  for (int k = pptr[p]; k < pptr[p + 1]; ++k) {
    const int o = pobs[k];
    const double* z = Z + (size_t)18 * o;
    const double* x6 = xc + (size_t)7 * oc[o];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) s += z[3 * r + c] * x6[r];
      d[c] -= s;
    }
  }
  xp[3 * (size_t)p] = d[0]; xp[3 * (size_t)p + 1] = d[1]; xp[3 * (size_t)p + 2] = d[2];
}

// VertexSE3Expmap::oplusImpl: T <- SE3Quat::exp([omega, upsilon]) T; points: p += dx
__global__ __launch_bounds__(WG) void k_ba_update(int nc, int np, const double* __restrict__ xc,
                                                  const double* __restrict__ xp,
                                                  const uint8_t* __restrict__ fixed, Cam* cams, double* pts,
                                                  const Scal* sc) {
  if (sc->fail) return;  // the host rejects the trial
  const int t = blockIdx.x * WG + threadIdx.x;
  if (t < nc && !fixed[t]) {
    Cam cm = cams[t];
    ba_se3_oplus(xc + (size_t)7 * t, cm.q, cm.t);
    cams[t] = cm;
  }
  if (t < 3 * np) pts[t] += xp[t];
}

// robustified chi2 (fixed-order block partials) and, with x given, the scale term x.(lambda x + b)
__global__ __launch_bounds__(WG) void k_ba_chi2(ObsArgs A, double* __restrict__ partials) {
  __shared__ double sh[WG];
  double acc = 0.0;
  for (int o = blockIdx.x * WG + threadIdx.x; o < A.n_obs; o += gridDim.x * WG) {
    double R[9], X[3], e[2], rho, w;
    ba_residual(A, o, R, X, e);
    ba_huber(A.omega * (e[0] * e[0] + e[1] * e[1]), A.huber, rho, w);
    acc += rho;
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = WG / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(WG) void k_ba_scale(int n, const double* __restrict__ x,
                                                 const double* __restrict__ b, double lambda,
                                                 double* __restrict__ partials) {
  __shared__ double sh[WG];
  double acc = 0.0;
  for (int i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) acc += x[i] * (lambda * x[i] + b[i]);
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = WG / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// out[0] = sum of pa (chi2) ; out[1] = sum of pb + sum of pc (scale) ; out[2] = max of the two diag arrays
__global__ __launch_bounds__(WG) void k_ba_final(const double* __restrict__ pa, int na,
                                                 const double* __restrict__ pb, int nb,
                                                 const double* __restrict__ pc, int ncn,
                                                 const double* __restrict__ d1, int n1,
                                                 const double* __restrict__ d2, int n2, Scal* sc) {
  __shared__ double sh[WG];
  auto sum = [&](const double* p, int n) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += WG) a += p[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int off = WG / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
      __syncthreads();
    }
    const double v = sh[0];
    __syncthreads();
    return v;
  };
  if (pa) {
    const double v = sum(pa, na);
    if (threadIdx.x == 0) sc->chi2 = v;
  }
  if (pb) {
    const double v = sum(pb, nb) + sum(pc, ncn);
    if (threadIdx.x == 0) sc->scale = v;
  }
  if (d1) {
    double m = 0.0;
    for (int i = threadIdx.x; i < n1; i += WG) m = fmax(m, d1[i]);
    for (int i = threadIdx.x; i < n2; i += WG) m = fmax(m, d2[i]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int off = WG / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + off]);
      __syncthreads();
    }
    if (threadIdx.x == 0) sc->maxdiag = sh[0];
  }
}

#include "ba_cov_kernels.hpp"

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Problem {
  std::vector<Cam> cams;
  std::vector<double> pts;  // 3 per point
  std::vector<int32_t> oc, op;
  std::vector<uint8_t> cam_fixed;
  std::vector<double> uv;
  double f = 718.856, cx = 607.1928, cy = 185.2157;  // kitti_surf.cpp:52-57, bal_example.cpp:90-91
  sim3opt_ba_options opt;
  std::vector<sim3opt_iter_stats> stats;
  std::string err;
  // device
  bool ready = false;
  hipStream_t stream = nullptr;
  sim3opt::DevArena mem;  // every device block of initialize() (the library's block cache: an out-of-memory hipMalloc
                          // elsewhere flushes it)
  Cam *d_cams = nullptr, *d_cams_bk = nullptr;
  double *d_pts = nullptr, *d_pts_bk = nullptr, *d_uv = nullptr, *d_lin = nullptr, *d_Z = nullptr;
  double *d_Hinv = nullptr, *d_bp = nullptr, *d_pdmax = nullptr, *d_cdmax = nullptr;
  double *d_S = nullptr, *d_g = nullptr, *d_bc = nullptr, *d_xc = nullptr, *d_xp = nullptr;
  double *d_r = nullptr, *d_z = nullptr, *d_p = nullptr, *d_q = nullptr, *d_Dinv = nullptr;
  double *d_pa = nullptr, *d_pb = nullptr, *d_pc = nullptr;
  int32_t *d_oc = nullptr, *d_op = nullptr, *d_pptr = nullptr, *d_pobs = nullptr, *d_cptr = nullptr,
          *d_cobs = nullptr, *d_brow = nullptr, *d_bcol = nullptr, *d_sptr = nullptr, *d_sa = nullptr,
          *d_sb = nullptr, *d_rptr = nullptr;
  uint8_t* d_fixed = nullptr;
  Scal *d_sc = nullptr, *h_sc = nullptr;
  int32_t nblk = 0;
  int grid_chi = 1;
  sim3opt::BlockLdl direct;  // exact factorisation of the reduced camera system (not ready: PCG fallback)
  // sim3opt_ba_covariances: a factorisation context of its own (with the selected inversion), built at the first call
  sim3opt::BlockLdl cov_factor;
  sim3opt::DevArena cov_mem;
  std::string cov_refused;  // why the plan was refused (remembered until the problem changes)
  CovTables cov_tab;
  int32_t *d_cslot = nullptr, *d_ctrans = nullptr, *d_cmask = nullptr, *d_cflags = nullptr;
  double *d_Zc = nullptr, *d_C = nullptr;  // S^-1 on S's blocks: as picked (7x7), masked and compacted (6x6)
  int64_t cov_stats[6] = {0, 0, 0, 0, 0, 0};

  ~Problem() { release(); }
  void release() {
    if (stream) (void)hipStreamSynchronize(stream);
    direct.release();
    cov_factor.release();
    cov_mem.release();
    cov_refused.clear();
    cov_tab = CovTables();
    mem.release();
    if (h_sc) (void)hipHostFree(h_sc);
    h_sc = nullptr;
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
    ready = false;
  }
  int nc() const { return (int)cams.size(); }
  int np() const { return (int)(pts.size() / 3); }
  int no() const { return (int)oc.size(); }

  // (synchronous copies and memsets on the null stream: initialize() ends with a device-wide synchronisation)
  template <typename T>
  hipError_t up(T*& d, const std::vector<T>& h) { return mem.upload(d, h, nullptr, nullptr); }
  hipError_t alloc(double*& d, size_t n) { return mem.alloc(d, n, nullptr); }

  int initialize() {
    release();
    if (int rc = sim3opt::select_device(opt.device, err)) return rc;
    const int NC = nc(), NP = np(), NO = no();
    if (NC < 1 || NP < 1 || NO < 1) { err = "empty problem"; return SIM3OPT_ERR_STATE; }
    // observation lists per point / per camera, ascending observation index
    std::vector<int32_t> pptr(NP + 1, 0), cptr(NC + 1, 0), pobs(NO), cobs(NO);
    for (int o = 0; o < NO; ++o) { ++pptr[op[o] + 1]; ++cptr[oc[o] + 1]; }
    for (int p = 0; p < NP; ++p) pptr[p + 1] += pptr[p];
    for (int c = 0; c < NC; ++c) cptr[c + 1] += cptr[c];
    {
      std::vector<int32_t> fp(pptr.begin(), pptr.end() - 1), fc(cptr.begin(), cptr.end() - 1);
      for (int o = 0; o < NO; ++o) { pobs[fp[op[o]]++] = o; cobs[fc[oc[o]]++] = o; }
    }
    // reduced camera system: blocks (i, j) for cameras sharing a point (and every diagonal), with
    // the observation pairs behind each block in (point, o1, o2) order
    std::map<std::pair<int32_t, int32_t>, std::vector<std::pair<int32_t, int32_t>>> blocks;
    for (int c = 0; c < NC; ++c) blocks[{c, c}];
    for (int p = 0; p < NP; ++p)
      for (int a = pptr[p]; a < pptr[p + 1]; ++a)
        for (int b = pptr[p]; b < pptr[p + 1]; ++b)
          blocks[{oc[pobs[a]], oc[pobs[b]]}].push_back({pobs[a], pobs[b]});
    // block-CSR, diagonal block first in every row
    std::vector<int32_t> rptr(NC + 1, 0), brow, bcol, sptr(1, 0), sa, sb;
    for (int pass = 0; pass < 1; ++pass) {
      int32_t cur = -1;
      std::vector<std::pair<std::pair<int32_t, int32_t>, const std::vector<std::pair<int32_t, int32_t>>*>> rowblk;
      auto flush = [&]() {
        if (cur < 0) return;
        // diagonal first
        std::stable_sort(rowblk.begin(), rowblk.end(), [&](const auto& x, const auto& y) {
          const bool dx = x.first.second == cur, dy = y.first.second == cur;
          if (dx != dy) return dx;
          return x.first.second < y.first.second;
        });
        for (auto& rb : rowblk) {
          brow.push_back(rb.first.first);
          bcol.push_back(rb.first.second);
          for (auto& pr : *rb.second) { sa.push_back(pr.first); sb.push_back(pr.second); }
          sptr.push_back((int32_t)sa.size());
        }
        rptr[cur + 1] = (int32_t)brow.size();
        rowblk.clear();
      };
      for (auto& kv : blocks) {
        if (kv.first.first != cur) { flush(); cur = kv.first.first; }
        rowblk.push_back({kv.first, &kv.second});
      }
      flush();
    }
    for (int c = 0; c < NC; ++c) rptr[c + 1] = std::max(rptr[c + 1], rptr[c]);
    nblk = (int32_t)brow.size();
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIPCHK(up(d_cams, cams));
    HIPCHK(mem.raw(d_cams_bk, (size_t)NC));
    HIPCHK(up(d_pts, pts));
    HIPCHK(alloc(d_pts_bk, 3 * (size_t)NP));
    HIPCHK(up(d_uv, uv));
    HIPCHK(up(d_oc, oc)); HIPCHK(up(d_op, op));
    HIPCHK(up(d_pptr, pptr)); HIPCHK(up(d_pobs, pobs)); HIPCHK(up(d_cptr, cptr)); HIPCHK(up(d_cobs, cobs));
    HIPCHK(up(d_brow, brow)); HIPCHK(up(d_bcol, bcol)); HIPCHK(up(d_sptr, sptr)); HIPCHK(up(d_sa, sa)); HIPCHK(up(d_sb, sb));
    HIPCHK(up(d_rptr, rptr));
    cam_fixed.resize(NC, 0);
    HIPCHK(up(d_fixed, cam_fixed));
    // the reduced camera system's factorisation plan (nested dissection, level schedule: direct.hpp)
    if (opt.linear_solver != 0) {
      int64_t max_pairs = 8000000;
      if (const char* ev = std::getenv("SIM3OPT_BA_MAX_PAIRS")) max_pairs = std::atoll(ev);
      // bottom subtrees of up to a sixth of the cameras, 8 wavefronts each: the reduced system of a
      // camera chain is a wide band (tracks span several keyframes), its separators are several
      // columns wide and the top of the tree is expensive -- more of it goes to the parallel groups
      // than for the pose graphs (profiles/r2_ba_sweep.log)
      const int32_t subtree = std::max(16, NC / 6);
      std::string why;
      if (direct.build_plan(NC, rptr.data(), bcol.data(), max_pairs, subtree, "SIM3OPT_BA", false, why)) {
        HIPCHK(direct.upload(stream));  // (synchronised below)
        const sim3opt::DirectPlan& P = direct.plan();
        if (opt.verbose)
          std::fprintf(stderr, "sim3opt ba: exact block Cholesky of the reduced system: %d cameras, %lld blocks in L, "
                       "%lld block products, tree height %d, %d groups\n", NC, (long long)P.nL,
                       (long long)P.npairs, P.height, P.ngroups());
      } else if (opt.linear_solver == 1) {
        err = "linear_solver = 1: " + why;
        return SIM3OPT_ERR_ARG;
      } else if (opt.verbose) {
        std::fprintf(stderr, "sim3opt ba: no exact factorisation (%s): PCG\n", why.c_str());
      }
    }
    HIPCHK(alloc(d_lin, 20 * (size_t)NO)); HIPCHK(alloc(d_Z, 18 * (size_t)NO));
    HIPCHK(alloc(d_Hinv, 9 * (size_t)NP)); HIPCHK(alloc(d_bp, 3 * (size_t)NP)); HIPCHK(alloc(d_pdmax, NP));
    HIPCHK(alloc(d_cdmax, 7 * (size_t)NC));
    HIPCHK(alloc(d_S, 49 * (size_t)nblk)); HIPCHK(alloc(d_g, 7 * (size_t)NC)); HIPCHK(alloc(d_bc, 7 * (size_t)NC));
    HIPCHK(alloc(d_xc, 7 * (size_t)NC)); HIPCHK(alloc(d_xp, 3 * (size_t)NP));
    HIPCHK(alloc(d_r, 7 * (size_t)NC)); HIPCHK(alloc(d_z, 7 * (size_t)NC)); HIPCHK(alloc(d_p, 7 * (size_t)NC));
    HIPCHK(alloc(d_q, 7 * (size_t)NC)); HIPCHK(alloc(d_Dinv, 49 * (size_t)NC));
    grid_chi = std::max(1, std::min(1024, (NO + WG - 1) / WG));
    HIPCHK(alloc(d_pa, 1024)); HIPCHK(alloc(d_pb, 1024)); HIPCHK(alloc(d_pc, 1024));
    HIPCHK(mem.alloc(d_sc, 1, nullptr));
    HIPCHK(hipHostMalloc((void**)&h_sc, sizeof(Scal)));
    // the uploads and memsets above ran on the null stream, the kernels run on a non-blocking one:
    // order them (engine.hip ends its init the same way)
    HIPCHK(hipDeviceSynchronize());
    ready = true;
    return SIM3OPT_OK;
  }

  ObsArgs oargs() const {
    return ObsArgs{no(), d_oc, d_op, d_uv, d_cams, d_pts, f, cx, cy,
                   1.0 / (opt.pixel_noise * opt.pixel_noise), opt.huber_delta};
  }
  int fetch() {
    HIPCHK(hipMemcpyAsync(h_sc, d_sc, sizeof(Scal), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return SIM3OPT_OK;
  }
  int chi2(double* out) {
    hipLaunchKernelGGL(k_ba_chi2, dim3(grid_chi), dim3(WG), 0, stream, oargs(), d_pa);
    hipLaunchKernelGGL(k_ba_final, dim3(1), dim3(WG), 0, stream, (const double*)d_pa, grid_chi,
                       (const double*)nullptr, 0, (const double*)nullptr, 0, (const double*)nullptr, 0,
                       (const double*)nullptr, 0, d_sc);
    HIPCHK(hipGetLastError());
    int rc = fetch();
    if (rc) return rc;
    *out = h_sc->chi2;
    return SIM3OPT_OK;
  }

  // ---- the launches of one LM iteration, shared by optimize() and the diagnostic read-outs ----
  int gobs() const { return (no() + WG - 1) / WG; }
  int gpts() const { return (np() + WG - 1) / WG; }
  void launch_linearize() {
    hipLaunchKernelGGL(k_ba_obs, dim3(gobs()), dim3(WG), 0, stream, oargs(), d_lin);
  }
  int backup() {
    HIPCHK(hipMemcpyAsync(d_cams_bk, d_cams, sizeof(Cam) * nc(), hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_pts_bk, d_pts, sizeof(double) * 3 * np(), hipMemcpyDeviceToDevice, stream));
    return SIM3OPT_OK;
  }
  int restore() {
    HIPCHK(hipMemcpyAsync(d_cams, d_cams_bk, sizeof(Cam) * nc(), hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_pts, d_pts_bk, sizeof(double) * 3 * np(), hipMemcpyDeviceToDevice, stream));
    return SIM3OPT_OK;
  }
  // H_pp^-1, b_p, Z, then S, g, b_c and the undamped diagonals, for the damping `lambda`
  void launch_reduced(double lambda) {
    hipLaunchKernelGGL(k_ba_points, dim3(gpts()), dim3(WG), 0, stream, np(), d_pptr, d_pobs, d_lin, lambda,
                       d_Hinv, d_bp, d_pdmax);
    hipLaunchKernelGGL(k_ba_obs2, dim3(gobs()), dim3(WG), 0, stream, no(), d_op, d_lin, d_Hinv, d_Z);
    hipLaunchKernelGGL(k_ba_reduced, dim3((nblk + 3) / 4), dim3(WG), 0, stream, nblk, d_brow, d_bcol,
                       d_sptr, d_sa, d_sb, d_op, d_lin, d_Z, d_bp, d_fixed, lambda, d_S, d_g, d_bc,
                       d_cdmax);
  }
  void launch_maxdiag() {
    hipLaunchKernelGGL(k_ba_final, dim3(1), dim3(WG), 0, stream, (const double*)nullptr, 0,
                       (const double*)nullptr, 0, (const double*)nullptr, 0, (const double*)d_pdmax, np(),
                       (const double*)d_cdmax, 7 * nc(), d_sc);
  }
  // pcg_iters, fail and pcg_rel (contiguous in Scal): what a solver leaves behind.  The exact solver writes only
  // `fail`, so a pcg_rel left by an earlier k_ba_pcg launch (a read-out may ask for one) must not reach the statistics.
  int clear_solver_flags() {
    static_assert(offsetof(Scal, pcg_rel) == offsetof(Scal, pcg_iters) + 2 * sizeof(int32_t), "Scal layout");
    HIPCHK(hipMemsetAsync(&d_sc->pcg_iters, 0, 2 * sizeof(int32_t) + sizeof(double), stream));
    return SIM3OPT_OK;
  }
  // S dx_c = g: the exact block Cholesky, or the one-workgroup PCG with the given cap (0: automatic) and tolerance
  int launch_solve(bool exact, int pcg_max_iters, double pcg_rel_tol) {
    if (exact) {
      direct.gather(d_S, d_g, stream);
      HIPCHK(direct.factor(0.0, &d_sc->fail, 1, d_xc, stream));  // lambda 0: S carries the damping already
    } else {
      hipLaunchKernelGGL(k_ba_pcg, dim3(1), dim3(1024), 0, stream, nc(), d_rptr, d_bcol, d_S, d_g, d_xc, d_r,
                         d_z, d_p, d_q, d_Dinv, pcg_max_iters > 0 ? pcg_max_iters : 20 * nc() + 100,
                         pcg_rel_tol * pcg_rel_tol, d_sc);
    }
    return SIM3OPT_OK;
  }
  void launch_backsub() {
    hipLaunchKernelGGL(k_ba_backsub, dim3(gpts()), dim3(WG), 0, stream, np(), d_pptr, d_pobs, d_oc, d_Hinv,
                       d_bp, d_Z, d_xc, d_xp);
  }
  void launch_update() {
    hipLaunchKernelGGL(k_ba_update, dim3((std::max(nc(), 3 * np()) + WG - 1) / WG), dim3(WG), 0, stream, nc(), np(),
                       d_xc, d_xp, d_fixed, d_cams, d_pts, (const Scal*)d_sc);
  }
  // chi2 of the estimate and scale = x.(lambda x + b) over cameras and points, into d_sc
  void launch_trial_sums(double lambda) {
    const int NC = nc(), NP = np();
    const int gsc = std::max(1, std::min(1024, (7 * NC + WG - 1) / WG));
    const int gsp = std::max(1, std::min(1024, (3 * NP + WG - 1) / WG));
    hipLaunchKernelGGL(k_ba_scale, dim3(gsc), dim3(WG), 0, stream, 7 * NC, d_xc, d_bc, lambda, d_pb);
    hipLaunchKernelGGL(k_ba_scale, dim3(gsp), dim3(WG), 0, stream, 3 * NP, d_xp, d_bp, lambda, d_pc);
    hipLaunchKernelGGL(k_ba_chi2, dim3(grid_chi), dim3(WG), 0, stream, oargs(), d_pa);
    hipLaunchKernelGGL(k_ba_final, dim3(1), dim3(WG), 0, stream, (const double*)d_pa, grid_chi,
                       (const double*)d_pb, gsc, (const double*)d_pc, gsp, (const double*)nullptr, 0,
                       (const double*)nullptr, 0, d_sc);
  }

  int optimize(int max_iters) {
    stats.clear();
    const int NC = nc(), NP = np();
    LmDamping damp;
    bool ok = true;
    int iters = 0;
    for (int it = 0; it < max_iters && ok; ++it) {
      sim3opt_iter_stats T{};
      double currentChi = 0.0;
      int rc = chi2(&currentChi);
      if (rc) return rc;
      T.chi2_before = currentChi;
      launch_linearize();
      double rho = 0.0;
      int qmax = 0;
      do {
        rc = backup();
        if (rc) return rc;
        if (it == 0 && qmax == 0) {
          double maxdiag = 0.0;
          if (!(opt.user_lambda_init > 0)) {
            // computeLambdaInit: tau * max diagonal entry of the (undamped) Hessian over all vertices
            launch_reduced(1.0);
            launch_maxdiag();
            HIPCHK(hipGetLastError());
            rc = fetch();
            if (rc) return rc;
            maxdiag = h_sc->maxdiag;
          }
          damp.start(opt.user_lambda_init, opt.tau, maxdiag);
        }
        const double lambda = damp.lambda;
        rc = clear_solver_flags();
        if (rc) return rc;
        launch_reduced(lambda);
        rc = launch_solve(direct.ready(), opt.pcg_max_iters, opt.pcg_rel_tol);
        if (rc) return rc;
        launch_backsub();
        launch_update();
        launch_trial_sums(lambda);
        HIPCHK(hipGetLastError());
        rc = fetch();
        if (rc) return rc;
        T.pcg_iters += h_sc->pcg_iters;
        T.pcg_rel_res = h_sc->pcg_rel;
        const double tempChi = h_sc->fail ? DBL_MAX : h_sc->chi2;
        const double scale = h_sc->fail ? 0.0 : h_sc->scale;
        if (damp.update(currentChi, tempChi, scale, 1.0 / 3.0, 2.0 / 3.0, rho)) {
          currentChi = tempChi;
        } else {
          rc = restore();
          if (rc) return rc;
        }
        ++qmax;
      } while (rho < 0 && qmax < opt.max_trials);
      T.chi2_after = currentChi;
      T.lambda = damp.lambda;
      T.rho = rho;
      T.trials = qmax;
      stats.push_back(T);
      ++iters;
      if (opt.verbose)
        std::fprintf(stderr, "ba iteration= %d\t chi2= %.9g\t lambda= %.6g\t levenbergIter= %d\t pcg= %d (rel %.1e)\n",
                     it, currentChi, damp.lambda, qmax, T.pcg_iters, T.pcg_rel_res);
      if (damp.terminate(qmax, opt.max_trials, rho)) ok = false;
    }
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipMemcpy(cams.data(), d_cams, sizeof(Cam) * NC, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pts.data(), d_pts, sizeof(double) * 3 * NP, hipMemcpyDeviceToHost));
    return iters;
  }

  // ---- diagnostic read-outs: the launches above, then copies to the host.  Every buffer they write is one
  // optimize() rewrites before it reads it, and the estimate is restored from the trial's backup buffers. ----
  int down(void* dst, const void* src, size_t bytes) {
    if (!dst || !bytes) return SIM3OPT_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return SIM3OPT_OK;
  }
  int read_lin(double* lin) {
    launch_linearize();
    HIPCHK(hipGetLastError());
    return down(lin, d_lin, sizeof(double) * 20 * no());
  }
  int read_reduced(double lambda, double* S, double* g, double* bc, double* Hinv, double* bp, double* Z,
                   double* pdmax, double* cdmax, double* maxdiag) {
    launch_linearize();
    launch_reduced(lambda);
    launch_maxdiag();
    HIPCHK(hipGetLastError());
    int rc = fetch();
    if (rc) return rc;
    if (maxdiag) *maxdiag = h_sc->maxdiag;
    const size_t NC = nc(), NP = np(), NO = no(), D = sizeof(double);
    if ((rc = down(S, d_S, D * 49 * nblk)) || (rc = down(g, d_g, D * 7 * NC)) || (rc = down(bc, d_bc, D * 7 * NC)) ||
        (rc = down(Hinv, d_Hinv, D * 9 * NP)) || (rc = down(bp, d_bp, D * 3 * NP)) || (rc = down(Z, d_Z, D * 18 * NO)) ||
        (rc = down(pdmax, d_pdmax, D * NP)) || (rc = down(cdmax, d_cdmax, D * 7 * NC)))
      return rc;
    return SIM3OPT_OK;
  }
  int read_step(double lambda, bool exact, int pcg_max_iters, double pcg_rel_tol, double* dxc, double* dxp,
                int32_t* iters, double* rel, int32_t* fail) {
    launch_linearize();
    int rc = clear_solver_flags();
    if (rc) return rc;
    launch_reduced(lambda);
    rc = launch_solve(exact, pcg_max_iters, pcg_rel_tol);
    if (rc) return rc;
    launch_backsub();
    HIPCHK(hipGetLastError());
    rc = fetch();
    if (rc) return rc;
    if (iters) *iters = h_sc->pcg_iters;
    if (rel) *rel = exact ? 0.0 : h_sc->pcg_rel;
    if (fail) *fail = h_sc->fail;
    if ((rc = down(dxc, d_xc, sizeof(double) * 7 * nc())) || (rc = down(dxp, d_xp, sizeof(double) * 3 * np())))
      return rc;
    return clear_solver_flags();
  }
  int read_update(const double* dxc, const double* dxp, double lambda, bool with_fail, double* cam_qt, double* points,
                  double* chi2_out, double* scale_out) {
    const int NC = nc(), NP = np();
    launch_linearize();
    launch_reduced(lambda);  // b_c, b_p of the scale term
    int rc = backup();
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(d_xc, dxc, sizeof(double) * 7 * NC, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_xp, dxp, sizeof(double) * 3 * NP, hipMemcpyHostToDevice, stream));
    const int32_t flags[2] = {0, with_fail ? 1 : 0};  // pcg_iters, fail
    HIPCHK(hipMemcpyAsync(&d_sc->pcg_iters, flags, sizeof(flags), hipMemcpyHostToDevice, stream));
    launch_update();
    launch_trial_sums(lambda);
    HIPCHK(hipGetLastError());
    rc = fetch();
    if (rc) return rc;
    if (chi2_out) *chi2_out = h_sc->chi2;
    if (scale_out) *scale_out = h_sc->scale;
    std::vector<Cam> hc(cam_qt ? NC : 0);
    if ((rc = down(hc.data(), d_cams, sizeof(Cam) * hc.size())) || (rc = down(points, d_pts, sizeof(double) * 3 * NP)))
      return rc;
    for (size_t c = 0; c < hc.size(); ++c) {
      for (int i = 0; i < 4; ++i) cam_qt[7 * c + i] = hc[c].q[i];
      for (int i = 0; i < 3; ++i) cam_qt[7 * c + 4 + i] = hc[c].t[i];
    }
    rc = restore();
    if (rc) return rc;
    rc = clear_solver_flags();
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(stream));
    return SIM3OPT_OK;
  }

  // ---- covariances (include/sim3opt.h, sim3opt_ba_covariances).  Like the read-outs above the call writes only
  // buffers optimize() rewrites before it reads them (d_lin, H_pp^-1, b_p, Z, S, g, b_c, the diagonals and
  // d_sc->maxdiag); the factorisation, its flags and everything else are the context's own. ----
  int cov_init() {
    if (!cov_refused.empty()) { err = cov_refused; return SIM3OPT_ERR_STATE; }
    const int NC = nc();
    std::vector<int32_t> rptr((size_t)NC + 1), bcol((size_t)nblk);
    int rc;
    if ((rc = down(rptr.data(), d_rptr, sizeof(int32_t) * rptr.size())) ||
        (rc = down(bcol.data(), d_bcol, sizeof(int32_t) * bcol.size())))
      return rc;
    // the plan the LM's factorisation uses (same knobs), with the limit of an explicit request
    int64_t max_pairs = 30000000;
    if (const char* ev = std::getenv("SIM3OPT_BA_MAX_PAIRS")) max_pairs = std::atoll(ev);
    if (const char* ev = std::getenv("SIM3OPT_BA_COV_MAX_PAIRS")) max_pairs = std::atoll(ev);
    const int32_t subtree = std::max(16, NC / 6);
    std::string why;
    if (!cov_factor.build_plan(NC, rptr.data(), bcol.data(), max_pairs, subtree, "SIM3OPT_BA", true, why)) {
      cov_refused = "ba_covariances: " + why;
      err = cov_refused;
      return SIM3OPT_ERR_STATE;
    }
    const sim3opt::DirectPlan& P = cov_factor.plan();
    const CovFactorPattern F{P.nb, P.perm.data(), P.colptr.data(), P.lrow.data()};
    why = cov_build_tables(NC, np(), oc, op, cam_fixed, rptr, bcol, F, cov_tab);
    if (!why.empty()) {
      cov_factor.release();
      cov_refused = "ba_covariances: " + why;
      err = cov_refused;
      return SIM3OPT_ERR_STATE;
    }
    auto body = [&]() -> int {
      HIPCHK(cov_factor.upload(stream));
      HIPCHK(cov_mem.upload(d_cslot, cov_tab.sslot, stream, nullptr));
      HIPCHK(cov_mem.upload(d_ctrans, cov_tab.strans, stream, nullptr));
      HIPCHK(cov_mem.upload(d_cmask, cov_tab.smask, stream, nullptr));
      HIPCHK(cov_mem.alloc(d_cflags, 4, stream));
      HIPCHK(cov_mem.alloc(d_Zc, 49 * (size_t)nblk, stream));
      HIPCHK(cov_mem.alloc(d_C, 36 * (size_t)nblk, stream));
      return SIM3OPT_OK;
    };
    rc = body();
    const hipError_t es = hipStreamSynchronize(stream);  // (the uploads read this frame's tables)
    if (rc == SIM3OPT_OK && es != hipSuccess) {
      err = std::string("ba_covariances: ") + hipGetErrorString(es);
      rc = SIM3OPT_ERR_HIP;
    }
    if (rc) {
      cov_factor.release();
      cov_mem.release();
      return rc;
    }
    if (opt.verbose)
      std::fprintf(stderr, "sim3opt ba: covariances: %d cameras, %lld blocks of L / Z, %lld + %lld block products, %d groups\n",
                   NC, (long long)P.nL, (long long)P.npairs, (long long)cov_factor.selinv_plan().nprod, P.ngroups());
    return SIM3OPT_OK;
  }

  int covariances(double lambda, int32_t n_cc, const int32_t* cam_a, const int32_t* cam_b, double* cov_cc, int32_t n_pp,
                  const int32_t* point, double* cov_pp, int32_t n_pc, const int32_t* pc_point, const int32_t* pc_cam,
                  double* cov_pc) {
    const std::string pre = "ba_covariances: ";
    if (!cov_factor.ready()) {
      int rc = cov_init();
      if (rc) return rc;
    }
    const sim3opt::DirectPlan& P = cov_factor.plan();
    const CovFactorPattern F{P.nb, P.perm.data(), P.colptr.data(), P.lrow.data()};
    CovRequest R;
    const std::string bad = cov_plan_request(cov_tab, F, oc, cam_fixed, n_cc, cam_a, cam_b, n_pp, point, n_pc, pc_point,
                                             pc_cam, R);
    if (!bad.empty()) { err = pre + bad; return SIM3OPT_ERR_ARG; }
    const int32_t npick = (int32_t)R.slot.size(), nup = (int32_t)R.upoint.size(), nx = (int32_t)R.xptr.size() - 1;
    const bool invert = npick > 0 || nup > 0;
    cov_stats[0] = P.nb; cov_stats[1] = P.nL; cov_stats[2] = P.npairs; cov_stats[3] = cov_factor.selinv_plan().nprod;
    cov_stats[4] = R.pair_terms; cov_stats[5] = invert ? 1 : 0;
    const int NC = nc(), NP = np();
    // ---- the system at the current estimates, the points' pivots ----
    launch_linearize();
    launch_reduced(lambda);
    launch_maxdiag();
    HIPCHK(hipMemsetAsync(d_cflags, 0, 4 * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_ba_cov_point_pivots, dim3(gpts()), dim3(WG), 0, stream, NP, d_pptr, d_pobs, d_lin, lambda,
                       d_pdmax, d_cflags);
    HIPCHK(hipGetLastError());
    int32_t hflags[4] = {0, 0, 0, 0};
    int rc = down(hflags, d_cflags, sizeof(hflags));
    if (rc) return rc;
    if (hflags[2] != 0) {
      // (S holds the inverse of a singular block: it is not factored)
      err = pre + "point " + std::to_string(NP - hflags[2]) + ": H_pp + lambda I is numerically singular (a pivot of its "
            "LDL^T below 1e-13 of its largest diagonal entry): a point seen once or without parallax wants lambda > 0";
      return SIM3OPT_ERR_STATE;
    }
    // ---- S = L L^T and S^-1 on the pattern of L ----
    hipLaunchKernelGGL(k_ba_cov_pads, dim3((NC + WG - 1) / WG), dim3(WG), 0, stream, NC, d_rptr, d_fixed,
                       (const Scal*)d_sc, d_S);
    cov_factor.gather(d_S, d_g, stream);
    HIPCHK(cov_factor.factor(0.0, d_cflags, 1, nullptr, stream));  // lambda 0: S carries the damping already
    cov_factor.selinv(reinterpret_cast<const unsigned long long*>(&d_sc->maxdiag), d_cflags + 1, stream, invert);
    HIPCHK(hipGetLastError());
    // ---- the blocks ----
    // per-call indices, one upload: [slot | trans | mask | upoint | xptr | xobs | xpick]
    std::vector<int32_t> idx;
    idx.reserve(3 * (size_t)npick + nup + R.xptr.size() + 2 * R.xobs.size());
    const size_t o_slot = 0, o_trans = (size_t)npick, o_mask = 2 * (size_t)npick, o_up = 3 * (size_t)npick,
                 o_xptr = o_up + nup, o_xobs = o_xptr + R.xptr.size(), o_xpick = o_xobs + R.xobs.size();
    idx.insert(idx.end(), R.slot.begin(), R.slot.end());
    idx.insert(idx.end(), R.trans.begin(), R.trans.end());
    idx.insert(idx.end(), R.mask.begin(), R.mask.end());
    idx.insert(idx.end(), R.upoint.begin(), R.upoint.end());
    idx.insert(idx.end(), R.xptr.begin(), R.xptr.end());
    idx.insert(idx.end(), R.xobs.begin(), R.xobs.end());
    idx.insert(idx.end(), R.xpick.begin(), R.xpick.end());
    // results, one download: [picked 6x6 blocks | point blocks | point-camera blocks]
    const size_t r_pp = 36 * (size_t)npick, r_pc = r_pp + 9 * (size_t)nup, r_end = r_pc + 18 * (size_t)std::max(nx, 0);
    std::vector<double> res(std::max<size_t>(r_end, 1));
    sim3opt::DevBuf<int32_t> d_idx;
    sim3opt::DevBuf<double> d_X49, d_res;
    // (the launches above and below are on the stream: whatever ends this, they are done before the blocks go)
    auto body = [&]() -> int {
      HIPCHK(d_idx.alloc(std::max<size_t>(idx.size(), 1)));
      HIPCHK(d_X49.alloc(49 * (size_t)std::max(npick, 1)));
      HIPCHK(d_res.alloc(std::max<size_t>(r_end, 1)));
      if (!idx.empty())
        HIPCHK(hipMemcpyAsync(d_idx, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, stream));
      if (invert) {
        cov_factor.pick(d_cslot, d_ctrans, nblk, d_Zc, stream);
        hipLaunchKernelGGL(k_ba_cov_cams, dim3((36 * nblk + WG - 1) / WG), dim3(WG), 0, stream, (int)nblk,
                           (const double*)d_Zc, (const int32_t*)d_cmask, d_C);
      }
      if (npick > 0) {
        cov_factor.pick(d_idx + o_slot, d_idx + o_trans, npick, d_X49, stream);
        hipLaunchKernelGGL(k_ba_cov_cams, dim3((36 * npick + WG - 1) / WG), dim3(WG), 0, stream, (int)npick,
                           (const double*)d_X49, (const int32_t*)(d_idx + o_mask), d_res.get());
      }
      if (nup > 0) {
        const CovPointArgs A{nup, d_idx + o_up, d_pptr, d_pobs, d_oc, d_fixed, d_rptr, d_bcol, d_Z, d_Hinv, d_C,
                             d_res + r_pp};
        hipLaunchKernelGGL(k_ba_cov_points, dim3((nup + 3) / 4), dim3(WG), 0, stream, A);
      }
      if (nx > 0)
        hipLaunchKernelGGL(k_ba_cov_cross, dim3((18 * nx + WG - 1) / WG), dim3(WG), 0, stream, (int)nx,
                           (const int32_t*)(d_idx + o_xptr), (const int32_t*)(d_idx + o_xobs),
                           (const int32_t*)(d_idx + o_xpick), (const double*)d_Z, (const double*)d_res.get(),
                           d_res + r_pc);
      HIPCHK(hipGetLastError());
      if (r_end > 0) HIPCHK(hipMemcpyAsync(res.data(), d_res, sizeof(double) * r_end, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(hflags, d_cflags, sizeof(hflags), hipMemcpyDeviceToHost, stream));
      return SIM3OPT_OK;
    };
    rc = body();
    const hipError_t es = hipStreamSynchronize(stream);
    if (rc) return rc;
    HIPCHK(es);
    bool finite = true;
    for (size_t k = 0; k < r_end && finite; ++k) finite = std::isfinite(res[k]);
    if (hflags[0] || hflags[1] || !finite) {
      err = pre + (hflags[0] ? "the reduced camera system is not positive definite (a non-positive pivot)"
                   : hflags[1] ? "the reduced camera system is numerically singular (a pivot below 1e-13 max |H_dd|)"
                               : "non-finite result");
      err += ": no fixed camera, a camera nobody observes with, or lambda too small for this map";
      return SIM3OPT_ERR_STATE;
    }
    for (int32_t q = 0; q < n_cc; ++q)
      std::memcpy(cov_cc + (size_t)36 * q, res.data() + (size_t)36 * R.cc_where[q], sizeof(double) * 36);
    for (int32_t q = 0; q < n_pp; ++q)
      std::memcpy(cov_pp + (size_t)9 * q, res.data() + r_pp + (size_t)9 * R.pp_where[q], sizeof(double) * 9);
    for (int32_t q = 0; q < n_pc; ++q) {
      double* dst = cov_pc + (size_t)18 * q;
      if (R.pc_where[q] < 0) {
        for (int k = 0; k < 18; ++k) dst[k] = 0.0;
      } else {
        std::memcpy(dst, res.data() + r_pc + (size_t)18 * R.pc_where[q], sizeof(double) * 18);
      }
    }
    return SIM3OPT_OK;
  }
};

}  // namespace sim3opt_bundle

// ------------------------------------------------------------------------------------------
// C-ABI (include/sim3opt.h, "bundle adjustment hand-off")
// ------------------------------------------------------------------------------------------
using sim3opt_bundle::Problem;
struct sim3opt_ba : Problem {};

extern "C" {

void sim3opt_ba_options_default(sim3opt_ba_options* o) {
  if (!o) return;
  o->huber_delta = 2.5;   // bal_example.cpp:151
  o->pixel_noise = 1.0;   // :62
  o->tau = 1e-5;
  o->user_lambda_init = 0.0;
  o->max_trials = 10;
  o->pcg_max_iters = 0;
  o->pcg_rel_tol = 1e-12;
  o->linear_solver = -1;
  o->device = -1;
  o->verbose = 0;
}

sim3opt_ba* sim3opt_ba_create(void) { return sim3opt::handle_create<sim3opt_ba>(sim3opt_ba_options_default); }

void sim3opt_ba_destroy(sim3opt_ba* b) { sim3opt::handle_destroy(b); }

const char* sim3opt_ba_last_error(const sim3opt_ba* b) { return b ? b->err.c_str() : "null problem"; }

int sim3opt_ba_set_options(sim3opt_ba* b, const sim3opt_ba_options* o) {
  if (!b || !o) return SIM3OPT_ERR_ARG;
  if (!(o->pixel_noise > 0) || o->max_trials < 1 || !(o->tau > 0) || !(o->pcg_rel_tol >= 0) || o->huber_delta < 0 ||
      o->linear_solver < -1 || o->linear_solver > 1) {
    b->err = "ba_set_options: value out of range";
    return SIM3OPT_ERR_ARG;
  }
  if (b->ready && (o->linear_solver != b->opt.linear_solver || o->device != b->opt.device))
    b->release();  // the factorisation plan / the device are chosen at the next upload
  b->opt = *o;
  return SIM3OPT_OK;
}

int sim3opt_ba_set_problem(sim3opt_ba* b, int32_t n_cams, const double* cam_qt, int32_t n_points,
                           const double* points, int32_t n_obs, const int32_t* obs_cam,
                           const int32_t* obs_point, const double* obs_uv, double focal, double cx,
                           double cy) {
  if (!b || n_cams < 1 || n_points < 1 || n_obs < 1 || !cam_qt || !points || !obs_cam || !obs_point ||
      !obs_uv || !(focal > 0)) {
    if (b) b->err = "ba_set_problem: bad argument";
    return SIM3OPT_ERR_ARG;
  }
  return sim3opt::guarded(b, "ba_set_problem", sim3opt::NO_MEMORY, [&]() -> int {
  for (int32_t o = 0; o < n_obs; ++o)
    if (obs_cam[o] < 0 || obs_cam[o] >= n_cams || obs_point[o] < 0 || obs_point[o] >= n_points) {
      b->err = "ba_set_problem: observation index out of range";  // (the reference asserts, :140-143)
      return SIM3OPT_ERR_ARG;
    }
  using sim3opt::all_finite;
  if (!all_finite(cam_qt, 7 * (size_t)n_cams)) { b->err = "ba_set_problem: non-finite camera"; return SIM3OPT_ERR_ARG; }
  if (!all_finite(points, 3 * (size_t)n_points)) { b->err = "ba_set_problem: non-finite point"; return SIM3OPT_ERR_ARG; }
  if (!all_finite(obs_uv, 2 * (size_t)n_obs)) { b->err = "ba_set_problem: non-finite observation"; return SIM3OPT_ERR_ARG; }
  b->release();
  b->cams.resize(n_cams);
  for (int32_t c = 0; c < n_cams; ++c) {
    const double* s = cam_qt + 7 * (size_t)c;
    const double nq = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3]);
    if (!(nq > 0)) { b->err = "ba_set_problem: zero quaternion"; return SIM3OPT_ERR_ARG; }
    for (int i = 0; i < 4; ++i) b->cams[c].q[i] = s[i] / nq;
    for (int i = 0; i < 3; ++i) b->cams[c].t[i] = s[4 + i];
    b->cams[c].pad = 0.0;
  }
  b->pts.assign(points, points + 3 * (size_t)n_points);
  b->oc.assign(obs_cam, obs_cam + n_obs);
  b->op.assign(obs_point, obs_point + n_obs);
  b->uv.assign(obs_uv, obs_uv + 2 * (size_t)n_obs);
  b->f = focal; b->cx = cx; b->cy = cy;
  b->cam_fixed.assign(n_cams, 0);
  b->stats.clear();
  return SIM3OPT_OK;
  });
}

int sim3opt_ba_set_fixed_cameras(sim3opt_ba* b, const uint8_t* fixed) {
  if (!b || !fixed) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_set_fixed_cameras", sim3opt::NO_MEMORY, [&]() -> int {
  if (b->nc() < 1) { b->err = "ba_set_fixed_cameras: no problem set"; return SIM3OPT_ERR_STATE; }
  b->cam_fixed.assign(fixed, fixed + b->nc());
  for (auto& f : b->cam_fixed) f = f ? 1 : 0;
  b->release();  // the next call re-uploads
  return SIM3OPT_OK;
  });
}

// The BAL file as ba_demo reads it (bal_example.cpp:104-189): "<cams> <points> <observations>", one
// observation per line, 9 numbers per camera (angle-axis, translation, f, k1, k2 -- the last three
// read and ignored: the reference projects with its fixed CameraParameters), 3 per point.
int sim3opt_ba_read_bal(sim3opt_ba* b, const char* path, double focal, double cx, double cy) {
  if (!b || !path) return SIM3OPT_ERR_ARG;
  FILE* f = std::fopen(path, "r");
  if (!f) { b->err = std::string("cannot open ") + path; return SIM3OPT_ERR_IO; }
  int nc = 0, np = 0, no = 0;
  if (std::fscanf(f, "%d %d %d", &nc, &np, &no) != 3 || nc < 1 || np < 1 || no < 1) {
    std::fclose(f);
    b->err = "BAL header";
    return SIM3OPT_ERR_IO;
  }
  {  // counts the file cannot hold (every number takes at least two bytes) are refused before any
     // allocation is sized from them
    const long at = std::ftell(f);
    std::fseek(f, 0, SEEK_END);
    const long long bytes = std::ftell(f);
    std::fseek(f, at, SEEK_SET);
    const long long need = 2 * (4LL * no + 9LL * nc + 3LL * np);
    if (at < 0 || bytes < need) {
      std::fclose(f);
      b->err = "BAL header: counts exceed the file";
      return SIM3OPT_ERR_IO;
    }
  }
  std::vector<int32_t> oc, op;
  std::vector<double> uv, cams, pts;
  try {
    oc.resize((size_t)no); op.resize((size_t)no);
    uv.resize(2 * (size_t)no); cams.resize(7 * (size_t)nc); pts.resize(3 * (size_t)np);
  } catch (const std::exception&) {
    std::fclose(f);
    b->err = "BAL file: out of host memory";
    return SIM3OPT_ERR_ARG;
  }
  bool ok = true;
  for (size_t o = 0; o < (size_t)no && ok; ++o) ok = std::fscanf(f, "%d %d %lf %lf", &oc[o], &op[o], &uv[2 * o], &uv[2 * o + 1]) == 4;
  for (int c = 0; c < nc && ok; ++c) {
    double v[9];
    for (int j = 0; j < 9 && ok; ++j) ok = std::fscanf(f, "%lf", &v[j]) == 1;
    // ceres AngleAxisToQuaternion (called at bal_example.cpp:168)
    const double th2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    double k = 0.5, w = 1.0;
    if (th2 > 0.0) {
      const double th = std::sqrt(th2);
      k = std::sin(0.5 * th) / th;
      w = std::cos(0.5 * th);
    }
    double* s = &cams[7 * (size_t)c];
    s[0] = v[0] * k; s[1] = v[1] * k; s[2] = v[2] * k; s[3] = w;
    s[4] = v[3]; s[5] = v[4]; s[6] = v[5];
  }
  for (size_t i = 0; i < pts.size() && ok; ++i) ok = std::fscanf(f, "%lf", &pts[i]) == 1;
  std::fclose(f);
  if (!ok) { b->err = "BAL file truncated or malformed"; return SIM3OPT_ERR_IO; }
  return sim3opt_ba_set_problem(b, nc, cams.data(), np, pts.data(), no, oc.data(), op.data(), uv.data(),
                                focal, cx, cy);
}

int sim3opt_ba_dims(const sim3opt_ba* b, int32_t* n_cams, int32_t* n_points, int32_t* n_obs) {
  if (!b) return SIM3OPT_ERR_ARG;
  if (n_cams) *n_cams = b->nc();
  if (n_points) *n_points = b->np();
  if (n_obs) *n_obs = b->no();
  return SIM3OPT_OK;
}

int sim3opt_ba_chi2(sim3opt_ba* b, double* chi2) {
  if (!b || !chi2) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_chi2", sim3opt::NO_MEMORY_OR_INTERNAL, [&]() -> int {
  if (!b->ready) { int rc = b->initialize(); if (rc) return rc; }
  return b->chi2(chi2);
  });
}

// ---- diagnostic read-outs (include/sim3opt.h, "Diagnostic."): nothing in the solver uses them ----
namespace {
// the checks every read-out begins with; leaves the problem uploaded
int ba_debug_enter(sim3opt_ba* b, const char* what) {
  b->err.clear();
  if (b->no() < 1) { b->err = std::string(what) + ": no problem set"; return SIM3OPT_ERR_STATE; }
  if (!b->ready) { int rc = b->initialize(); if (rc) return rc; }
  return SIM3OPT_OK;
}
}  // namespace

int sim3opt_ba_debug_pattern(sim3opt_ba* b, int32_t* n_blocks, int32_t* rptr, int32_t* bcol) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_debug_pattern", sim3opt::NO_MEMORY_OR_INTERNAL, [&]() -> int {
  int rc = ba_debug_enter(b, "ba_debug_pattern");
  if (rc) return rc;
  if (!n_blocks || (!rptr != !bcol)) { b->err = "ba_debug_pattern: NULL output"; return SIM3OPT_ERR_ARG; }
  *n_blocks = b->nblk;
  if (!rptr) return SIM3OPT_OK;  // size query
  if ((rc = b->down(rptr, b->d_rptr, sizeof(int32_t) * (b->nc() + 1))) ||
      (rc = b->down(bcol, b->d_bcol, sizeof(int32_t) * b->nblk)))
    return rc;
  return SIM3OPT_OK;
  });
}

int sim3opt_ba_debug_linearization(sim3opt_ba* b, double* lin) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_debug_linearization", sim3opt::NO_MEMORY_OR_INTERNAL, [&]() -> int {
  int rc = ba_debug_enter(b, "ba_debug_linearization");
  if (rc) return rc;
  if (!lin) { b->err = "ba_debug_linearization: NULL output"; return SIM3OPT_ERR_ARG; }
  return b->read_lin(lin);
  });
}

int sim3opt_ba_debug_reduced(sim3opt_ba* b, double lambda, double* S, double* g, double* b_c, double* Hpp_inv,
                             double* b_p, double* Z, double* point_maxdiag, double* cam_maxdiag, double* maxdiag) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_debug_reduced", sim3opt::NO_MEMORY_OR_INTERNAL, [&]() -> int {
  int rc = ba_debug_enter(b, "ba_debug_reduced");
  if (rc) return rc;
  if (!std::isfinite(lambda)) { b->err = "ba_debug_reduced: lambda is not finite"; return SIM3OPT_ERR_ARG; }
  if (!S && !g && !b_c && !Hpp_inv && !b_p && !Z && !point_maxdiag && !cam_maxdiag && !maxdiag) {
    b->err = "ba_debug_reduced: every output is NULL";
    return SIM3OPT_ERR_ARG;
  }
  return b->read_reduced(lambda, S, g, b_c, Hpp_inv, b_p, Z, point_maxdiag, cam_maxdiag, maxdiag);
  });
}

int sim3opt_ba_debug_step(sim3opt_ba* b, double lambda, int32_t solver, int32_t pcg_max_iters, double pcg_rel_tol,
                          double* dx_c, double* dx_p, int32_t* pcg_iters, double* pcg_rel, int32_t* fail) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_debug_step", sim3opt::NO_MEMORY_OR_INTERNAL, [&]() -> int {
  int rc = ba_debug_enter(b, "ba_debug_step");
  if (rc) return rc;
  if (!std::isfinite(lambda) || solver < 0 || solver > 1 || pcg_max_iters < 0 || !(pcg_rel_tol >= 0)) {
    b->err = "ba_debug_step: value out of range";
    return SIM3OPT_ERR_ARG;
  }
  if (!dx_c || !dx_p || !fail) { b->err = "ba_debug_step: NULL output"; return SIM3OPT_ERR_ARG; }
  if (solver == 1 && !b->direct.ready()) {
    b->err = "ba_debug_step: the exact solver was asked of a problem initialised without a factorisation plan "
             "(options.linear_solver = 0, or the plan was refused)";
    return SIM3OPT_ERR_STATE;
  }
  return b->read_step(lambda, solver == 1, pcg_max_iters, pcg_rel_tol, dx_c, dx_p, pcg_iters, pcg_rel, fail);
  });
}

int sim3opt_ba_debug_update(sim3opt_ba* b, const double* dx_c, const double* dx_p, double lambda, int32_t with_fail,
                            double* cam_qt, double* points, double* chi2, double* scale) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_debug_update", sim3opt::NO_MEMORY_OR_INTERNAL, [&]() -> int {
  int rc = ba_debug_enter(b, "ba_debug_update");
  if (rc) return rc;
  if (!dx_c || !dx_p) { b->err = "ba_debug_update: NULL step"; return SIM3OPT_ERR_ARG; }
  if (!cam_qt && !points && !chi2 && !scale) { b->err = "ba_debug_update: every output is NULL"; return SIM3OPT_ERR_ARG; }
  if (!std::isfinite(lambda)) { b->err = "ba_debug_update: lambda is not finite"; return SIM3OPT_ERR_ARG; }
  return b->read_update(dx_c, dx_p, lambda, with_fail != 0, cam_qt, points, chi2, scale);
  });
}

// ---- covariances (include/sim3opt.h, "Bundle-adjustment covariances") ----
int sim3opt_ba_covariances(sim3opt_ba* b, double lambda, int32_t n_cc, const int32_t* cam_a, const int32_t* cam_b,
                           double* cov_cc, int32_t n_pp, const int32_t* point, double* cov_pp, int32_t n_pc,
                           const int32_t* pc_point, const int32_t* pc_cam, double* cov_pc) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_covariances", sim3opt::NO_MEMORY_OR_INTERNAL, [&]() -> int {
  b->err.clear();
  if (n_cc < 0 || n_pp < 0 || n_pc < 0 || (n_cc > 0 && (!cam_a || !cam_b || !cov_cc)) ||
      (n_pp > 0 && (!point || !cov_pp)) || (n_pc > 0 && (!pc_point || !pc_cam || !cov_pc))) {
    b->err = "ba_covariances: negative count or NULL array";
    return SIM3OPT_ERR_ARG;
  }
  if (!sim3opt::all_finite(&lambda, 1) || lambda < 0.0) {
    b->err = "ba_covariances: lambda must be finite and >= 0";
    return SIM3OPT_ERR_ARG;
  }
  if (b->no() < 1) { b->err = "ba_covariances: no problem set"; return SIM3OPT_ERR_STATE; }
  if (!b->ready) { int rc = b->initialize(); if (rc) return rc; }
  return b->covariances(lambda, n_cc, cam_a, cam_b, cov_cc, n_pp, point, cov_pp, n_pc, pc_point, pc_cam, cov_pc);
  });
}

int sim3opt_ba_covariance_plan(sim3opt_ba* b, int32_t* nb, int64_t* nL, int32_t* ngroups, int32_t* perm, int32_t* colptr,
                               int32_t* lrow) {
  if (!b) return SIM3OPT_ERR_ARG;
  return sim3opt::guarded(b, "ba_covariance_plan", sim3opt::NO_MEMORY_OR_INTERNAL, [&]() -> int {
  int rc = ba_debug_enter(b, "ba_covariance_plan");
  if (rc) return rc;
  if (!nb || !nL || !ngroups) { b->err = "ba_covariance_plan: NULL output"; return SIM3OPT_ERR_ARG; }
  if (!b->cov_factor.ready() && (rc = b->cov_init())) return rc;
  const sim3opt::DirectPlan& P = b->cov_factor.plan();
  *nb = P.nb;
  *nL = P.nL;
  *ngroups = P.ngroups();
  if (perm) std::memcpy(perm, P.perm.data(), sizeof(int32_t) * P.perm.size());
  if (colptr) std::memcpy(colptr, P.colptr.data(), sizeof(int32_t) * P.colptr.size());
  if (lrow) std::memcpy(lrow, P.lrow.data(), sizeof(int32_t) * P.lrow.size());
  return SIM3OPT_OK;
  });
}

int sim3opt_ba_covariance_stats(const sim3opt_ba* b, int64_t out[6]) {
  if (!b || !out) return SIM3OPT_ERR_ARG;
  for (int k = 0; k < 6; ++k) out[k] = b->cov_stats[k];
  return SIM3OPT_OK;
}

int sim3opt_ba_optimize(sim3opt_ba* b, int32_t max_iters) {
  if (!b) return 0;
  try {
  b->err.clear();
  if (max_iters < 1 || b->no() < 1) return -1;
  if (!b->ready) { int rc = b->initialize(); if (rc) return 0; }
  const int n = b->optimize(max_iters);
  return n < 0 ? 0 : n;
  } catch (...) {  // nothing crosses the C boundary
    b->err = "ba_optimize: out of host memory or internal error"; return 0;
  }
}

int sim3opt_ba_get_cameras(const sim3opt_ba* b, double* cam_qt) {
  if (!b || !cam_qt) return SIM3OPT_ERR_ARG;
  for (int c = 0; c < b->nc(); ++c) {
    for (int i = 0; i < 4; ++i) cam_qt[7 * (size_t)c + i] = b->cams[c].q[i];
    for (int i = 0; i < 3; ++i) cam_qt[7 * (size_t)c + 4 + i] = b->cams[c].t[i];
  }
  return SIM3OPT_OK;
}

int sim3opt_ba_get_points(const sim3opt_ba* b, double* points) {
  if (!b || !points) return SIM3OPT_ERR_ARG;
  std::memcpy(points, b->pts.data(), sizeof(double) * b->pts.size());
  return SIM3OPT_OK;
}

int32_t sim3opt_ba_num_iterations(const sim3opt_ba* b) { return b ? (int32_t)b->stats.size() : 0; }

int sim3opt_ba_get_stats(const sim3opt_ba* b, int32_t iter, sim3opt_iter_stats* out) {
  if (!b || !out || iter < 0 || iter >= (int32_t)b->stats.size()) return SIM3OPT_ERR_ARG;
  *out = b->stats[iter];
  return SIM3OPT_OK;
}

// "% SE3 optimization result: kf id, tcinw, rc2w(qxyzw)" rows (bal_example.cpp:223-238), 17 digits
int sim3opt_ba_write_poses(const sim3opt_ba* b, const char* path) {
  if (!b || !path) return SIM3OPT_ERR_ARG;
  FILE* f = std::fopen(path, "w");
  if (!f) return SIM3OPT_ERR_IO;
  std::fprintf(f, "%% SE3 optimization result: kf id, tcinw, rc2w(qxyzw):\n");
  for (int c = 0; c < b->nc(); ++c) {
    const double* q = b->cams[c].q;
    const double* t = b->cams[c].t;
    const double qc[4] = {-q[0], -q[1], -q[2], q[3]};
    // tcinw = -R^T t
    const double ux = 2 * (qc[1] * t[2] - qc[2] * t[1]), uy = 2 * (qc[2] * t[0] - qc[0] * t[2]),
                 uz = 2 * (qc[0] * t[1] - qc[1] * t[0]);
    const double r0 = t[0] + qc[3] * ux + (qc[1] * uz - qc[2] * uy);
    const double r1 = t[1] + qc[3] * uy + (qc[2] * ux - qc[0] * uz);
    const double r2 = t[2] + qc[3] * uz + (qc[0] * uy - qc[1] * ux);
    std::fprintf(f, "%d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", c, -r0, -r1, -r2, qc[0], qc[1], qc[2], qc[3]);
  }
  return std::fclose(f) == 0 ? SIM3OPT_OK : SIM3OPT_ERR_IO;
}

}  // extern "C"
