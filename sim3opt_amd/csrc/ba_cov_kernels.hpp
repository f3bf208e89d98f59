// ba_cov_kernels.hpp -- device side of sim3opt_ba_covariances (included by ba.hip inside namespace sim3opt_bundle, after
// its kernels; the specification is in include/sim3opt.h, the host side in ba_cov_host.hpp).
//
// After k_ba_obs / k_ba_points / k_ba_obs2 / k_ba_reduced have left H_pp^-1, Z = (A^T B) H_pp^-1 and the reduced camera
// system S for the caller's lambda:
//   k_ba_cov_point_pivots  thread / point: the 3x3 LDL^T of H_pp + lambda I in x, y, z order; the lowest point with a pivot
//                          <= 1e-13 pdmax (or <= 0) is reported through an integer maximum (no floating-point atomics)
//   k_ba_cov_pads          thread / camera: the unit pad of the 7x7 storage and a fixed camera's identity row take the
//                          value max(1, max |H_dd|), so that the selected inversion's 1e-13 max |H_dd| pivot test
//                          sees them as well scaled as the rest; the 6x6 parts are untouched (the pads couple to nothing)
//   (BlockLdl: gather, factor, selinv, pick)
//   k_ba_cov_cams          thread / entry: a picked 7x7 block of S^-1 -> 6x6, exactly +0 where a fixed camera masks it
//   k_ba_cov_points        wavefront / requested point: the n^2 ordered observation pairs are dealt to the lanes (pair e =
//                          a n + b to lane e mod 64, ascending), each lane keeps a private 3x3 sum of Z_a^T Sigma_cc Z_b,
//                          a butterfly adds the lanes in a fixed order, then H_pp^-1 is added and the block symmetrised
//   k_ba_cov_cross         thread / entry of a 3x6 block: -sum over the point's observations, list order
// Every block depends on the problem and lambda alone, never on where it stands in the request.
#pragma once

constexpr double BA_COV_PIVOT_REL = 1e-13;

// flags: [0] the factorisation's fail word, [1] the selected inversion's singular flag, [2] np - p of the lowest point
// that fails the pivot test (0: none)
__global__ __launch_bounds__(WG) void k_ba_cov_point_pivots(int np, const int32_t* __restrict__ pptr,
                                                            const int32_t* __restrict__ pobs,
                                                            const double* __restrict__ lin, double lambda,
                                                            const double* __restrict__ pdmax, int32_t* flags) {
  const int p = blockIdx.x * WG + threadIdx.x;
  if (p >= np) return;
  double H[6] = {0, 0, 0, 0, 0, 0};  // xx xy xz yy yz zz, summed as k_ba_points sums them
  for (int k = pptr[p]; k < pptr[p + 1]; ++k) {
    const double* B = lin + (size_t)20 * pobs[k] + 12;
    H[0] += B[0] * B[0] + B[3] * B[3];
    H[1] += B[0] * B[1] + B[3] * B[4];
    H[2] += B[0] * B[2] + B[3] * B[5];
    H[3] += B[1] * B[1] + B[4] * B[4];
    H[4] += B[1] * B[2] + B[4] * B[5];
    H[5] += B[2] * B[2] + B[5] * B[5];
  }
  const double thr = BA_COV_PIVOT_REL * pdmax[p];
  const double d0 = H[0] + lambda;
  bool ok = d0 > thr && d0 > 0.0;
  const double l10 = H[1] / d0, l20 = H[2] / d0;
  const double d1 = H[3] + lambda - l10 * H[1];
  ok = ok && d1 > thr && d1 > 0.0;
  const double l21 = (H[4] - l20 * H[1]) / d1;
  const double d2 = H[5] + lambda - l20 * H[2] - l21 * l21 * d1;
  ok = ok && d2 > thr && d2 > 0.0;
  if (!ok) atomicMax(&flags[2], np - p);
}

__global__ __launch_bounds__(WG) void k_ba_cov_pads(int nc, const int32_t* __restrict__ rptr,
                                                    const uint8_t* __restrict__ fixed, const Scal* sc,
                                                    double* __restrict__ S) {
  const int i = blockIdx.x * WG + threadIdx.x;
  if (i >= nc) return;
  const double v = sc->maxdiag > 1.0 ? sc->maxdiag : 1.0;
  double* blk = S + (size_t)49 * rptr[i];  // the diagonal block comes first in its row
  if (fixed[i]) {
#pragma unroll
    for (int d = 0; d < 7; ++d) blk[8 * d] = v;
  } else {
    blk[48] = v;
  }
}

// out[q] (6x6 column-major) = the 6x6 part of in[q] (7x7 column-major), +0 where mask[q]
__global__ __launch_bounds__(WG) void k_ba_cov_cams(int n, const double* __restrict__ in,
                                                    const int32_t* __restrict__ mask, double* __restrict__ out) {
  const int t = blockIdx.x * WG + threadIdx.x;
  if (t >= 36 * n) return;
  const int q = t / 36, e = t % 36, r = e % 6, c = e / 6;
  out[t] = mask[q] ? 0.0 : in[(size_t)49 * q + r + 7 * c];
}

// block of S that holds (camera ca, camera cb), or -1 (cannot happen for two observers of one point)
__device__ __forceinline__ int ba_cov_block(const int32_t* __restrict__ rptr, const int32_t* __restrict__ bcol, int ca,
                                            int cb) {
  int lo = rptr[ca];
  if (ca == cb) return lo;
  int hi = rptr[ca + 1];
  const int end = hi;
  ++lo;  // the off-diagonal blocks of a row: columns ascending
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (bcol[mid] < cb) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && bcol[lo] == cb ? lo : -1;
}

struct CovPointArgs {
  int32_t n;              // requested points
  const int32_t* upoint;  // their indices
  const int32_t* pptr;
  const int32_t* pobs;
  const int32_t* oc;
  const uint8_t* fixed;
  const int32_t* rptr;
  const int32_t* bcol;
  const double* Z;     // n_obs x 18 (6x3 row-major)
  const double* Hinv;  // n_points x 9
  const double* C;     // blocks of S^-1 in S's block order, 6x6 column-major, masked
  double* out;         // n x 9
};

__global__ __launch_bounds__(WG) void k_ba_cov_points(CovPointArgs A) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= A.n) return;
  const int p = A.upoint[w];
  const int k0 = A.pptr[p], n = A.pptr[p + 1] - k0;
  const long long nn = (long long)n * n;
  double acc[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) acc[q] = 0.0;
  for (long long e = lane; e < nn; e += 64) {
    const int a = (int)(e / n), b = (int)(e % n);
    const int oa = A.pobs[k0 + a], ob = A.pobs[k0 + b];
    const int ca = A.oc[oa], cb = A.oc[ob];
    if (A.fixed[ca] | A.fixed[cb]) continue;  // contributes nothing
    const int k = ba_cov_block(A.rptr, A.bcol, ca, cb);
    if (k < 0) continue;
    const double* cp = A.C + (size_t)36 * k;
    const double* zap = A.Z + (size_t)18 * oa;
    const double* zbp = A.Z + (size_t)18 * ob;
    double cc[36], za[18], zb[18];
#pragma unroll
    for (int q = 0; q < 36; ++q) cc[q] = cp[q];
#pragma unroll
    for (int q = 0; q < 18; ++q) { za[q] = zap[q]; zb[q] = zbp[q]; }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double t6[6];  // column j of Sigma_cc Z_b
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += cc[r + 6 * c] * zb[3 * c + j];
        t6[r] = s;
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) s += za[3 * r + i] * t6[r];
        acc[3 * i + j] += s;
      }
    }
  }
  // butterfly sums (every lane ends with the total); lane 3 i + j takes entries (i, j) and (j, i)
  const int i = lane < 9 ? lane / 3 : 0, j = lane < 9 ? lane % 3 : 0;
  double mij = 0.0, mji = 0.0;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    double v = acc[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    mij = q == 3 * i + j ? v : mij;
    mji = q == 3 * j + i ? v : mji;
  }
  if (lane < 9) {
    const double* Hi = A.Hinv + (size_t)9 * p;
    const double x = Hi[3 * i + j] + mij, y = Hi[3 * j + i] + mji;
    A.out[(size_t)9 * w + lane] = 0.5 * (x + y);
  }
}

// out[u] (3x6 column-major, entry (i, c) at i + 3 c) = -sum_t Z_{xobs[t]}^T X[xpick[t]], t = xptr[u] .. xptr[u + 1)
__global__ __launch_bounds__(WG) void k_ba_cov_cross(int n, const int32_t* __restrict__ xptr,
                                                     const int32_t* __restrict__ xobs,
                                                     const int32_t* __restrict__ xpick, const double* __restrict__ Z,
                                                     const double* __restrict__ X, double* __restrict__ out) {
  const int t = blockIdx.x * WG + threadIdx.x;
  if (t >= 18 * n) return;
  const int u = t / 18, e = t % 18, i = e % 3, c = e / 3;
  double acc = 0.0;
  for (int k = xptr[u]; k < xptr[u + 1]; ++k) {
    if (xpick[k] < 0) continue;
    const double* z = Z + (size_t)18 * xobs[k];
    const double* x = X + (size_t)36 * xpick[k] + 6 * c;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += z[3 * r + i] * x[r];
    acc -= s;
  }
  out[t] = acc;
}
