// ba_math.hpp -- the camera / point arithmetic of the bundle-adjustment kernels, device only: the restatement
// of g2o's VertexSE3Expmap, EdgeProjectXYZ2UV and RobustKernelHuber that ba.hip (one large problem, a launch per
// step) and ba_batch.hip (many two-view problems, one launch) share.
#pragma once
#include <hip/hip_runtime.h>

namespace sim3opt_bundle {

__device__ __forceinline__ void quat_to_R(const double q[4], double R[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// Eigen's Quaternion(Matrix3) (trace branch, else the largest diagonal entry)
__device__ __forceinline__ void R_to_quat(const double R[9], double q[4]) {
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0) {
    double k = sqrt(tr + 1.0);
    q[3] = 0.5 * k; k = 0.5 / k;
    q[0] = (R[7] - R[5]) * k; q[1] = (R[2] - R[6]) * k; q[2] = (R[3] - R[1]) * k;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, l = (j + 1) % 3;
    double k = sqrt(R[4 * i] - R[4 * j] - R[4 * l] + 1.0);
    q[i] = 0.5 * k; k = 0.5 / k;
    q[3] = (R[3 * l + j] - R[3 * j + l]) * k;
    q[j] = (R[3 * j + i] + R[3 * i + j]) * k;
    q[l] = (R[3 * l + i] + R[3 * i + l]) * k;
  }
}

// EdgeProjectXYZ2UV::computeError: e = uv - K (R p + t); R of the camera's quaternion, X = camera-frame point
__device__ __forceinline__ void ba_project_residual(const double q[4], const double t[3], const double* p, double u,
                                                    double v, double f, double cx, double cy, double R[9],
                                                    double X[3], double e[2]) {
  quat_to_R(q, R);
#pragma unroll
  for (int i = 0; i < 3; ++i) X[i] = R[3 * i] * p[0] + R[3 * i + 1] * p[1] + R[3 * i + 2] * p[2] + t[i];
  e[0] = u - (f * X[0] / X[2] + cx);
  e[1] = v - (f * X[1] / X[2] + cy);
}

// g2o RobustKernelHuber on e2 = e^T Omega e
__device__ __forceinline__ void ba_huber(double e2, double delta, double& rho, double& w) {
  if (delta <= 0.0 || e2 <= delta * delta) {
    rho = e2;
    w = 1.0;
  } else {
    const double sq = sqrt(e2);
    rho = 2 * sq * delta - delta * delta;
    w = delta / sq;
  }
}

// EdgeProjectXYZ2UV::linearizeOplus (analytic): Jc = J_cam over [omega, upsilon] (2x6 row-major),
// Jp = J_point = -1/z [[f, 0, -f x/z], [0, f, -f y/z]] R (2x3 row-major)
__device__ __forceinline__ void ba_jacobians(const double R[9], const double X[3], double f, double Jc[12],
                                             double Jp[6]) {
  const double x = X[0], y = X[1], z = X[2], z2 = z * z;
  Jc[0] = x * y / z2 * f; Jc[1] = -(1 + x * x / z2) * f; Jc[2] = y / z * f;
  Jc[3] = -1.0 / z * f; Jc[4] = 0.0; Jc[5] = x / z2 * f;
  Jc[6] = (1 + y * y / z2) * f; Jc[7] = -x * y / z2 * f; Jc[8] = -x / z * f;
  Jc[9] = 0.0; Jc[10] = -1.0 / z * f; Jc[11] = y / z2 * f;
  const double t0[3] = {f, 0.0, -x / z * f}, t1[3] = {0.0, f, -y / z * f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    Jp[c] = -(t0[0] * R[c] + t0[1] * R[3 + c] + t0[2] * R[6 + c]) / z;
    Jp[3 + c] = -(t1[0] * R[c] + t1[1] * R[3 + c] + t1[2] * R[6 + c]) / z;
  }
}

// VertexSE3Expmap::oplusImpl: T <- SE3Quat::exp([omega, upsilon]) T on (q, t), the quaternion normalised after
__device__ __forceinline__ void ba_se3_oplus(const double* u, double cq[4], double ct[3]) {
  const double th = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  const double Om[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
  double Om2[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Om2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
  double R[9], V[9];
  if (th < 1e-5) {  // se3quat.h: R = I + Omega + Omega^2, V = R
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Om[i] + Om2[i];
    R[0] += 1; R[4] += 1; R[8] += 1;
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = R[i];
  } else {
    const double a = sin(th) / th, b = (1 - cos(th)) / (th * th), c = (th - sin(th)) / (th * th * th);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      R[i] = a * Om[i] + b * Om2[i];
      V[i] = b * Om[i] + c * Om2[i];
    }
    R[0] += 1; R[4] += 1; R[8] += 1;
    V[0] += 1; V[4] += 1; V[8] += 1;
  }
  double Rc[9], Rn[9];
  quat_to_R(cq, Rc);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = R[3 * i] * Rc[j] + R[3 * i + 1] * Rc[3 + j] + R[3 * i + 2] * Rc[6 + j];
  double tn[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    tn[i] = R[3 * i] * ct[0] + R[3 * i + 1] * ct[1] + R[3 * i + 2] * ct[2] +
            V[3 * i] * u[3] + V[3 * i + 1] * u[4] + V[3 * i + 2] * u[5];
  double q[4];
  R_to_quat(Rn, q);
  const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) cq[i] = q[i] / nq;
#pragma unroll
  for (int i = 0; i < 3; ++i) ct[i] = tn[i];
}

// inverse of the symmetric 3x3 [[a, b, c], [b, d, e], [c, e, f]] by cofactors, row-major 3x3
__device__ __forceinline__ void ba_sym3_inverse(double a, double bb, double c, double dd, double ee, double ff,
                                                double Hi[9]) {
  const double c00 = dd * ff - ee * ee, c01 = c * ee - bb * ff, c02 = bb * ee - c * dd;
  const double det = a * c00 + bb * c01 + c * c02;
  const double id = 1.0 / det;
  Hi[0] = c00 * id; Hi[1] = c01 * id; Hi[2] = c02 * id;
  Hi[3] = c01 * id; Hi[4] = (a * ff - c * c) * id; Hi[5] = (bb * c - a * ee) * id;
  Hi[6] = c02 * id; Hi[7] = (bb * c - a * ee) * id; Hi[8] = (a * dd - bb * bb) * id;
}

// ---- what a workgroup of 256 threads (four wavefronts) that owns one small problem shares: ba_batch.hip and
// pnp_batch.hip sum over their points with wg_sum and solve their 6x6 camera system with chol6_solve ----

// Sum of v[q] over the workgroup, left in v[q] of every thread with the same bits: xor butterfly over the
// wavefront (a + b and b + a are the same double), then the wavefronts' partials in the order 0, 1, 2, 3.
template <int N>
__device__ __forceinline__ void wg_sum(double (&v)[N], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    double x = v[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    v[q] = x;
  }
  __syncthreads();  // the readers of the previous sum are done with red
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) red[wave * N + q] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = ((red[q] + red[N + q]) + red[2 * N + q]) + red[3 * N + q];
}

__device__ __forceinline__ double wg_max(double x, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off));
  __syncthreads();
  if (lane == 0) red[wave] = x;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// upper triangle of a symmetric 6x6, row by row
__device__ __forceinline__ constexpr int tri6(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }

// S dx = g by Cholesky (S symmetric, upper triangle given); false on a non-positive pivot
__device__ __forceinline__ bool chol6_solve(const double Su[21], const double g[6], double x[6]) {
  double L[6][6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = Su[tri6(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) ok = false;
    const double l = sqrt(d);
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = Su[tri6(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / l;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  return ok;
}

}  // namespace sim3opt_bundle
