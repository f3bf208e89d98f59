// sim3_batch_math.hpp -- the arithmetic of the batched Sim(3) stage (sim3_batch.hip): Horn's closed form on three 3-D
// -- 3-D matches, the two reprojection errors of a match under C = (R, t, s), the terms of a Levenberg-Marquardt
// iteration on the seven parameters of C with its 7 x 7 Cholesky solve, and the update C <- exp(delta) C (the sampler:
// ransac_sample.hpp; exp: sim3_math.hpp).  Host and device: tests/cxx/sim3_batch_math_driver.cpp runs the same
// statements on the CPU against tests/sim3_batch_ref.py.
//
// PARITY UNPINNED: the reference has no such step (its loop edges carry a median depth ratio, a rigid two-view BA and
// the identity as information).  The method is Horn's closed form as ORB-SLAM's Sim3Solver / OptimizeSim3 use it; ours:
//   rotation      Horn's 4 x 4 symmetric eigenproblem by JACOBI_SWEEPS cyclic Jacobi sweeps (ORB-SLAM: cv::eigen); the
//                 eigenvector of the largest eigenvalue is the quaternion, so three points (a cross-covariance of rank
//                 two) need no special case and no determinant fix
//   scale         Horn's asymmetric form s = sum x1'.R x0' / sum |x0'|^2, as ORB-SLAM
//   camera plane  a match is staged as (x, y, depth) per frame with (x, y) = ((u, v) - c) / f, X = depth (x, y, 1), and
//                 a reprojection error is f ((X'/Z') - (x, y)): the pixel error up to rounding
//   exp           g2o's Sim(3) exp with the exact small-angle limit of B (sim3_math.hpp's fix_small_b = 1): as written
//                 (sim3_rv.h:166) that coefficient grows like 1 / sigma^3 and would wreck a small LM step
// Every loop has a constant bound; every index of a private array is a compile-time constant once unrolled, so
// nothing goes to scratch.
#pragma once
#include <cmath>
#include <cstdint>

#include "ransac_sample.hpp"
#include "sim3_math.hpp"

#define SIM3OPT_S3B_HD SIM3OPT_RANSAC_HD

// No fused multiply-add anywhere in this stage, as in its siblings: the device rounds every operation as the host
// build of these statements does (tests/test_gpu_sim3_batch.py compares bit for bit).
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sim3opt_sim3b {

constexpr int JACOBI_SWEEPS = 10;  // cyclic sweeps on Horn's 4 x 4 matrix (Jacobi's method converges quadratically)
constexpr int S3B_ACC = 36;        // what an LM iteration sums: 28 of J^T W J (upper), 7 of -J^T W r, chi2
constexpr double EXP_EPS = 1e-5;   // sim3_math.hpp's branch threshold, the library's default

SIM3OPT_S3B_HD constexpr int tri7(int r, int c) { return r * 7 - r * (r - 1) / 2 + (c - r); }

// a match as the kernel holds it: p = (x0, y0, depth0, x1, y1, depth1), camera-plane coordinates
SIM3OPT_S3B_HD void s3b_match(double u0, double v0, double d0, double u1, double v1, double d1, double f, double cx,
                              double cy, double p[6]) {
  p[0] = (u0 - cx) / f; p[1] = (v0 - cy) / f; p[2] = d0;
  p[3] = (u1 - cx) / f; p[4] = (v1 - cy) / f; p[5] = d1;
}

SIM3OPT_S3B_HD void s3b_points(const double p[6], double X0[3], double X1[3]) {
  X0[0] = p[2] * p[0]; X0[1] = p[2] * p[1]; X0[2] = p[2];
  X1[0] = p[5] * p[3]; X1[1] = p[5] * p[4]; X1[2] = p[5];
}

// whether the triangle P[0] P[1] P[2] is one: sin^2 of its angle at P[0] above min_sin2 (false for NaN, for repeated
// and for collinear points)
SIM3OPT_S3B_HD bool s3b_triangle(const double P[3][3], double min_sin2) {
  const double a[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
  const double b[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
  const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  return cc > min_sin2 * (aa * bb);
}

// The eigenvector of the largest eigenvalue of the symmetric N (4 x 4) by cyclic Jacobi sweeps: v, not normalised
// beyond what the rotations keep.
SIM3OPT_S3B_HD void s3b_max_eigenvector(double N[4][4], double v[4]) {
  double V[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = N[p][q];
        if (apq != 0.0) {
          const double theta = (N[q][q] - N[p][p]) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double a = N[k][p], b = N[k][q];
            N[k][p] = c * a - s * b; N[k][q] = s * a + c * b;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double a = N[p][k], b = N[q][k];
            N[p][k] = c * a - s * b; N[q][k] = s * a + c * b;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double a = V[k][p], b = V[k][q];
            V[k][p] = c * a - s * b; V[k][q] = s * a + c * b;
          }
        }
      }
  }
  double lam = N[0][0];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = V[k][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const bool take = N[j][j] > lam;
    lam = take ? N[j][j] : lam;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = take ? V[k][j] : v[k];
  }
}

struct S3bPrep {  // what scoring and linearisation need of C: X1 ~ A X0 + t, X0 ~ Ai X1 + ti
  double A[9], t[3], Ai[9], ti[3];
};

SIM3OPT_S3B_HD void s3b_prepare(const double m[8], S3bPrep& P) {
  double R[9];
  const double q[4] = {m[0], m[1], m[2], m[3]};
  sim3::R_from_quat(q, R);
  const double s = m[7], is = 1.0 / s;
#pragma unroll
  for (int i = 0; i < 9; ++i) P.A[i] = s * R[i];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) P.Ai[3 * r + c] = is * R[3 * c + r];
#pragma unroll
  for (int i = 0; i < 3; ++i) P.t[i] = m[4 + i];
#pragma unroll
  for (int r = 0; r < 3; ++r) P.ti[r] = -((P.Ai[3 * r] * m[4] + P.Ai[3 * r + 1] * m[5]) + P.Ai[3 * r + 2] * m[6]);
}

SIM3OPT_S3B_HD void s3b_apply(const double M[9], const double t[3], const double X[3], double Y[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) Y[r] = ((M[3 * r] * X[0] + M[3 * r + 1] * X[1]) + M[3 * r + 2] * X[2]) + t[r];
}

// The residuals of match p: r[0..1] = pi(C X0) - uv1, r[2..3] = pi(C^-1 X1) - uv0 (pixels), with Y = C X0 and
// Z = C^-1 X1.  True when both lie in front of their camera.
SIM3OPT_S3B_HD bool s3b_residuals(const S3bPrep& P, const double p[6], double f, double r[4], double Y[3],
                                  double Z[3]) {
  double X0[3], X1[3];
  s3b_points(p, X0, X1);
  s3b_apply(P.A, P.t, X0, Y);
  s3b_apply(P.Ai, P.ti, X1, Z);
  r[0] = f * (Y[0] / Y[2] - p[3]); r[1] = f * (Y[1] / Y[2] - p[4]);
  r[2] = f * (Z[0] / Z[2] - p[0]); r[3] = f * (Z[1] / Z[2] - p[1]);
  return Y[2] > 0.0 && Z[2] > 0.0;
}

// the scoring rule: inlier iff both depths are positive and both squared errors are at most max2; e2 = e0 + e1
SIM3OPT_S3B_HD bool s3b_inlier(const S3bPrep& P, const double p[6], double f, double max2, double& e2) {
  double r[4], Y[3], Z[3];
  const bool front = s3b_residuals(P, p, f, r, Y, Z);
  const double e1 = r[0] * r[0] + r[1] * r[1], e0 = r[2] * r[2] + r[3] * r[3];
  e2 = e0 + e1;
  return front && e1 <= max2 && e0 <= max2;
}

// Horn's closed form on the three matches s[0..2]: model = [qx qy qz qw tx ty tz s] with X1 ~ s R X0 + t.  False (and
// the identity) when a triangle is degenerate in either frame, when s is not finite and positive, or when a sample
// point has a non-positive depth after the transform in either direction.
SIM3OPT_S3B_HD bool s3b_horn(const double s[3][6], double min_sin2, double model[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) model[i] = (i == 3 || i == 7) ? 1.0 : 0.0;
  double A[3][3], B[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) s3b_points(s[i], A[i], B[i]);
  if (!s3b_triangle(A, min_sin2) || !s3b_triangle(B, min_sin2)) return false;
  double ca[3], cb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ca[c] = ((A[0][c] + A[1][c]) + A[2][c]) / 3.0;
    cb[c] = ((B[0][c] + B[1][c]) + B[2][c]) / 3.0;
  }
  double S[3][3], a[3][3], b[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[i][c] = A[i][c] - ca[c]; b[i][c] = B[i][c] - cb[c]; }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) S[r][c] = (a[0][r] * b[0][c] + a[1][r] * b[1][c]) + a[2][r] * b[2][c];
  double N[4][4];  // Horn (1987), eq. for N; quaternion order (w, x, y, z)
  N[0][0] = (S[0][0] + S[1][1]) + S[2][2];
  N[0][1] = S[1][2] - S[2][1]; N[0][2] = S[2][0] - S[0][2]; N[0][3] = S[0][1] - S[1][0];
  N[1][1] = (S[0][0] - S[1][1]) - S[2][2];
  N[1][2] = S[0][1] + S[1][0]; N[1][3] = S[2][0] + S[0][2];
  N[2][2] = (S[1][1] - S[0][0]) - S[2][2];
  N[2][3] = S[1][2] + S[2][1];
  N[3][3] = (S[2][2] - S[0][0]) - S[1][1];
#pragma unroll
  for (int r = 1; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < r; ++c) N[r][c] = N[c][r];
  double v[4];
  s3b_max_eigenvector(N, v);
  const double nv = sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
  if (!(nv > 0.0) || !std::isfinite(nv)) return false;
  const double sg = v[0] < 0.0 ? -1.0 : 1.0;  // qw >= 0
  const double q[4] = {sg * v[1] / nv, sg * v[2] / nv, sg * v[3] / nv, sg * v[0] / nv};
  double R[9];
  sim3::R_from_quat(q, R);
  const double zero[3] = {0.0, 0.0, 0.0};
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double Ra[3];
    s3b_apply(R, zero, a[i], Ra);
    num += (b[i][0] * Ra[0] + b[i][1] * Ra[1]) + b[i][2] * Ra[2];
    den += (a[i][0] * a[i][0] + a[i][1] * a[i][1]) + a[i][2] * a[i][2];
  }
  const double sc = num / den;
  if (!(sc > 0.0) || !std::isfinite(sc)) return false;
  double Rc[3];
  s3b_apply(R, zero, ca, Rc);
  double m[8] = {q[0], q[1], q[2], q[3], cb[0] - sc * Rc[0], cb[1] - sc * Rc[1], cb[2] - sc * Rc[2], sc};
  S3bPrep P;
  s3b_prepare(m, P);
  bool front = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double Y[3], Z[3];
    s3b_apply(P.A, P.t, A[i], Y);
    s3b_apply(P.Ai, P.ti, B[i], Z);
    front = front && Y[2] > 0.0 && Z[2] > 0.0;
  }
  if (!front) return false;
#pragma unroll
  for (int i = 0; i < 8; ++i) model[i] = m[i];
  return true;
}

// Huber of width delta on a 2-vector of squared length e2 (g2o's RobustKernelHuber): rho and the weight rho'.
// delta <= 0: no robust kernel.
SIM3OPT_S3B_HD void s3b_huber(double e2, double delta, double& rho, double& w) {
  rho = e2; w = 1.0;
  if (delta > 0.0) {
    const double e = sqrt(e2);
    if (e > delta) { rho = 2.0 * e * delta - delta * delta; w = delta / e; }
  }
}

// The two 2 x 7 Jacobians of match p with respect to delta in C <- exp(delta) C, delta = [omega, upsilon, sigma]:
// exp(delta) Y = Y + omega x Y + upsilon + sigma Y and (exp(delta) C)^-1 X1 = Z - Ai (omega x X1 + upsilon + sigma X1)
// to first order.  J[0..1] the rows of r[0..1], J[2..3] those of r[2..3].
SIM3OPT_S3B_HD void s3b_jacobians(const S3bPrep& P, const double p[6], double f, const double Y[3], const double Z[3],
                                  double J[4][7]) {
  double X0[3], X1[3];
  s3b_points(p, X0, X1);
  // d pi / d Y, and d pi / d Z times Ai
  const double iy = 1.0 / Y[2], iz = 1.0 / Z[2];
  const double P1[2][3] = {{f * iy, 0.0, -(f * iy) * (Y[0] * iy)}, {0.0, f * iy, -(f * iy) * (Y[1] * iy)}};
  const double P0[2][3] = {{f * iz, 0.0, -(f * iz) * (Z[0] * iz)}, {0.0, f * iz, -(f * iz) * (Z[1] * iz)}};
  double G[2][3];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      G[r][c] = (P0[r][0] * P.Ai[c] + P0[r][1] * P.Ai[3 + c]) + P0[r][2] * P.Ai[6 + c];
  // D1 = [-[Y]x, I, Y], D0 = [[X1]x, -I, -X1] (3 x 7)
  const double D1[3][7] = {{0.0, Y[2], -Y[1], 1.0, 0.0, 0.0, Y[0]},
                           {-Y[2], 0.0, Y[0], 0.0, 1.0, 0.0, Y[1]},
                           {Y[1], -Y[0], 0.0, 0.0, 0.0, 1.0, Y[2]}};
  const double D0[3][7] = {{0.0, -X1[2], X1[1], -1.0, 0.0, 0.0, -X1[0]},
                           {X1[2], 0.0, -X1[0], 0.0, -1.0, 0.0, -X1[1]},
                           {-X1[1], X1[0], 0.0, 0.0, 0.0, -1.0, -X1[2]}};
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      J[r][k] = (P1[r][0] * D1[0][k] + P1[r][1] * D1[1][k]) + P1[r][2] * D1[2][k];
      J[2 + r][k] = (G[r][0] * D0[0][k] + G[r][1] * D0[1][k]) + G[r][2] * D0[2][k];
    }
}

// A match's terms of an LM iteration into acc (S3B_ACC): J^T W J (upper, tri7), -J^T W r, rho.  w[0] is the Huber
// weight of the residual in image 1, w[1] that in image 0.
SIM3OPT_S3B_HD void s3b_accumulate(const S3bPrep& P, const double p[6], double f, double delta, double acc[S3B_ACC],
                                   double w[2]) {
  double r[4], Y[3], Z[3], J[4][7];
  s3b_residuals(P, p, f, r, Y, Z);
  s3b_jacobians(P, p, f, Y, Z, J);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double rho;
    s3b_huber(r[2 * h] * r[2 * h] + r[2 * h + 1] * r[2 * h + 1], delta, rho, w[h]);
#pragma unroll
    for (int a = 0; a < 7; ++a) {
#pragma unroll
      for (int c = a; c < 7; ++c)
        acc[tri7(a, c)] += w[h] * (J[2 * h][a] * J[2 * h][c] + J[2 * h + 1][a] * J[2 * h + 1][c]);
      acc[28 + a] -= w[h] * (J[2 * h][a] * r[2 * h] + J[2 * h + 1][a] * r[2 * h + 1]);
    }
    acc[35] += rho;
  }
}

// a match's share of chi2: the two Huber costs
SIM3OPT_S3B_HD double s3b_chi2(const S3bPrep& P, const double p[6], double f, double delta) {
  double r[4], Y[3], Z[3], rho0, rho1, w;
  s3b_residuals(P, p, f, r, Y, Z);
  s3b_huber(r[0] * r[0] + r[1] * r[1], delta, rho1, w);
  s3b_huber(r[2] * r[2] + r[3] * r[3], delta, rho0, w);
  return rho1 + rho0;
}

// S x = g by Cholesky (S symmetric 7 x 7, upper triangle given by tri7); false on a non-positive pivot
SIM3OPT_S3B_HD bool s3b_chol7_solve(const double Su[28], const double g[7], double x[7]) {
  double L[7][7];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    double d = Su[tri7(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) ok = false;
    const double l = sqrt(d);
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 7; ++i) {
      double s = Su[tri7(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / l;
    }
  }
  double y[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    double s = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 6; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 7; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  return ok;
}

// C <- exp(dx) C, the quaternion normalised
SIM3OPT_S3B_HD void s3b_oplus(const double dx[7], double m[8]) {
  const sim3::Opts o{EXP_EPS, 0, 1};
  const sim3::Sim3 E = sim3::exp(dx, o);
  sim3::Sim3 C;
#pragma unroll
  for (int i = 0; i < 4; ++i) C.q[i] = m[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) C.t[i] = m[4 + i];
  C.s = m[7];
  const sim3::Sim3 N = sim3::mul(E, C);
  const double nq = sqrt(((N.q[0] * N.q[0] + N.q[1] * N.q[1]) + N.q[2] * N.q[2]) + N.q[3] * N.q[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = N.q[i] / nq;
#pragma unroll
  for (int i = 0; i < 3; ++i) m[4 + i] = N.t[i];
  m[7] = N.s;
}

// Omega (49, column-major; it is symmetric) from the sums of an iteration, divided by pixel_noise^2
SIM3OPT_S3B_HD void s3b_information(const double acc[S3B_ACC], double pixel_noise, double info[49]) {
  const double k = 1.0 / (pixel_noise * pixel_noise);
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int c = r; c < 7; ++c) {
      const double v = acc[tri7(r, c)] * k;
      info[7 * c + r] = v;
      info[7 * r + c] = v;
    }
}

}  // namespace sim3opt_sim3b
