// pnp_math.hpp -- the per-hypothesis arithmetic of the batched PnP RANSAC (pnp_batch.hip): a closed-form quartic, the
// three-point pose (P3P) and the squared reprojection error (the sampler: ransac_sample.hpp).  Host and device:
// tests/cxx/pnp_math_driver.cpp runs the same statements on the CPU against tests/pnp_ref.py.
//
// P3P, the formulation: with unit bearings j1 j2 j3 of the three pixels, depths s1, s2 = u s1, s3 = v s1 and the
// side lengths a = |X2 - X3|, b = |X1 - X3|, c = |X1 - X2|, the law of cosines gives
//     s1^2 (1 + u^2 - 2 u cos(g)) = c^2,   s1^2 (1 + v^2 - 2 v cos(b)) = b^2,   s1^2 (u^2 + v^2 - 2 u v cos(a)) = a^2.
// The difference of the last and the first, each over the second, is linear in u: u = N(v) / D(v), N quadratic, D
// linear.  Put into the first over the second it leaves a quartic in v (Grunert's elimination), whose coefficients
// are built here by polynomial products rather than copied from a table.  Its real roots come from Ferrari's
// factorisation (resolvent cubic by Cardano / the trigonometric form) and a FIXED number of Newton steps on the
// quartic itself; nothing iterates "until converged".  Each root with positive depths gives the three points in the
// camera's frame; the pose is the rotation between the two orthonormal frames spanned by the triangles.
#pragma once
#include <cmath>
#include <cstdint>

#include "ransac_sample.hpp"

#define SIM3OPT_PNP_HD SIM3OPT_RANSAC_HD

namespace sim3opt_pnp {

constexpr int QUARTIC_POLISH = 3;  // Newton steps on every root of the quartic
constexpr int CUBIC_POLISH = 2;    // ... and on the resolvent cubic's root

// largest real root of m^3 + B m^2 + C m + D
SIM3OPT_PNP_HD double cubic_largest_root(double B, double C, double D) {
  const double P = C - B * B / 3.0, Q = 2.0 * B * B * B / 27.0 - B * C / 3.0 + D;
  const double disc = 0.25 * Q * Q + P * P * P / 27.0;
  double z;
  if (disc > 0.0) {
    const double sd = sqrt(disc);
    z = cbrt(-0.5 * Q + sd) + cbrt(-0.5 * Q - sd);
  } else if (P < 0.0) {
    const double k = sqrt(-P / 3.0);
    double c = 3.0 * Q / (2.0 * P * k);
    c = fmin(1.0, fmax(-1.0, c));
    z = 2.0 * k * cos(acos(c) / 3.0);
  } else {
    z = 0.0;
  }
  double m = z - B / 3.0;
#pragma unroll
  for (int it = 0; it < CUBIC_POLISH; ++it) {
    const double fv = ((m + B) * m + C) * m + D, dv = (3.0 * m + 2.0 * B) * m + C;
    const double step = fv / dv;
    if (dv != 0.0 && std::isfinite(step)) m -= step;
  }
  return m;
}

// real roots of c[4] x^4 + c[3] x^3 + c[2] x^2 + c[1] x + c[0]; returns how many (0..4)
SIM3OPT_PNP_HD int quartic_real_roots(const double c[5], double x[4]) {
  x[0] = x[1] = x[2] = x[3] = 0.0;
  if (!(fabs(c[4]) > 0.0)) return 0;
  const double a = c[3] / c[4], b = c[2] / c[4], cc = c[1] / c[4], d = c[0] / c[4];
  const double a2 = a * a;
  const double p = b - 0.375 * a2;
  const double q = cc - 0.5 * a * b + 0.125 * a2 * a;
  const double r = d - 0.25 * a * cc + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2;
  // y^4 + p y^2 + q y + r = (y^2 + s y + al)(y^2 - s y + be), s^2 = 2 m, m a root of the resolvent cubic
  const double m = cubic_largest_root(p, 0.25 * p * p - r, -0.125 * q * q);
  int n = 0;
  if (m > 0.0) {
    const double s = sqrt(2.0 * m), hh = 0.5 * p + m, g = q / (2.0 * s);
    const double d1 = 2.0 * m - 4.0 * (hh - g), d2 = 2.0 * m - 4.0 * (hh + g);
    if (d1 >= 0.0) {
      const double sq = sqrt(d1);
      x[n++] = 0.5 * (-s + sq);
      x[n++] = 0.5 * (-s - sq);
    }
    if (d2 >= 0.0) {
      const double sq = sqrt(d2);
      x[n++] = 0.5 * (s + sq);
      x[n++] = 0.5 * (s - sq);
    }
  } else {  // q = 0: a quadratic in y^2
    const double dd = p * p - 4.0 * r;
    if (dd >= 0.0) {
      const double sq = sqrt(dd);
      const double z0 = 0.5 * (-p + sq), z1 = 0.5 * (-p - sq);
      if (z0 >= 0.0) { x[n++] = sqrt(z0); x[n++] = -sqrt(z0); }
      if (z1 >= 0.0) { x[n++] = sqrt(z1); x[n++] = -sqrt(z1); }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double v = x[k] - 0.25 * a;
#pragma unroll
    for (int it = 0; it < QUARTIC_POLISH; ++it) {
      const double fv = (((c[4] * v + c[3]) * v + c[2]) * v + c[1]) * v + c[0];
      const double dv = ((4.0 * c[4] * v + 3.0 * c[3]) * v + 2.0 * c[2]) * v + c[1];
      const double step = fv / dv;
      if (dv != 0.0 && std::isfinite(step)) v -= step;
    }
    x[k] = k < n ? v : 0.0;
  }
  return n;
}

// The inlier decision is made in plain IEEE arithmetic, every product and sum rounded on its own and in the order
// written (no fused multiply-add): a restatement in another language then gets the same squared error for a pose
// and a point bit for bit, so counts compare exactly and costs to the rounding of their sums, also where a fit is
// exact and the error itself is rounding.
#if defined(__clang__)
#define SIM3OPT_PNP_NO_FMA _Pragma("clang fp contract(off)")
#else
#define SIM3OPT_PNP_NO_FMA
#endif

// R (row-major) of the unit quaternion q = x y z w
SIM3OPT_PNP_HD void pnp_quat_to_R(const double q[4], double R[9]) {
  SIM3OPT_PNP_NO_FMA
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// squared reprojection error of X (camera 0's frame) under (R row-major, t) against the pixel (u, v); z = its depth
SIM3OPT_PNP_HD double pnp_sqerr(const double R[9], const double t[3], const double X[3], double u, double v, double f,
                                double cx, double cy, double& z) {
  SIM3OPT_PNP_NO_FMA
  const double x = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + t[0];
  const double y = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + t[1];
  z = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + t[2];
  const double e0 = u - ((f * x) / z + cx), e1 = v - ((f * y) / z + cy);
  return e0 * e0 + e1 * e1;
}

// orthonormal frame of the triangle A0 A1 A2, columns E[3 * i + k]: e1 along A0 -> A1, e3 the normal, e2 = e3 x e1
SIM3OPT_PNP_HD void triangle_frame(const double A0[3], const double A1[3], const double A2[3], double E[9]) {
  double d1[3], d2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { d1[i] = A1[i] - A0[i]; d2[i] = A2[i] - A0[i]; }
  const double n1 = sqrt(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) d1[i] /= n1;
  double w[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
  const double nw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] /= nw;
  const double e2[3] = {w[1] * d1[2] - w[2] * d1[1], w[2] * d1[0] - w[0] * d1[2], w[0] * d1[1] - w[1] * d1[0]};
#pragma unroll
  for (int i = 0; i < 3; ++i) { E[3 * i] = d1[i]; E[3 * i + 1] = e2[i]; E[3 * i + 2] = w[i]; }
}

// One hypothesis: X (4 x 3) and uv (4 x 2) of the sample.  All P3P solutions with positive depths of the first three
// points (n_solutions counts them); of those that put the fourth point in front of the camera, the one with the
// smallest squared reprojection error on it goes to R (row-major), t.  Returns whether there is one; R and t are
// finite then, and untouched garbage is never left: without one they are the identity.
SIM3OPT_PNP_HD bool p3p_hypothesis(const double X[4][3], const double uv[4][2], double f, double cx, double cy,
                                   double R[9], double t[3], int& n_solutions) {
  n_solutions = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  t[0] = t[1] = t[2] = 0.0;
  double J[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double x = (uv[k][0] - cx) / f, y = (uv[k][1] - cy) / f;
    const double nn = sqrt(x * x + y * y + 1.0);
    J[k][0] = x / nn; J[k][1] = y / nn; J[k][2] = 1.0 / nn;
  }
  double d12[3], d13[3], d23[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { d12[i] = X[1][i] - X[0][i]; d13[i] = X[2][i] - X[0][i]; d23[i] = X[2][i] - X[1][i]; }
  const double c2 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
  const double b2 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
  const double a2 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];
  const double w0 = d12[1] * d13[2] - d12[2] * d13[1], w1 = d12[2] * d13[0] - d12[0] * d13[2],
               w2 = d12[0] * d13[1] - d12[1] * d13[0];
  // two equal points, or three on a line (the sine of their angle below 1e-10): no pose
  if (!(a2 > 0.0) || !(b2 > 0.0) || !(c2 > 0.0) || !(w0 * w0 + w1 * w1 + w2 * w2 > 1e-20 * b2 * c2)) return false;
  const double cg = J[0][0] * J[1][0] + J[0][1] * J[1][1] + J[0][2] * J[1][2];
  const double cb = J[0][0] * J[2][0] + J[0][1] * J[2][1] + J[0][2] * J[2][2];
  const double ca = J[1][0] * J[2][0] + J[1][1] * J[2][1] + J[1][2] * J[2][2];
  // u = N / D:  N = (k - 1) v^2 - 2 k cos(b) v + (1 + k), k = (a^2 - c^2) / b^2;  D = 2 (cos(g) - cos(a) v)
  const double k = (a2 - c2) / b2, qq = c2 / b2;
  const double N[3] = {1.0 + k, -2.0 * k * cb, k - 1.0};
  const double D[2] = {2.0 * cg, -2.0 * ca};
  // N^2 - 2 cos(g) N D + D^2 (1 - q (1 + v^2 - 2 cos(b) v)) = 0,  q = c^2 / b^2
  const double D2[3] = {D[0] * D[0], 2.0 * D[0] * D[1], D[1] * D[1]};
  const double W[3] = {1.0 - qq, 2.0 * qq * cb, -qq};
  double c[5];
  c[0] = N[0] * N[0] - 2.0 * cg * (N[0] * D[0]) + D2[0] * W[0];
  c[1] = 2.0 * N[0] * N[1] - 2.0 * cg * (N[0] * D[1] + N[1] * D[0]) + D2[0] * W[1] + D2[1] * W[0];
  c[2] = 2.0 * N[0] * N[2] + N[1] * N[1] - 2.0 * cg * (N[1] * D[1] + N[2] * D[0]) + D2[0] * W[2] + D2[1] * W[1] +
         D2[2] * W[0];
  c[3] = 2.0 * N[1] * N[2] - 2.0 * cg * (N[2] * D[1]) + D2[1] * W[2] + D2[2] * W[1];
  c[4] = N[2] * N[2] + D2[2] * W[2];
  double root[4];
  const int nr = quartic_real_roots(c, root);
  double E[9];
  triangle_frame(X[0], X[1], X[2], E);
  double best = 0.0;
  bool found = false;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double v = root[r];
    const double den = D[0] + D[1] * v;
    const double u = ((N[2] * v + N[1]) * v + N[0]) / den;
    const double s1 = sqrt(b2 / (1.0 + v * v - 2.0 * v * cb));
    const double s2 = u * s1, s3 = v * s1;
    if (!(r < nr) || !(v > 0.0) || !(u > 0.0) || !(s1 > 0.0) || !std::isfinite(s1 + s2 + s3)) continue;
    ++n_solutions;
    double Y[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { Y[0][i] = s1 * J[0][i]; Y[1][i] = s2 * J[1][i]; Y[2][i] = s3 * J[2][i]; }
    double F[9], Rr[9], tr[3];
    triangle_frame(Y[0], Y[1], Y[2], F);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Rr[3 * i + j] = F[3 * i] * E[3 * j] + F[3 * i + 1] * E[3 * j + 1] + F[3 * i + 2] * E[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) tr[i] = Y[0][i] - (Rr[3 * i] * X[0][0] + Rr[3 * i + 1] * X[0][1] + Rr[3 * i + 2] * X[0][2]);
    double z, fin = tr[0] + tr[1] + tr[2];
#pragma unroll
    for (int i = 0; i < 9; ++i) fin += Rr[i];
    const double e2 = pnp_sqerr(Rr, tr, X[3], uv[3][0], uv[3][1], f, cx, cy, z);
    if (!std::isfinite(fin) || !(z > 0.0) || !std::isfinite(e2)) continue;
    if (!found || e2 < best) {
      found = true;
      best = e2;
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = Rr[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = tr[i];
    }
  }
  return found;
}

}  // namespace sim3opt_pnp
