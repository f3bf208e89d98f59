// sim3_jac.hpp -- closed-form Jacobians of EdgeSim3's residual (host + device), the opt-in alternative to the
// central differences of k_linearize_numeric (options.jacobians = 1; DESIGN.md "Analytic Jacobians").
//
//   e = log(C S0 S1^-1),  updates S <- exp(d) S,  tangent order [omega, upsilon, sigma]
//   J0 = de/dd0 =  J_l(e)^-1 Ad_C
//   J1 = de/dd1 = -J_l(e)^-1 Ad_exp(e)                      (= -J_r(e)^-1)
//   Ad_S = [[R, 0, 0], [[t]x R, s R, -t], [0, 0, 1]]         for S = (R, t, s)
//   J_l(xi) = int_0^1 Ad_exp(u xi) du = [[J_SO3, 0, 0], [Q, V, q], [0, 0, 1]]
//
// J_l is evaluated by a 12-node Gauss-Legendre rule on [0, 1] (its integrand is an entire function of u: the
// rule converges spectrally, 8 nodes are at 1.5e-14 for theta <= pi, |sigma| <= 3), summed in node order.
// exp(u xi) at the nodes is evaluated to full precision for every argument (exp_exact below: no small-angle
// branch, whatever the graph's exp/log options are).  J_l^-1 is applied by block substitution (3x3 LU solves
// with J_SO3 and V); no inverse is formed.  These are the derivatives of the EXACT map: the library's log
// switches to theta = 0 coefficients below theta ~ 4.5e-3, where the numeric Jacobians of the residual as
// evaluated differ from these by ~0.12 theta^2 (fix_small_angle_b = 1) or by O(1) (as-written B: refused).
#pragma once

#include "sim3_math.hpp"

namespace sim3 {

constexpr int JAC_NODES = 12;
constexpr int JAC_SUMS = 30;  // per node: R (9), e^{u sigma} R (9), [t]x R (9), -t (3) -- weighted

// Gauss-Legendre rule on [0, 1]: node k and its weight (selects, not a table: no private-memory array on the
// device when k is a lane index)
S3_HD void gl_node(int k, double& u, double& w) {
  u = k == 0 ? 0.009219682876640375 : k == 1 ? 0.04794137181476257 : k == 2 ? 0.11504866290284765
    : k == 3 ? 0.2063410228566913 : k == 4 ? 0.3160842505009099 : k == 5 ? 0.43738329574426554
    : k == 6 ? 0.5626167042557345 : k == 7 ? 0.6839157494990901 : k == 8 ? 0.7936589771433087
    : k == 9 ? 0.8849513370971523 : k == 10 ? 0.9520586281852375 : 0.9907803171233597;
  w = (k == 0 || k == 11) ? 0.023587668193255914 : (k == 1 || k == 10) ? 0.05346966299765921
    : (k == 2 || k == 9) ? 0.08003916427167311 : (k == 3 || k == 8) ? 0.10158371336153296
    : (k == 4 || k == 7) ? 0.1167462682691774 : 0.12457352290670139;
}

// sin(x)/x and (1 - cos x)/x^2 = 2 (sin(x/2)/x)^2 without cancellation, x >= 0
S3_HD void sinc_and_h(double x, double& sinc, double& h) {
  S3_STRICT_FP
  if (x == 0.0) {
    sinc = 1.0;
    h = 0.5;
  } else {
    const double ix = 1.0 / x;
    sinc = sin(x) * ix;
    const double r = sin(0.5 * x) * ix;
    h = 2.0 * r * r;
  }
}

// A, B, C of W = A Omega + B Omega^2 + C I = int_0^1 e^{u sigma} R(u omega) du, accurate for every (theta, sigma):
//   C = phi(sigma), A = Im phi(z) / theta, B = (phi(sigma) - Re phi(z)) / theta^2,  phi(z) = (e^z - 1)/z, z = sigma + i theta.
// |z| < 1: the power series of phi, with z^n = p_n + i theta q_n and sigma^n - p_n = theta^2 r_n (no division by
// theta); else the closed forms, rearranged so that neither theta nor sigma divides a difference that vanishes
// (s = e^sigma, sinc and h of theta as sinc_and_h gives them; cos theta = 1 - theta^2 h).
S3_HD void w_coeffs_exact(double theta, double sigma, double s, double sinc, double h, double& A, double& B,
                          double& C) {
  S3_STRICT_FP
  const double th2 = theta * theta, rho2 = th2 + sigma * sigma;
  if (rho2 < 1.0) {
    double p = 1.0, q = 0.0, r = 0.0, sg = 1.0, f = 1.0;  // f = 1/(n+1)!
    A = 0.0;
    B = 0.0;
    C = 0.0;
#pragma unroll
    for (int n = 0; n < 20; ++n) {  // |term| < n^2 / (n+1)! : below 1e-17 after 20 terms
      C += sg * f;
      A += q * f;
      B += r * f;
      const double p1 = sigma * p - th2 * q, q1 = p + sigma * q, r1 = sigma * r + q;
      p = p1;
      q = q1;
      r = r1;
      sg *= sigma;
      f *= 1.0 / (double)(n + 2);  // (a constant once unrolled: no division on the device)
    }
  } else {
    const double irho2 = 1.0 / rho2;
    C = sigma == 0.0 ? 1.0 : expm1(sigma) / sigma;
    A = (s * sinc * sigma + ((1.0 - s) + s * th2 * h)) * irho2;  // 1 - s cos(theta)
    B = (C + s * sigma * h - s * sinc) * irho2;
  }
}

// exp(u xi) as R (row-major), t, scale -- the exact map, no branch thresholds
S3_HD void exp_exact(const double xi[7], double u, double R[9], double t[3], double& scale) {
  S3_STRICT_FP
  const double om[3] = {u * xi[0], u * xi[1], u * xi[2]};
  const double up[3] = {u * xi[3], u * xi[4], u * xi[5]};
  const double sigma = u * xi[6];
  const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
  double Om[9], Om2[9], sinc, h, A, B, C;
  skew_and_square(om, Om, Om2);
  sinc_and_h(theta, sinc, h);
  scale = ::exp(sigma);
  w_coeffs_exact(theta, sigma, scale, sinc, h, A, B, C);
  double W[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    R[i] = sinc * Om[i] + h * Om2[i];
    W[i] = A * Om[i] + B * Om2[i];
  }
  R[0] += 1; R[4] += 1; R[8] += 1;
  W[0] += C; W[4] += C; W[8] += C;
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = W[3 * i] * up[0] + W[3 * i + 1] * up[1] + W[3 * i + 2] * up[2];
}

// y = Ad_S x for S = (R row-major, t, s).  (Jacobian columns apply it to unit vectors: with a lane's column index
// a select of R's entries would become a dynamically indexed private array; x 1 and x 0 are exact)
S3_HD void adjoint_apply(const double R[9], const double t[3], double s, const double x[7], double y[7]) {
  S3_STRICT_FP
  double Rw[3], Ru[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Rw[i] = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
    Ru[i] = R[3 * i] * x[3] + R[3 * i + 1] * x[4] + R[3 * i + 2] * x[5];
  }
  y[0] = Rw[0]; y[1] = Rw[1]; y[2] = Rw[2];
  y[3] = (t[1] * Rw[2] - t[2] * Rw[1]) + s * Ru[0] - t[0] * x[6];  // [t]x R w + s R u - t sigma
  y[4] = (t[2] * Rw[0] - t[0] * Rw[2]) + s * Ru[1] - t[1] * x[6];
  y[5] = (t[0] * Rw[1] - t[1] * Rw[0]) + s * Ru[2] - t[2] * x[6];
  y[6] = x[6];
}

// Ad_S, row-major 7x7
S3_HD void adjoint(const Sim3& S, double Ad[49]) {
  double R[9], x[7], col[7];
  R_from_quat(S.q, R);
  for (int c = 0; c < 7; ++c) {
    for (int i = 0; i < 7; ++i) x[i] = i == c ? 1.0 : 0.0;
    adjoint_apply(R, S.t, S.s, x, col);
    for (int r = 0; r < 7; ++r) Ad[7 * r + c] = col[r];
  }
}

// weighted contribution of Gauss-Legendre node k to the J_l integrals (JAC_SUMS values, see above)
S3_HD void left_jacobian_node(const double xi[7], int k, double out[JAC_SUMS]) {
  S3_STRICT_FP
  double u, w, R[9], t[3], sc;
  gl_node(k, u, w);
  exp_exact(xi, u, R, t, sc);
  const double ws = w * sc;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int a = (i + 1) % 3, b = (i + 2) % 3;  // ([t]x R)_ij = t_a R_bj - t_b R_aj
      out[3 * i + j] = w * R[3 * i + j];
      out[9 + 3 * i + j] = ws * R[3 * i + j];
      out[18 + 3 * i + j] = w * (t[a] * R[3 * b + j] - t[b] * R[3 * a + j]);
    }
  out[27] = -(w * t[0]);
  out[28] = -(w * t[1]);
  out[29] = -(w * t[2]);
}

// J_l(xi) as its blocks M = [J_SO3 (9), V (9), Q (9), q (3)] (row-major 3x3): node contributions summed in
// node order (the linearisation kernel sums the same contributions in the same order through LDS)
S3_HD void left_jacobian_blocks(const double xi[7], double M[JAC_SUMS]) {
#pragma unroll
  for (int i = 0; i < JAC_SUMS; ++i) M[i] = 0.0;
  for (int k = 0; k < JAC_NODES; ++k) {
    double v[JAC_SUMS];
    left_jacobian_node(xi, k, v);
#pragma unroll
    for (int i = 0; i < JAC_SUMS; ++i) M[i] += v[i];
  }
}

// x = J_l^-1 y by block substitution over the blocks M of left_jacobian_blocks
S3_HD void left_jacobian_solve(const double M[JAC_SUMS], const double y[7], double x[7]) {
  S3_STRICT_FP
  x[6] = y[6];
  solve33(M, y, x);
  const double r[3] = {y[3] - (M[18] * x[0] + M[19] * x[1] + M[20] * x[2]) - M[27] * x[6],
                       y[4] - (M[21] * x[0] + M[22] * x[1] + M[23] * x[2]) - M[28] * x[6],
                       y[5] - (M[24] * x[0] + M[25] * x[1] + M[26] * x[2]) - M[29] * x[6]};
  solve33(M + 9, r, x + 3);
}

// exp(e) as the 13 values [R (9), t (3), s] edge_jacobian_column takes
S3_HD void exp_of_residual(const double e[7], double X[13]) {
  exp_exact(e, 1.0, X, X + 9, X[12]);
}

// Column c (0..13) of [J0 | J1] at the residual e: c < 7 is column c of J0 (S0's tangent), else column c - 7 of
// J1.  M: left_jacobian_blocks(e), X: exp_of_residual(e).  Cleared bit d of dof_mask zeroes column d of both
// endpoints, as in k_linearize_numeric.
S3_HD void edge_jacobian_column(const double M[JAC_SUMS], const double X[13], const Sim3& C, int c, int dof_mask,
                                double col[7]) {
  S3_STRICT_FP
  const int d = c < 7 ? c : c - 7;
  if (!((dof_mask >> d) & 1)) {
#pragma unroll
    for (int r = 0; r < 7; ++r) col[r] = 0.0;
    return;
  }
  double x[7], y[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) x[i] = i == d ? 1.0 : 0.0;
  if (c < 7) {
    double R[9];
    R_from_quat(C.q, R);
    adjoint_apply(R, C.t, C.s, x, y);
  } else {
    adjoint_apply(X, X + 9, X[12], x, y);
#pragma unroll
    for (int r = 0; r < 7; ++r) y[r] = -y[r];
  }
  left_jacobian_solve(M, y, col);
}

// e = log(C S0 S1^-1) (sim3::edge_error with the graph's options: the residual, and chi2, are the numeric path's)
// and its Jacobians, J row-major 7 x 14: J[14 r + c], columns 0..6 for S0, 7..13 for S1
S3_HD void edge_jacobians(const Sim3& C, const Sim3& S0, const Sim3& S1, const Opts& o, int dof_mask,
                          double e[7], double J[98]) {
  edge_error(C, S0, S1, o, e);
  double M[JAC_SUMS], X[13];
  left_jacobian_blocks(e, M);
  exp_of_residual(e, X);
  for (int c = 0; c < 14; ++c) {
    double col[7];
    edge_jacobian_column(M, X, C, c, dof_mask, col);
    for (int r = 0; r < 7; ++r) J[14 * r + c] = col[r];
  }
}

}  // namespace sim3
