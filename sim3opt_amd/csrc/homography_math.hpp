// homography_math.hpp -- the arithmetic of the batched homography stage (homography_batch.hip): the four-point
// homography, the pixel error of a correspondence under H, the terms of a Tukey-reweighted refinement round with its
// 9 x 9 solve, the Faugeras-Lustman decomposition and the order of its eight results (HomographyInit.cc:14-33, :65-177,
// :232-435; MEstimator.h:54-89; the sampler: ransac_sample.hpp).  Host and device: tests/cxx/homography_math_driver.cpp
// runs the same statements on the CPU against tests/homography_ref.py.
//
// What is the reference's: every formula from the pixel error on, in the order it writes them.  What is ours: the
// linear algebra (TooN's SVD and WLS are a closed form, a Cholesky factorisation and a Jacobi eigen-solver here).
//   four points   the reference takes the null vector of the 8 x 9 system.  Here: a_3 = sum_j l_j a_j makes
//                 A = [l_0 a_0 | l_1 a_1 | l_2 a_2] the map from the standard projective basis to the four points of
//                 view 0, B likewise for view 1, and H = B adj(A), the same matrix up to scale.  No pivoting, no array
//                 indexed at run time.  Scaled to Frobenius norm 1 (the refinement's unit prior sees that scale).
//   9 x 9 solve   J^T W J of a correspondence is a multiple of (x, y, 1)(x, y, 1)^T in each of its 3 x 3 blocks, so a
//                 round sums HOM_ACC = 33 numbers per thread instead of 54.
//   3 x 3 SVD     V and d_i^2 from JACOBI_SWEEPS cyclic Jacobi sweeps on H^T H, U = H V diag(1 / d).
// Every loop has a constant bound; every index of a private array is a compile-time constant once unrolled, so
// nothing goes to scratch.
#pragma once
#include <cmath>
#include <cstdint>

#include "ransac_sample.hpp"

#define SIM3OPT_HOM_HD SIM3OPT_RANSAC_HD

// No fused multiply-add anywhere in this stage, as in essential_math.hpp: the device rounds every operation as the
// host build of these statements does (tests/test_gpu_homography_batch.py compares the hypotheses bit for bit).
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sim3opt_homography {

// A sample is refused when twice the area of a triangle of three of its points, in camera-plane units, is at most
// this in either view (0.55 x 0.18 is the image; 1e-9 is a triangle of 0.02 px side): collinear or repeated points.
constexpr double COLLINEAR_MIN = 1e-9;
constexpr int JACOBI_SWEEPS = 8;  // cyclic sweeps on the 3 x 3 matrix H^T H (converged to the last bit after four)
constexpr int HOM_ACC = 33;       // what a refinement round sums: 4 x 6 of the normal matrix, 9 of its right side
constexpr int MAX_ROUNDS = 8;     // refine_rounds at most

// twice the signed area of the triangle a b c
SIM3OPT_HOM_HD double hom_area2(const double a[2], const double b[2], const double c[2]) {
  return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]);
}

// The map from the standard projective basis to p[0..3] (x, y, 1), columns scaled so that their sum is p[3] times
// the area of the first three: M row-major.  False when a triple is (nearly) collinear.
SIM3OPT_HOM_HD bool hom_basis(const double p0[2], const double p1[2], const double p2[2], const double p3[2],
                              double M[9]) {
  const double D = hom_area2(p0, p1, p2);
  const double l0 = hom_area2(p3, p1, p2), l1 = hom_area2(p0, p3, p2), l2 = hom_area2(p0, p1, p3);
  M[0] = l0 * p0[0]; M[1] = l1 * p1[0]; M[2] = l2 * p2[0];
  M[3] = l0 * p0[1]; M[4] = l1 * p1[1]; M[5] = l2 * p2[1];
  M[6] = l0;         M[7] = l1;         M[8] = l2;
  return fabs(D) > COLLINEAR_MIN && fabs(l0) > COLLINEAR_MIN && fabs(l1) > COLLINEAR_MIN && fabs(l2) > COLLINEAR_MIN;
}

SIM3OPT_HOM_HD void hom_identity(double H[9]) {
  H[0] = 1.0; H[1] = 0.0; H[2] = 0.0; H[3] = 0.0; H[4] = 1.0; H[5] = 0.0; H[6] = 0.0; H[7] = 0.0; H[8] = 1.0;
}

// HomographyFromMatches (:65-115) of four correspondences q[k] = (x0, y0, x1, y1), second = H first, Frobenius norm
// 1, the sign as it comes.  Invalid (the identity stored): a collinear triple or a repeated point in either view,
// a non-finite entry.
SIM3OPT_HOM_HD bool hom_four_point(const double q[4][4], double H[9]) {
  double A[9], B[9];
  const bool oka = hom_basis(&q[0][0], &q[1][0], &q[2][0], &q[3][0], A);
  const bool okb = hom_basis(&q[0][2], &q[1][2], &q[2][2], &q[3][2], B);
  // adj(A), row-major
  const double C[9] = {A[4] * A[8] - A[5] * A[7], A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                       A[5] * A[6] - A[3] * A[8], A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                       A[3] * A[7] - A[4] * A[6], A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
  double G[9], s = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      G[3 * r + c] = (B[3 * r] * C[c] + B[3 * r + 1] * C[3 + c]) + B[3 * r + 2] * C[6 + c];
      s += G[3 * r + c] * G[3 * r + c];
    }
  }
  const double norm = sqrt(s);
  bool ok = oka && okb && norm > 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    G[i] = G[i] / norm;
    ok = ok && std::isfinite(G[i]);
  }
  if (ok) {
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = G[i];
  } else {
    hom_identity(H);
  }
  return ok;
}

// The pixel error of (x0, y0) -> (x1, y1) under H (:16-19, :133-136; m2PixelProjectionJac = f I): e = f (second -
// project(H unproject(first))), returns |e|^2 [px^2] and the projective depth in den.
SIM3OPT_HOM_HD double hom_error(const double H[9], double x0, double y0, double x1, double y1, double f, double& ex,
                                double& ey, double& p0, double& p1, double& den) {
  p0 = (H[0] * x0 + H[1] * y0) + H[2];
  p1 = (H[3] * x0 + H[4] * y0) + H[5];
  den = (H[6] * x0 + H[7] * y0) + H[8];
  ex = f * (x1 - p0 / den);
  ey = f * (y1 - p1 / den);
  return ex * ex + ey * ey;
}

SIM3OPT_HOM_HD double hom_sqerr(const double H[9], double x0, double y0, double x1, double y1, double f) {
  double ex, ey, p0, p1, den;
  return hom_error(H, x0, y0, x1, y1, f, ex, ey, p0, p1, den);
}

// MLESACScore (:23-33): the squared error, max2 where it is larger or not a number
SIM3OPT_HOM_HD double hom_mlesac(double e2, double max2) { return e2 < max2 ? e2 : max2; }

// Tukey::FindSigmaSquared (MEstimator.h:79-89) once the median (the element of rank m / 2 of the m squared errors)
// is known, and Tukey::Weight (:54-66)
SIM3OPT_HOM_HD double hom_sigma2(double median, int m) {
  double sigma = 1.4826 * (1 + 5.0 / (double)(m * 2 - 6)) * sqrt(median);
  sigma = 4.6851 * sigma;
  return sigma * sigma;
}

SIM3OPT_HOM_HD double hom_weight(double e2, double sigma2) {
  if (e2 > sigma2) return 0.0;
  const double r = 1.0 - e2 / sigma2;
  return r * r;
}

// One correspondence's share of the normal equations of RefineHomographyWithInliers (:129-169), weight w.  The rows
// of its Jacobian are a (u, 0, 0) + c0 (0, 0, u) and a (0, u, 0) + c1 (0, 0, u), u = (x0, y0, 1), a = f / den,
// c = -f p / den^2.  acc: [0, 6) w a^2 uu, [6, 12) w a c0 uu, [12, 18) w a c1 uu, [18, 24) w (c0^2 + c1^2) uu, with
// uu = (xx, xy, x, yy, y, 1); [24, 27) w a ex u, [27, 30) w a ey u, [30, 33) w (c0 ex + c1 ey) u.
SIM3OPT_HOM_HD void hom_accumulate(double acc[HOM_ACC], double w, double x0, double y0, double f, double ex,
                                   double ey, double p0, double p1, double den) {
  const double a = f / den, den2 = den * den;
  const double c0 = -(f * p0) / den2, c1 = -(f * p1) / den2;
  const double uu[6] = {x0 * x0, x0 * y0, x0, y0 * y0, y0, 1.0}, u[3] = {x0, y0, 1.0};
  const double k[4] = {w * (a * a), w * (a * c0), w * (a * c1), w * (c0 * c0 + c1 * c1)};
  const double g[3] = {w * (a * ex), w * (a * ey), w * (c0 * ex + c1 * ey)};
#pragma unroll
  for (int b = 0; b < 4; ++b) {
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[6 * b + i] += k[b] * uu[i];
  }
#pragma unroll
  for (int b = 0; b < 3; ++b) {
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[24 + 3 * b + i] += g[b] * u[i];
  }
}

SIM3OPT_HOM_HD constexpr int hom_sym(int i, int j) {  // where (i, j) of a symmetric 3 x 3 lies in uu's order
  return i == j ? (i == 0 ? 0 : i == 1 ? 3 : 5) : (i + j == 1 ? 1 : i + j == 2 ? 2 : 4);
}

// wls.add_prior(1.0), compute(), get_mu() (:122-123, :170-171): (I + J^T W J) update = J^T W e from the sums of a
// round, by a Cholesky factorisation.  A pivot that is not positive leaves NaN in the update (and in H: the problem
// then ends as degenerate).
SIM3OPT_HOM_HD void hom_solve_update(const double acc[HOM_ACC], double prior, double upd[9]) {
  double M[9][9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int s = hom_sym(i, j);
      M[i][j] = acc[s];          M[i][3 + j] = 0.0;          M[i][6 + j] = acc[6 + s];
      M[3 + i][j] = 0.0;         M[3 + i][3 + j] = acc[s];   M[3 + i][6 + j] = acc[12 + s];
      M[6 + i][j] = acc[6 + s];  M[6 + i][3 + j] = acc[12 + s]; M[6 + i][6 + j] = acc[18 + s];
    }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) M[i][i] += prior;
  // M = L L^T, L in the lower triangle
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    double d = M[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= M[j][k] * M[j][k];
    d = sqrt(d);
    M[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < 9; ++i) {
      double s = M[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= M[i][k] * M[j][k];
      M[i][j] = s / d;
    }
  }
  double y[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    double s = acc[24 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= M[i][k] * y[k];
    y[i] = s / M[i][i];
  }
#pragma unroll
  for (int i = 8; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 9; ++k) s -= M[k][i] * upd[k];
    upd[i] = s / M[i][i];
  }
}

// ---- DecomposeHomography (:232-339) ----
struct HomSvd {
  double U[9], V[9];  // row-major; H = U diag(d) V^T
  double d1, d2, d3;  // descending
  double s;           // det U det V
};

template <int P, int Q>
SIM3OPT_HOM_HD void hom_jacobi_rotate(double a[3][3], double v[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = 0.0; a[Q][P] = 0.0;
  const double arp = a[R][P], arq = a[R][Q];
  a[R][P] = c * arp - s * arq; a[P][R] = a[R][P];
  a[R][Q] = s * arp + c * arq; a[Q][R] = a[R][Q];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = v[k][P], vq = v[k][Q];
    v[k][P] = c * vp - s * vq;
    v[k][Q] = s * vp + c * vq;
  }
}

template <int P, int Q>
SIM3OPT_HOM_HD void hom_order_columns(double lam[3], double v[3][3]) {  // the larger eigenvalue to column P < Q
  if (lam[Q] > lam[P]) {
    const double l = lam[P]; lam[P] = lam[Q]; lam[Q] = l;
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double x = v[k][P]; v[k][P] = v[k][Q]; v[k][Q] = x; }
  }
}

SIM3OPT_HOM_HD double hom_det3(const double M[9]) {
  return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) +
         M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// The SVD of H.  False -- the reference's "not implemented or degenerate" (:249-260) -- unless d1 != d2 and
// d2 != d3 exactly and everything is finite.
SIM3OPT_HOM_HD bool hom_svd(const double H[9], HomSvd& S) {
  double a[3][3], v[3][3], lam[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      a[i][j] = (H[i] * H[j] + H[3 + i] * H[3 + j]) + H[6 + i] * H[6 + j];
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  }
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    hom_jacobi_rotate<0, 1>(a, v);
    hom_jacobi_rotate<0, 2>(a, v);
    hom_jacobi_rotate<1, 2>(a, v);
  }
  lam[0] = a[0][0]; lam[1] = a[1][1]; lam[2] = a[2][2];
  hom_order_columns<0, 1>(lam, v);
  hom_order_columns<0, 2>(lam, v);
  hom_order_columns<1, 2>(lam, v);
  // An eigenvector's sign is open, and with it which of the eight is which: the component of largest magnitude (the
  // first such) of every column of V is positive.
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double m0 = fabs(v[0][j]), m1 = fabs(v[1][j]), m2 = fabs(v[2][j]);
    const double lead = (m0 >= m1 && m0 >= m2) ? v[0][j] : (m1 >= m2 ? v[1][j] : v[2][j]);
    if (lead < 0.0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k][j] = -v[k][j];
    }
  }
  const double d[3] = {sqrt(fabs(lam[0])), sqrt(fabs(lam[1])), sqrt(fabs(lam[2]))};
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      S.V[3 * i + j] = v[i][j];
      S.U[3 * i + j] = ((H[3 * i] * v[0][j] + H[3 * i + 1] * v[1][j]) + H[3 * i + 2] * v[2][j]) / d[j];
      finite = finite && std::isfinite(S.U[3 * i + j]) && std::isfinite(v[i][j]);
    }
  }
  S.d1 = d[0]; S.d2 = d[1]; S.d3 = d[2];
  S.s = hom_det3(S.U) * hom_det3(S.V);
  return finite && std::isfinite(S.s) && S.d1 != S.d2 && S.d2 != S.d3;
}

// d of decomposition k (0..3: d' > 0, 4..7: d' < 0), all the first visibility test needs
SIM3OPT_HOM_HD double hom_decomposition_d(const HomSvd& S, int k) { return k < 4 ? S.s * S.d2 : S.s * -S.d2; }

// Decomposition k of the eight (:262-338), signs e1 = + - + -, e3 = + + - - within each four: R = s U Rp V^T,
// t = U tp, n = V np, d.
SIM3OPT_HOM_HD void hom_decomposition(const HomSvd& S, int k, double R[9], double t[3], double n[3], double& d) {
  const double d1 = S.d1, d2 = S.d2, d3 = S.d3;
  const double x1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));  // Eq. 12
  const double x3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const double e1 = (k & 1) ? -1.0 : 1.0, e3 = (k & 2) ? -1.0 : 1.0;
  double Rp[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, tp[3];
  if (k < 4) {
    d = S.s * d2;
    const double sn = (d1 - d3) * x1 * x3 * e1 * e3 / d2;  // Eq. 13
    const double cs = (d1 * x3 * x3 + d3 * x1 * x1) / d2;
    Rp[0] = cs; Rp[2] = -sn; Rp[4] = 1.0; Rp[6] = sn; Rp[8] = cs;
    tp[0] = (d1 - d3) * x1 * e1;  // Eq. 14
    tp[2] = (d1 - d3) * -x3 * e3;
  } else {
    d = S.s * -d2;
    const double sn = (d1 + d3) * x1 * x3 * e1 * e3 / d2;  // Eq. 15
    const double cs = (d3 * x1 * x1 - d1 * x3 * x3) / d2;
    Rp[0] = cs; Rp[2] = sn; Rp[4] = -1.0; Rp[6] = sn; Rp[8] = -cs;
    tp[0] = (d1 + d3) * x1 * e1;  // Eq. 16
    tp[2] = (d1 + d3) * x3 * e3;
  }
  tp[1] = 0.0;
  const double np0 = x1 * e1, np2 = x3 * e3;
  double W[9];  // Rp V^T
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    n[i] = S.V[3 * i] * np0 + S.V[3 * i + 2] * np2;
    t[i] = S.U[3 * i] * tp[0] + S.U[3 * i + 2] * tp[2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      W[3 * i + j] = (Rp[3 * i] * S.V[3 * j] + Rp[3 * i + 1] * S.V[3 * j + 1]) + Rp[3 * i + 2] * S.V[3 * j + 2];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      R[3 * i + j] = S.s * ((S.U[3 * i] * W[j] + S.U[3 * i + 1] * W[3 + j]) + S.U[3 * i + 2] * W[6 + j]);
  }
}

// ---- ChooseBestDecomposition (:363-435) ----
// the two visibility tests of an inlier (x0, y0) of view 0
SIM3OPT_HOM_HD bool hom_visible_h(const double H[9], double x0, double y0, double d) {
  return ((H[6] * x0 + H[7] * y0) + H[8]) / d > 0.0;
}

SIM3OPT_HOM_HD bool hom_visible_n(const double n[3], double x0, double y0, double d) {
  return ((x0 * n[0] + y0 * n[1]) + n[2]) / d > 0.0;
}

// The first K of id[0..N) by larger count, then by smaller id (the reference's std::sort leaves the order of equals
// open; the decomposition's number decides here).  The ids are distinct.
template <int N, int K>
SIM3OPT_HOM_HD void hom_keep(const int id[N], const int count[N], int kept[K], int kept_count[K]) {
#pragma unroll
  for (int p = 0; p < K; ++p) { kept[p] = 0; kept_count[p] = 0; }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) rank += (count[j] > count[k] || (count[j] == count[k] && id[j] < id[k])) ? 1 : 0;
#pragma unroll
    for (int p = 0; p < K; ++p)
      if (rank == p) { kept[p] = id[k]; kept_count[p] = count[k]; }
  }
}

// the essential matrix [t]x R of a decomposition (:412-415) and SampsonusError (:346-360) of second^T E first
SIM3OPT_HOM_HD void hom_essential(const double R[9], const double t[3], double E[9]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
    E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
    E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
  }
}

SIM3OPT_HOM_HD double hom_sampson(const double E[9], double x0, double y0, double x1, double y1, double limit) {
  const double a0 = (E[0] * x0 + E[1] * y0) + E[2];
  const double a1 = (E[3] * x0 + E[4] * y0) + E[5];
  const double a2 = (E[6] * x0 + E[7] * y0) + E[8];
  const double b0 = (E[0] * x1 + E[3] * y1) + E[6];
  const double b1 = (E[1] * x1 + E[4] * y1) + E[7];
  const double e = (x1 * a0 + y1 * a1) + a2;
  const double d = (e * e) / ((a0 * a0 + a1 * a1) + (b0 * b0 + b1 * b1));
  return d > limit ? limit : d;
}

// dRatio and the branch (:402-404): a comparison with NaN is false, so 0 / 0 takes the ambiguity branch
SIM3OPT_HOM_HD bool hom_ambiguous(int count0, int count1) {
  const double ratio = (double)(-count1) / (double)(-count0);
  return !(ratio < 0.9);
}

// R (row-major, a rotation) as the unit quaternion x y z w
SIM3OPT_HOM_HD void hom_R_to_quat(const double R[9], double q[4]) {
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0.0) {
    const double k = 2.0 * sqrt(tr + 1.0);
    q[3] = 0.25 * k; q[0] = (R[7] - R[5]) / k; q[1] = (R[2] - R[6]) / k; q[2] = (R[3] - R[1]) / k;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double k = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
    q[3] = (R[7] - R[5]) / k; q[0] = 0.25 * k; q[1] = (R[1] + R[3]) / k; q[2] = (R[2] + R[6]) / k;
  } else if (R[4] > R[8]) {
    const double k = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
    q[3] = (R[2] - R[6]) / k; q[0] = (R[1] + R[3]) / k; q[1] = 0.25 * k; q[2] = (R[5] + R[7]) / k;
  } else {
    const double k = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
    q[3] = (R[3] - R[1]) / k; q[0] = (R[2] + R[6]) / k; q[1] = (R[5] + R[7]) / k; q[2] = 0.25 * k;
  }
}

}  // namespace sim3opt_homography
