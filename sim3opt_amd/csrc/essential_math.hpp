// essential_math.hpp -- the per-hypothesis arithmetic of the batched essential-matrix RANSAC (essential_batch.hip):
// Nister's five-point method, the Sampson error, and the pose candidates of an essential matrix with the depths they
// are voted on (the sampler: ransac_sample.hpp).  Host and device: tests/cxx/essential_math_driver.cpp runs the same
// statements on the CPU against tests/essential_ref.py.
//
// Five points, the formulation.  Rows kron(x1, x0) of the five correspondences leave a four-dimensional null space
// X, Y, Z, W (Gauss-Jordan with full pivoting, then Gram-Schmidt); E = x X + y Y + z Z + W.  det E = 0 and
// 2 E E^T E - tr(E E^T) E = 0 are ten cubics in x, y, z: a 10 x 20 matrix in Nister's monomial order
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1,
// built from the trilinear forms of the basis (no table of expanded coefficients).  Gauss-Jordan with row pivoting
// on the left ten columns; the rows of x^2z, x^2, y^2z, y^2, xyz, xy give k = e - z f, l = g - z h, m = i - z j, a
// 3 x 3 matrix B(z) of polynomials with B (x, y, 1)^T = 0.  det B is the degree-10 polynomial; (x, y, 1) is
// proportional to the cross product of B's first two rows at a root.
// Real roots: a Sturm chain, the k-th smallest root by BISECTIONS halvings of the Cauchy interval on the chain's
// count, then NEWTON steps kept inside the last bracket.  Every solution then takes POLISH Gauss-Newton steps on the
// ten cubics themselves (ess_polish), which gives back the digits the elimination and the polynomial lose.  Every
// loop has a constant bound; nothing iterates "until converged".
//
// Work space: everything whose rows and columns are chosen at run time (the 5 x 9 system, the basis, the 10 x 20
// matrix, the polynomials, the Sturm chain) lives in WS_DOUBLES doubles the caller supplies -- LDS on the device, so
// that no run-time index ever addresses a private array (which the compiler would put in scratch).
// Lanes: a hypothesis is made by a group of lanes sharing that work space, one matrix row, and later one root, per
// lane (HostGroup below: the host runs the same statements with one lane taking every row).
#pragma once
#include <cmath>
#include <cstdint>

#include "pnp_math.hpp"

#define SIM3OPT_ESS_HD SIM3OPT_PNP_HD

// No fused multiply-add anywhere in this stage: the device then rounds every operation as the host build of these
// statements does, and a hypothesis has the same bits on both (division and sqrt are correctly rounded on both;
// tests/test_gpu_essential_batch.py compares the device's hypotheses with the host driver's bit for bit).
// That is what lets tests/test_essential_ref.py speak for the kernel: the number of real roots of a polynomial with
// two nearly equal roots can hang on the last bits of its coefficients.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sim3opt_essential {

constexpr int WS_DOUBLES = 236;           // the 10 x 20 matrix and the 4 x 9 basis; the layout is WS_* below
constexpr int BISECTIONS = 40;            // halvings of the Cauchy interval per root
constexpr int NEWTON = 6;                 // Newton steps on the degree-10 polynomial per root
constexpr int POLISH = 8;                 // Gauss-Newton steps of every solution on the ten cubics themselves
constexpr double POLISH_DONE = 1e-20;     // the polish has arrived when |r|^2 before its last step is at most this
constexpr double NULL_PIVOT_MIN = 1e-12;  // pivot of the 5 x 9 system (its entries are at most about 1)
constexpr double ELIM_PIVOT_MIN = 1e-12;  // pivot of the 10 x 20 matrix (built from an orthonormal basis)
constexpr double STURM_LEAD_MIN = 1e-14;  // leading coefficient of a member of the chain scaled to max |c| = 1

// Sampson's squared error of (x0, y0, 1) <-> (x1, y1, 1) under E (row-major), x1^T E x0 = 0.  Plain IEEE arithmetic,
// every operation rounded on its own in the order written (no fused multiply-add), as pnp_sqerr: a restatement gets
// the same bits.  A vanishing denominator gives NaN or inf, which no threshold admits.
SIM3OPT_ESS_HD double ess_sampson(const double E[9], double x0, double y0, double x1, double y1) {
  SIM3OPT_PNP_NO_FMA
  const double a0 = (E[0] * x0 + E[1] * y0) + E[2];
  const double a1 = (E[3] * x0 + E[4] * y0) + E[5];
  const double a2 = (E[6] * x0 + E[7] * y0) + E[8];
  const double b0 = (E[0] * x1 + E[3] * y1) + E[6];
  const double b1 = (E[1] * x1 + E[4] * y1) + E[7];
  const double d = (x1 * a0 + y1 * a1) + a2;
  const double den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
  return (d * d) / den;
}

// column of the monomial v_a v_b v_c (variables 0 x, 1 y, 2 z, 3 the constant 1) in Nister's order
SIM3OPT_ESS_HD constexpr int ess_col(int a, int b, int c) {
  const int nx = (a == 0) + (b == 0) + (c == 0), ny = (a == 1) + (b == 1) + (c == 1),
            nz = (a == 2) + (b == 2) + (c == 2);
  const int key = 16 * nx + 4 * ny + nz;
  return key == 48 ? 0 : key == 12 ? 1 : key == 36 ? 2 : key == 24 ? 3 : key == 33 ? 4 : key == 32 ? 5 :
         key == 9 ? 6 : key == 8 ? 7 : key == 21 ? 8 : key == 20 ? 9 : key == 18 ? 10 : key == 17 ? 11 :
         key == 16 ? 12 : key == 6 ? 13 : key == 5 ? 14 : key == 4 ? 15 : key == 3 ? 16 : key == 2 ? 17 :
         key == 1 ? 18 : 19;
}

// A hypothesis belongs to a group of lanes that share one work space.  The statements below are written once for
// both ways of running them: the rows of a matrix, and the roots, are dealt to the lanes by a stride loop
//   for (int r = g.first(); r < 10; r += g.step())
// and g.sync() stands between a phase that writes the work space and one that reads it.  On the host one "lane"
// takes every row in turn (first 0, step 1, sync nothing); on the device a lane takes the row of its own number.
struct HostGroup {
  int first() const { return 0; }
  int step() const { return 1; }
  bool leader() const { return true; }
  void sync() const {}
};

// Work space layout (doubles).  A and the basis V are live together; everything else aliases A once it is consumed.
constexpr int WS_A = 0;         // 10 x 20; before it the 5 x 9 system at 0 and the flag of the null space at 0
constexpr int WS_V = 200;       // 4 x 9 orthonormal basis
constexpr int WS_S = 0;         // Sturm chain: member i (degree 10 - i, 11 - i coefficients) at sturm_at(i), 66 in all
constexpr int WS_P = 66;        // the degree-10 polynomial det B (11)
constexpr int WS_B = 77;        // B(z): per row the x column (4 coefficients), the y column (4), the constant column (5)
constexpr int WS_META = 116;    // ok, Cauchy bound, real roots, sign changes at -inf
constexpr int WS_ROOT = 120;    // per root: the sixth point's error (-1 no root, -2 no finite error), then c (4)
constexpr int WS_E = 170;       // where the caller may leave the hypothesis's E (9): nothing above reads it

SIM3OPT_ESS_HD constexpr int sturm_at(int i) { return 11 * i - (i * (i - 1)) / 2; }

// Orthonormal basis of the null space of the rows kron(x1, x0) of q[0..4] = (x0, y0, x1, y1) into ws + WS_V.  False
// when a pivot is below NULL_PIVOT_MIN: two equal correspondences, or five that leave more than four dimensions.
// One lane's work.
SIM3OPT_ESS_HD bool ess_nullspace(const double q[6][4], double* ws) {
  double* const M = ws;  // 5 x 9
  double* const V = ws + WS_V;
  for (int r = 0; r < 5; ++r) {
    const double x0 = q[r][0], y0 = q[r][1], x1 = q[r][2], y1 = q[r][3];
    double* m = M + 9 * r;
    m[0] = x1 * x0; m[1] = x1 * y0; m[2] = x1;
    m[3] = y1 * x0; m[4] = y1 * y0; m[5] = y1;
    m[6] = x0; m[7] = y0; m[8] = 1.0;
  }
  unsigned used = 0;
  int pc[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    int br = k, bc = 0;
    double bv = -1.0;
    for (int r = k; r < 5; ++r)
      for (int c = 0; c < 9; ++c) {
        const double v = fabs(M[9 * r + c]);
        if (!((used >> c) & 1u) && v > bv) { bv = v; br = r; bc = c; }
      }
    if (!(bv > NULL_PIVOT_MIN)) return false;
    for (int c = 0; c < 9; ++c) { const double s = M[9 * br + c]; M[9 * br + c] = M[9 * k + c]; M[9 * k + c] = s; }
    const double inv = 1.0 / M[9 * k + bc];
    for (int c = 0; c < 9; ++c) M[9 * k + c] *= inv;
    for (int r = 0; r < 5; ++r) {
      if (r == k) continue;
      const double f = M[9 * r + bc];
      for (int c = 0; c < 9; ++c) M[9 * r + c] -= f * M[9 * k + c];
    }
    used |= 1u << bc;
    pc[k] = bc;
  }
  int j = 0;
  for (int c = 0; c < 9; ++c) {
    if ((used >> c) & 1u) continue;
    for (int i = 0; i < 9; ++i) V[9 * j + i] = 0.0;
    V[9 * j + c] = 1.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) V[9 * j + pc[k]] = -M[9 * k + c];
    ++j;
  }
  for (int a = 0; a < 4; ++a) {  // modified Gram-Schmidt
    for (int b = 0; b < a; ++b) {
      double dot = 0.0;
      for (int i = 0; i < 9; ++i) dot += V[9 * a + i] * V[9 * b + i];
      for (int i = 0; i < 9; ++i) V[9 * a + i] -= dot * V[9 * b + i];
    }
    double nn = 0.0;
    for (int i = 0; i < 9; ++i) nn += V[9 * a + i] * V[9 * a + i];
    const double inv = 1.0 / sqrt(nn);
    for (int i = 0; i < 9; ++i) V[9 * a + i] *= inv;
  }
  return true;
}

// Row r of the ten cubic constraints on E = x V[0] + y V[1] + z V[2] + V[3] (each V[a] a 3 x 3 matrix, row-major):
// row 0 det E, row 1 + 3 i + j the entry (i, j) of 2 E E^T E - tr(E E^T) E.  Each is a trilinear form of the basis,
// summed over the ordered triples (a, b, c) into the column of v_a v_b v_c.  One lane's work, row by row.
SIM3OPT_ESS_HD void ess_constraint_row(const double* V, int r, double* row) {
  for (int c = 0; c < 20; ++c) row[c] = 0.0;
  const int i = r > 0 ? (r - 1) / 3 : 0, j = r > 0 ? (r - 1) % 3 : 0;
  for (int a = 0; a < 4; ++a) {
    const double* Ea = V + 9 * a;
    for (int b = 0; b < 4; ++b) {
      const double* Eb = V + 9 * b;
      double g[3] = {0.0, 0.0, 0.0}, tr = 0.0;  // row i of Ea Eb^T, and its trace
      if (r > 0) {
#pragma unroll
        for (int l = 0; l < 3; ++l) g[l] = Ea[3 * i] * Eb[3 * l] + Ea[3 * i + 1] * Eb[3 * l + 1] + Ea[3 * i + 2] * Eb[3 * l + 2];
#pragma unroll
        for (int k = 0; k < 9; ++k) tr += Ea[k] * Eb[k];
      }
      for (int c = 0; c < 4; ++c) {
        const double* Ec = V + 9 * c;
        double val;
        if (r == 0)
          val = Ea[0] * (Eb[4] * Ec[8] - Eb[5] * Ec[7]) - Ea[1] * (Eb[3] * Ec[8] - Eb[5] * Ec[6]) +
                Ea[2] * (Eb[3] * Ec[7] - Eb[4] * Ec[6]);
        else
          val = 2.0 * (g[0] * Ec[j] + g[1] * Ec[3 + j] + g[2] * Ec[6 + j]) - tr * Ec[3 * i + j];
        row[ess_col(a, b, c)] += val;
      }
    }
  }
}

// Step k of the Gauss-Jordan elimination of A's left ten columns with row pivoting, in three phases with a sync
// between them: every lane finds the pivot row (the same in all: they read the same numbers); the leader swaps it
// into place and scales it; the owner of every other row subtracts its multiple.
SIM3OPT_ESS_HD int ess_pivot_row(const double* A, int k, double& big) {
  int br = k;
  big = -1.0;
  for (int r = k; r < 10; ++r) {
    const double v = fabs(A[20 * r + k]);
    if (v > big) { big = v; br = r; }
  }
  return br;
}

SIM3OPT_ESS_HD void ess_swap_scale(double* A, int k, int br) {
  for (int c = k; c < 20; ++c) { const double s = A[20 * br + c]; A[20 * br + c] = A[20 * k + c]; A[20 * k + c] = s; }
  const double inv = 1.0 / A[20 * k + k];
  for (int c = k; c < 20; ++c) A[20 * k + c] *= inv;
}

SIM3OPT_ESS_HD void ess_reduce_row(double* A, int k, int r) {
  if (r == k) return;
  const double f = A[20 * r + k];
  for (int c = k; c < 20; ++c) A[20 * r + c] -= f * A[20 * k + c];
}

// out (+)= sign * a * b for polynomials with NA and NB coefficients, lowest degree first
template <int NA, int NB>
SIM3OPT_ESS_HD void poly_mul_add(const double* a, const double* b, double sign, double* out) {
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) out[i + j] += sign * (a[i] * b[j]);
}

SIM3OPT_ESS_HD double poly_eval(const double* p, int n, double x) {  // n coefficients
  double v = p[n - 1];
  for (int i = n - 2; i >= 0; --i) v = v * x + p[i];
  return v;
}

// Sturm chain of the degree-10 polynomial p into S (member i of degree 10 - i at sturm_at(i), each scaled to
// max |c| = 1 by a positive factor); false when a leading coefficient is below STURM_LEAD_MIN
SIM3OPT_ESS_HD bool sturm_chain(const double* p, double* S) {
  double mx = 0.0;
  for (int j = 0; j < 11; ++j) mx = fmax(mx, fabs(p[j]));
  if (!(mx > 0.0) || !std::isfinite(mx)) return false;
  for (int j = 0; j < 11; ++j) S[j] = p[j] / mx;
  mx = 0.0;
  for (int j = 0; j < 10; ++j) { S[11 + j] = (double)(j + 1) * S[j + 1]; mx = fmax(mx, fabs(S[11 + j])); }
  if (!(mx > 0.0)) return false;
  for (int j = 0; j < 10; ++j) S[11 + j] /= mx;
  if (!(fabs(S[10]) > STURM_LEAD_MIN)) return false;
  for (int i = 1; i < 10; ++i) {
    const int d = 10 - i;  // degree of b = S[i]; a = S[i - 1] has degree d + 1; the next member d - 1
    const double* a = S + sturm_at(i - 1);
    const double* b = S + sturm_at(i);
    double* nx = S + sturm_at(i + 1);
    const double lb = b[d];
    if (!(fabs(lb) > STURM_LEAD_MIN)) return false;
    const double q1 = a[d + 1] / lb, q0 = (a[d] - q1 * b[d - 1]) / lb;
    mx = 0.0;
    for (int j = 0; j < d; ++j) {
      const double r = a[j] - q0 * b[j] - (j > 0 ? q1 * b[j - 1] : 0.0);
      nx[j] = -r;
      mx = fmax(mx, fabs(r));
    }
    if (!(mx > 0.0) || !std::isfinite(mx)) return false;
    for (int j = 0; j < d; ++j) nx[j] /= mx;
  }
  return true;
}

// sign changes of the chain at x
SIM3OPT_ESS_HD int sturm_changes(const double* S, double x) {
  int changes = 0, last = 0;
  for (int i = 0; i <= 10; ++i) {
    const int d = 10 - i;
    const double v = poly_eval(S + sturm_at(i), d + 1, x);
    const int s = v > 0.0 ? 1 : (v < 0.0 ? -1 : 0);
    if (s != 0) {
      if (last != 0 && s != last) ++changes;
      last = s;
    }
  }
  return changes;
}

// ... and at -inf (minus = true) or +inf
SIM3OPT_ESS_HD int sturm_changes_inf(const double* S, bool minus) {
  int changes = 0, last = 0;
  for (int i = 0; i <= 10; ++i) {
    const int d = 10 - i;
    int s = S[sturm_at(i) + d] > 0.0 ? 1 : -1;
    if (minus && (d & 1)) s = -s;
    if (last != 0 && s != last) ++changes;
    last = s;
  }
  return changes;
}

// From the eliminated A: B(z) of rows 4..9 (x^2z, x^2, y^2z, y^2, xyz, xy; columns 10..19: xz^2 xz x | yz^2 yz y |
// z^3 z^2 z 1), det B through the cross product (p1, p2, p3) of its first two rows, the Sturm chain and what the
// root finding needs, all into ws (which A leaves).  One lane's work.  ws[WS_META] says whether it succeeded.
SIM3OPT_ESS_HD void ess_polynomials(double* ws) {
  double bx[3][4], by[3][4], bc[3][5];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double* e = ws + 20 * (4 + 2 * r) + 10;
    const double* f = ws + 20 * (5 + 2 * r) + 10;
    bx[r][0] = e[2]; bx[r][1] = e[1] - f[2]; bx[r][2] = e[0] - f[1]; bx[r][3] = -f[0];
    by[r][0] = e[5]; by[r][1] = e[4] - f[5]; by[r][2] = e[3] - f[4]; by[r][3] = -f[3];
    bc[r][0] = e[9]; bc[r][1] = e[8] - f[9]; bc[r][2] = e[7] - f[8]; bc[r][3] = e[6] - f[7]; bc[r][4] = -f[6];
  }
  double p1[8], p2[8], p3[7], p[11];
#pragma unroll
  for (int i = 0; i < 8; ++i) p1[i] = p2[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) p3[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 11; ++i) p[i] = 0.0;
  poly_mul_add<4, 5>(by[0], bc[1], 1.0, p1);
  poly_mul_add<5, 4>(bc[0], by[1], -1.0, p1);
  poly_mul_add<5, 4>(bc[0], bx[1], 1.0, p2);
  poly_mul_add<4, 5>(bx[0], bc[1], -1.0, p2);
  poly_mul_add<4, 4>(bx[0], by[1], 1.0, p3);
  poly_mul_add<4, 4>(by[0], bx[1], -1.0, p3);
  poly_mul_add<8, 4>(p1, bx[2], 1.0, p);
  poly_mul_add<8, 4>(p2, by[2], 1.0, p);
  poly_mul_add<7, 5>(p3, bc[2], 1.0, p);
  double fin = 0.0, bound = 0.0;
#pragma unroll
  for (int i = 0; i < 11; ++i) { fin += p[i]; ws[WS_P + i] = p[i]; }
#pragma unroll
  for (int i = 0; i < 10; ++i) bound = fmax(bound, fabs(p[i] / p[10]));
  bound += 1.0;  // Cauchy: every root lies in [-bound, bound]
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { ws[WS_B + 13 * r + i] = bx[r][i]; ws[WS_B + 13 * r + 4 + i] = by[r][i]; }
#pragma unroll
    for (int i = 0; i < 5; ++i) ws[WS_B + 13 * r + 8 + i] = bc[r][i];
  }
  bool ok = std::isfinite(fin) && std::isfinite(bound);
  if (ok) ok = sturm_chain(ws + WS_P, ws + WS_S);
  int at_minus = 0, nr = 0;
  if (ok) {
    at_minus = sturm_changes_inf(ws + WS_S, true);
    nr = at_minus - sturm_changes_inf(ws + WS_S, false);
  }
  ws[WS_META] = ok ? 1.0 : 0.0;
  ws[WS_META + 1] = ok ? bound : 0.0;
  ws[WS_META + 2] = (double)nr;
  ws[WS_META + 3] = (double)at_minus;
}

// E = c0 V[0] + c1 V[1] + c2 V[2] + c3 V[3] scaled to Frobenius norm 1; false (E zero) when it is not finite
SIM3OPT_ESS_HD bool ess_E_of_c(const double* V, const double c[4], double E[9]) {
  double nn = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    E[i] = c[0] * V[i] + c[1] * V[9 + i] + c[2] * V[18 + i] + c[3] * V[27 + i];
    nn += E[i] * E[i];
  }
  const double inv = 1.0 / sqrt(nn);
  const bool ok = std::isfinite(inv) && std::isfinite(nn);
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = ok ? E[i] * inv : 0.0;
  return ok;
}

// POLISH Gauss-Newton steps of a solution on the ten cubics r = (det E, 2 E E^T E - tr(E E^T) E), evaluated from E
// itself rather than from the eliminated coefficients: what the elimination and the polynomial lost of a solution's
// digits comes back, since the residual vanishes at a solution and the steps converge quadratically.  The unknown is
// the unit vector c of E = sum c_v V[v] (so a solution with a small share of V[3], where x, y, z are large, is as
// well scaled as any other); the cubics are homogeneous in c, and c c^T added to J^T J keeps the step across c.
// A step that is not finite, or that the 4 x 4 Cholesky cannot take, is not taken.
SIM3OPT_ESS_HD double ess_polish(const double* V, double c[4]) {
  double res = 0.0;  // |r|^2 before the last step
#pragma unroll 1
  for (int it = 0; it < POLISH; ++it) {
    double E[9], M[9], cof[9], r[10], J[4][10];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = c[0] * V[i] + c[1] * V[9 + i] + c[2] * V[18 + i] + c[3] * V[27 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) M[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
    const double tr = M[0] + M[4] + M[8];
    cof[0] = E[4] * E[8] - E[5] * E[7]; cof[1] = E[5] * E[6] - E[3] * E[8]; cof[2] = E[3] * E[7] - E[4] * E[6];
    cof[3] = E[7] * E[2] - E[8] * E[1]; cof[4] = E[8] * E[0] - E[6] * E[2]; cof[5] = E[6] * E[1] - E[7] * E[0];
    cof[6] = E[1] * E[5] - E[2] * E[4]; cof[7] = E[2] * E[3] - E[0] * E[5]; cof[8] = E[0] * E[4] - E[1] * E[3];
    r[0] = E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        r[1 + 3 * i + j] = 2.0 * (M[3 * i] * E[j] + M[3 * i + 1] * E[3 + j] + M[3 * i + 2] * E[6 + j]) - tr * E[3 * i + j];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const double* D = V + 9 * v;  // dE / dc_v
      double dM[9], dtr = 0.0, dd = 0.0;
#pragma unroll
      for (int i = 0; i < 9; ++i) { dd += cof[i] * D[i]; dtr += 2.0 * E[i] * D[i]; }
      J[v][0] = dd;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          dM[3 * i + j] = (D[3 * i] * E[3 * j] + D[3 * i + 1] * E[3 * j + 1] + D[3 * i + 2] * E[3 * j + 2]) +
                          (E[3 * i] * D[3 * j] + E[3 * i + 1] * D[3 * j + 1] + E[3 * i + 2] * D[3 * j + 2]);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          J[v][1 + 3 * i + j] = 2.0 * ((dM[3 * i] * E[j] + dM[3 * i + 1] * E[3 + j] + dM[3 * i + 2] * E[6 + j]) +
                                       (M[3 * i] * D[j] + M[3 * i + 1] * D[3 + j] + M[3 * i + 2] * D[6 + j])) -
                                dtr * E[3 * i + j] - tr * D[3 * i + j];
    }
    res = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k) res += r[k] * r[k];
    double H[4][4], g[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      g[a] = 0.0;
#pragma unroll
      for (int k = 0; k < 10; ++k) g[a] -= J[a][k] * r[k];
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        double h = c[a] * c[b];
#pragma unroll
        for (int k = 0; k < 10; ++k) h += J[a][k] * J[b][k];
        H[a][b] = h;
      }
    }
    // H = L L^T, then the two triangular solves
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        double h = H[a][b];
#pragma unroll
        for (int k = 0; k < b; ++k) h -= H[a][k] * H[b][k];
        if (a == b) { ok = ok && h > 0.0; H[a][a] = sqrt(h); } else H[a][b] = h / H[b][b];
      }
    }
    double y[4], d[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double h = g[a];
#pragma unroll
      for (int k = 0; k < a; ++k) h -= H[a][k] * y[k];
      y[a] = h / H[a][a];
    }
#pragma unroll
    for (int a = 3; a >= 0; --a) {
      double h = y[a];
#pragma unroll
      for (int k = a + 1; k < 4; ++k) h -= H[k][a] * d[k];
      d[a] = h / H[a][a];
    }
    double n[4], nn = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) { n[a] = c[a] + d[a]; nn += n[a] * n[a]; }
    const double inv = 1.0 / sqrt(nn);
    if (ok && std::isfinite(inv) && std::isfinite(nn)) {
#pragma unroll
      for (int a = 0; a < 4; ++a) c[a] = n[a] * inv;
    }
  }
  return res;
}

// The (k + 1)-th smallest real root: BISECTIONS halvings of the Cauchy interval on the chain's count, then NEWTON
// steps kept inside the last bracket; c ~ (x, y, z, 1) from the null vector of B(z); the polish; the sixth point's error of its E.
// All into the root's slot.  One lane's work.
SIM3OPT_ESS_HD void ess_root(double* ws, int k, const double q5[4]) {
  const double bound = ws[WS_META + 1];
  const int nr = (int)ws[WS_META + 2], at_minus = (int)ws[WS_META + 3];
  double e2 = -1.0, c[4] = {0.0, 0.0, 0.0, 0.0};
  if (k < nr) {
    double lo = -bound, hi = bound;
    for (int it = 0; it < BISECTIONS; ++it) {  // the root lies in (lo, hi]
      const double mid = 0.5 * (lo + hi);
      if (at_minus - sturm_changes(ws + WS_S, mid) >= k + 1) hi = mid; else lo = mid;
    }
    double z = 0.5 * (lo + hi);
    for (int it = 0; it < NEWTON; ++it) {
      double v = ws[WS_P + 10], dv = 0.0;
      for (int i = 9; i >= 0; --i) { dv = dv * z + v; v = v * z + ws[WS_P + i]; }
      const double zn = z - v / dv;
      if (std::isfinite(zn) && zn >= lo && zn <= hi) z = zn;
    }
    // (x, y, 1) spans the null space of B(z): the largest cross product of two of its rows
    double Bz[3][3], big = -1.0, nv[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      Bz[r][0] = poly_eval(ws + WS_B + 13 * r, 4, z);
      Bz[r][1] = poly_eval(ws + WS_B + 13 * r + 4, 4, z);
      Bz[r][2] = poly_eval(ws + WS_B + 13 * r + 8, 5, z);
    }
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {
      const int a = pair == 2 ? 1 : 0, b = pair == 0 ? 1 : 2;
      const double w0 = Bz[a][1] * Bz[b][2] - Bz[a][2] * Bz[b][1], w1 = Bz[a][2] * Bz[b][0] - Bz[a][0] * Bz[b][2],
                   w2 = Bz[a][0] * Bz[b][1] - Bz[a][1] * Bz[b][0];
      const double nn = w0 * w0 + w1 * w1 + w2 * w2;
      if (nn > big) { big = nn; nv[0] = w0; nv[1] = w1; nv[2] = w2; }
    }
    c[0] = nv[0]; c[1] = nv[1]; c[2] = z * nv[2]; c[3] = nv[2];
    const double inv = 1.0 / sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3]);
    double E[9];
    e2 = -2.0;
    if (std::isfinite(inv)) {
#pragma unroll
      for (int a = 0; a < 4; ++a) c[a] *= inv;
      // A solution with a small share of V[3] lies near this chart's infinity, where z = c2 / c3 says little and
      // the start may lie on the wrong side of it: when the polish has not arrived, it starts once more from there.
      double alt[4] = {c[0], c[1], -c[2], -c[3]};
      if (!(ess_polish(ws + WS_V, c) <= POLISH_DONE) && ess_polish(ws + WS_V, alt) <= POLISH_DONE) {
#pragma unroll
        for (int a = 0; a < 4; ++a) c[a] = alt[a];
      }
      if (ess_E_of_c(ws + WS_V, c, E)) {
        const double e = ess_sampson(E, q5[0], q5[1], q5[2], q5[3]);
        if (std::isfinite(e)) e2 = e;
      } else {
        e2 = -1.0;
      }
    } else {
      e2 = -1.0;
      c[0] = c[1] = c[2] = c[3] = 0.0;
    }
  }
  ws[WS_ROOT + 5 * k] = e2;
#pragma unroll
  for (int a = 0; a < 4; ++a) ws[WS_ROOT + 5 * k + 1 + a] = c[a];
}

// One hypothesis, by the lanes of group g together: q[0..4] = (x0, y0, x1, y1) make it, q[5] chooses among its
// solutions (the smallest Sampson error, the lower root on a tie).  n_solutions counts the real roots that give a
// finite E.  Returns whether there is one; E has Frobenius norm 1 then, and is zero otherwise: never a non-finite
// number; a repeated correspondence among the six makes it invalid (among the five through the null space's pivot,
// the sixth by comparison).  Every lane returns the same.  ws: WS_DOUBLES doubles shared by the group.
template <class Group>
SIM3OPT_ESS_HD bool ess_hypothesis(const Group& g, const double q[6][4], double* ws, double E[9], int& n_solutions) {
  n_solutions = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = 0.0;
  // a sixth correspondence equal to one of the five fits every solution and chooses nothing: a repeated point
  bool sixth_repeats = false;
#pragma unroll
  for (int k = 0; k < 5; ++k)
    sixth_repeats = sixth_repeats || (q[5][0] == q[k][0] && q[5][1] == q[k][1] && q[5][2] == q[k][2] && q[5][3] == q[k][3]);
  if (sixth_repeats) return false;
  if (g.leader()) {
    const bool ok = ess_nullspace(q, ws);
    ws[0] = ok ? 1.0 : 0.0;
  }
  g.sync();
  const bool have_basis = ws[0] != 0.0;
  g.sync();
  if (!have_basis) return false;
  for (int r = g.first(); r < 10; r += g.step()) ess_constraint_row(ws + WS_V, r, ws + WS_A + 20 * r);
  g.sync();
  for (int k = 0; k < 10; ++k) {
    double big;
    const int br = ess_pivot_row(ws + WS_A, k, big);
    g.sync();
    if (!(big > ELIM_PIVOT_MIN)) return false;
    if (g.leader()) ess_swap_scale(ws + WS_A, k, br);
    g.sync();
    for (int r = g.first(); r < 10; r += g.step()) ess_reduce_row(ws + WS_A, k, r);
    g.sync();
  }
  if (g.leader()) ess_polynomials(ws);
  g.sync();
  if (ws[WS_META] == 0.0) return false;
  for (int k = g.first(); k < 10; k += g.step()) ess_root(ws, k, q[5]);
  g.sync();
  double best = 0.0, cbest[4] = {0.0, 0.0, 0.0, 0.0};
  bool found = false;
  for (int k = 0; k < 10; ++k) {
    const double e2 = ws[WS_ROOT + 5 * k];
    if (e2 != -1.0) ++n_solutions;
    if (e2 >= 0.0 && (!found || e2 < best)) {
      found = true; best = e2;
#pragma unroll
      for (int a = 0; a < 4; ++a) cbest[a] = ws[WS_ROOT + 5 * k + 1 + a];
    }
  }
  if (found) found = ess_E_of_c(ws + WS_V, cbest, E);
  return found;
}

// The pose candidates of E = +-s [t]x R (s > 0), Horn's closed form: t, a unit vector, spans E's left null space -- the
// largest cross product of two columns of E, normalised, its component of largest magnitude (the first such) made
// positive; with ts = t sqrt(|E|_F^2 / 2):  Ra = (Cof(E) - [ts]x E) / |ts|^2, E = +s [t]x Ra, and
// Rb = (Cof(E) + [ts]x E) / |ts|^2, E = -s [t]x Rb.  Candidates, in the order of include/sim3opt.h:
// 0 (Ra, t), 1 (Rb, t), 2 (Ra, -t), 3 (Rb, -t).  False (R the identity, t zero) when E has no such null direction.
SIM3OPT_ESS_HD bool ess_candidates(const double E[9], double R[2][9], double t[3]) {
#pragma unroll
  for (int i = 0; i < 9; ++i) R[0][i] = R[1][i] = (i % 4 == 0) ? 1.0 : 0.0;
  t[0] = t[1] = t[2] = 0.0;
  double best = 0.0, tt[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int pair = 0; pair < 3; ++pair) {
    const int a = pair == 2 ? 1 : 0, b = pair == 0 ? 1 : 2;
    const double u[3] = {E[a], E[3 + a], E[6 + a]}, v[3] = {E[b], E[3 + b], E[6 + b]};
    const double w[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double nn = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (nn > best) { best = nn; tt[0] = w[0]; tt[1] = w[1]; tt[2] = w[2]; }
  }
  double f2 = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) f2 += E[i] * E[i];
  if (!(best > 0.0) || !std::isfinite(best) || !std::isfinite(f2)) return false;
  const double inv = 1.0 / sqrt(best);
  double sgn = 1.0, big = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    tt[i] *= inv;
    if (fabs(tt[i]) > big) { big = fabs(tt[i]); sgn = tt[i] < 0.0 ? -1.0 : 1.0; }
  }
  const double len2 = 0.5 * f2, len = sqrt(len2);
  double ts[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { tt[i] *= sgn; ts[i] = tt[i] * len; }
  const double* r0 = E;
  const double* r1 = E + 3;
  const double* r2 = E + 6;
  const double cof[9] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0],
                         r2[1] * r0[2] - r2[2] * r0[1], r2[2] * r0[0] - r2[0] * r0[2], r2[0] * r0[1] - r2[1] * r0[0],
                         r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
  double fin = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double txe[3] = {ts[1] * E[6 + j] - ts[2] * E[3 + j], ts[2] * E[j] - ts[0] * E[6 + j],
                           ts[0] * E[3 + j] - ts[1] * E[j]};  // column j of [ts]x E
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      R[0][3 * i + j] = (cof[3 * i + j] - txe[i]) / len2;
      R[1][3 * i + j] = (cof[3 * i + j] + txe[i]) / len2;
      fin += R[0][3 * i + j] + R[1][3 * i + j];
    }
  }
  if (!std::isfinite(fin)) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[0][i] = R[1][i] = (i % 4 == 0) ? 1.0 : 0.0;
    return false;
  }
  t[0] = tt[0]; t[1] = tt[1]; t[2] = tt[2];
  return true;
}

// The depths of a correspondence under X1 = R X0 + t: the least-squares solution of z0 R x0 - z1 x1 = -t (the 2 x 2
// normal equations).  Parallel rays give non-finite depths, which vote for nothing.
SIM3OPT_ESS_HD void ess_depths(const double R[9], const double t[3], double x0, double y0, double x1, double y1,
                               double& z0, double& z1) {
  const double a[3] = {R[0] * x0 + R[1] * y0 + R[2], R[3] * x0 + R[4] * y0 + R[5], R[6] * x0 + R[7] * y0 + R[8]};
  const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = x1 * x1 + y1 * y1 + 1.0;
  const double ab = a[0] * x1 + a[1] * y1 + a[2];
  const double at = a[0] * t[0] + a[1] * t[1] + a[2] * t[2], bt = x1 * t[0] + y1 * t[1] + t[2];
  const double det = aa * bb - ab * ab;
  z0 = (ab * bt - at * bb) / det;
  z1 = (aa * bt - ab * at) / det;
}

// whether the correspondence votes for (R, t): both depths positive and below distance_threshold
SIM3OPT_ESS_HD bool ess_votes(const double R[9], const double t[3], double x0, double y0, double x1, double y1,
                              double dist) {
  double z0, z1;
  ess_depths(R, t, x0, y0, x1, y1, z0, z1);
  return z0 > 0.0 && z1 > 0.0 && z0 < dist && z1 < dist;
}

// unit quaternion x y z w of a rotation matrix (row-major), w >= 0 branch first (Shepperd)
SIM3OPT_ESS_HD void ess_R_to_quat(const double R[9], double q[4]) {
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
  const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (nq > 0.0 && std::isfinite(nq)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] /= nq;
  } else {
    q[0] = q[1] = q[2] = 0.0; q[3] = 1.0;
  }
}

}  // namespace sim3opt_essential
