// gate_kernels.hpp -- the chi-square gate of candidate edges that are not in the graph (sim3opt_gate_edges; included
// by engine_direct.hip inside namespace sim3opt).  Per candidate (v0, v1, C, Omega):
//   e  = log(C S0 S1^-1) at the current estimates                         (sim3::edge_error, as k_edge_errors)
//   J  = [J0 | J1], update S <- exp(d) S: closed form (options.jacobians = 1: sim3::edge_jacobian_column, as
//        k_edge_jacobians) or central differences with fd_delta (mode 0: the residual function on exp(+-delta e_d) S,
//        the quotient k_linearize_numeric forms); dof_mask zeroes the frozen columns
//   S  = J Sigma J^T + Omega^-1,  Sigma = [[S00, S01], [S01^T, S11]] the joint covariance of the two endpoints
//        (blocks of (H + lambda I)^-1; zero for a fixed endpoint), lower triangle computed, mirrored
//   d2 = e^T S^-1 e by a 7x7 Cholesky (chi-square with 7 degrees of freedom under the linearised Gaussian model)
// One lane per candidate: a gate is a handful of candidates, the work is in the covariance blocks.
#pragma once

struct GateArgs {
  int32_t n;
  const int32_t* v0;      // vertex indices (into states)
  const int32_t* v1;
  const Sim3* meas;
  const double* sigma;    // n x 3 x 49 column-major: S00, S01 (rows v0's tangent, cols v1's), S11
  const double* infoinv;  // n x 49 column-major: Omega^-1
  const Sim3* states;
  sim3::Opts opts;
  int32_t analytic;       // options.jacobians
  int32_t dof_mask;
  double delta;           // options.fd_delta
  double* e_out;          // n x 7
  double* S_out;          // n x 49 column-major
  double* d2_out;         // n (NaN: S not positive definite)
};

__global__ __launch_bounds__(WG) void k_gate_edges(GateArgs A) {
  const int k = blockIdx.x * WG + threadIdx.x;
  if (k >= A.n) return;
  const Sim3 C = load_sim3(A.meas + k);
  const Sim3 S0 = load_sim3(A.states + A.v0[k]);
  const Sim3 S1 = load_sim3(A.states + A.v1[k]);
  double e[7], J[7][14];
  sim3::edge_error(C, S0, S1, A.opts, e);
  if (A.analytic) {
    double M[sim3::JAC_SUMS], X[13];
    sim3::left_jacobian_blocks(e, M);
    sim3::exp_of_residual(e, X);
    for (int c = 0; c < 14; ++c) {
      double col[7];
      sim3::edge_jacobian_column(M, X, C, c, A.dof_mask, col);
#pragma unroll
      for (int r = 0; r < 7; ++r) J[r][c] = col[r];
    }
  } else {
    const double scalar = 1.0 / (2.0 * A.delta);
    for (int c = 0; c < 14; ++c) {
      const int d = c < 7 ? c : c - 7;
      double xi[7], ep[7], em[7];
#pragma unroll
      for (int i = 0; i < 7; ++i) xi[i] = i == d ? A.delta : 0.0;
      const Sim3 Pp = sim3::exp(xi, A.opts);
      xi[d] = -A.delta;
      const Sim3 Pm = sim3::exp(xi, A.opts);
      if (c < 7) {
        sim3::edge_error(C, sim3::mul(Pp, S0), S1, A.opts, ep);
        sim3::edge_error(C, sim3::mul(Pm, S0), S1, A.opts, em);
      } else {
        sim3::edge_error(C, S0, sim3::mul(Pp, S1), A.opts, ep);
        sim3::edge_error(C, S0, sim3::mul(Pm, S1), A.opts, em);
      }
      const bool on = (A.dof_mask >> d) & 1;
#pragma unroll
      for (int r = 0; r < 7; ++r) J[r][c] = on ? scalar * (ep[r] - em[r]) : 0.0;
    }
  }
  // T = J Sigma (7 x 14)
  const double* S00 = A.sigma + (size_t)147 * k;
  const double* S01 = S00 + 49;
  const double* S11 = S00 + 98;
  double T[7][14];
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 14; ++c) {
      double acc = 0.0;
      for (int q = 0; q < 14; ++q) {
        // Sigma(q, c), blocks column-major; the lower-left block is S01^T
        double s;
        if (q < 7) s = c < 7 ? S00[q + 7 * c] : S01[q + 7 * (c - 7)];
        else s = c < 7 ? S01[c + 7 * (q - 7)] : S11[(q - 7) + 7 * (c - 7)];
        acc += J[r][q] * s;
      }
      T[r][c] = acc;
    }
  // S = T J^T + Omega^-1: lower triangle, mirrored
  const double* Oi = A.infoinv + (size_t)49 * k;
  double Sm[7][7];
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c <= r; ++c) {
      double acc = 0.0;
      for (int q = 0; q < 14; ++q) acc += T[r][q] * J[c][q];
      acc += Oi[r + 7 * c];
      Sm[r][c] = acc;
      Sm[c][r] = acc;
    }
  // d2 = |L^-1 e|^2, S = L L^T
  double Lc[7][7], y[7];
  bool ok = true;
  for (int j = 0; j < 7; ++j) {
    double d = Sm[j][j];
    for (int q = 0; q < j; ++q) d -= Lc[j][q] * Lc[j][q];
    if (!(d > 0.0) || !(d < DBL_MAX)) { ok = false; d = 1.0; }
    const double ljj = sqrt(d);
    Lc[j][j] = ljj;
    for (int r = j + 1; r < 7; ++r) {
      double v = Sm[r][j];
      for (int q = 0; q < j; ++q) v -= Lc[r][q] * Lc[j][q];
      Lc[r][j] = v / ljj;
    }
  }
  double d2 = 0.0;
  for (int r = 0; r < 7; ++r) {
    double v = e[r];
    for (int q = 0; q < r; ++q) v -= Lc[r][q] * y[q];
    y[r] = v / Lc[r][r];
    d2 += y[r] * y[r];
  }
  for (int r = 0; r < 7; ++r) A.e_out[(size_t)7 * k + r] = e[r];
  for (int c = 0; c < 7; ++c)
    for (int r = 0; r < 7; ++r) A.S_out[(size_t)49 * k + r + 7 * c] = Sm[r][c];
  A.d2_out[k] = ok ? d2 : __builtin_nan("");
}
