// col_kernels.hpp -- the vector kernels of the blocks of (H + lambda I)^-1 by columns (included by engine_columns.hip
// only, inside namespace sim3opt): SparseOptimizer::computeMarginals on graphs too large to factor.  A column of the
// inverse is the solution for a unit right-hand side; these kernels build K of them, form the true residual of a
// solution, add a refinement step and pick the requested 7x7 blocks out of the solutions.  Streaming FP64, wave64,
// 16 bytes per lane where the length allows, grid-stride under MAX_GRID workgroups, plain vector stores, no atomics.
// Vectors of system s live at base + s * vs; vs is a multiple of 64 doubles, so every system's base is 16-byte aligned.
#pragma once

struct ColUnits {
  int64_t at[KB];  // index of the unit entry of system s (7 row + column), < 0: none (the vector stays zero)
};

// g_s = e_{at[s]}, s < K: clears the K vectors and sets their unit entries
template <int K>
__global__ __launch_bounds__(WG) void k_cols_rhs(int64_t n, int64_t vs, double* __restrict__ g, ColUnits u) {
  const int64_t n2 = n / 2;
  const int64_t step = (int64_t)gridDim.x * WG;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    double2* g2 = reinterpret_cast<double2*>(g + (size_t)s * vs);
    const int64_t at = u.at[s];
    for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n2; i += step) {
      double2 v = make_double2(0.0, 0.0);
      if (2 * i == at) v.x = 1.0;
      if (2 * i + 1 == at) v.y = 1.0;
      g2[i] = v;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) g[(size_t)s * vs + n - 1] = at == n - 1 ? 1.0 : 0.0;
  }
}

// r = g - q: the true residual of a solution y from q = (H + lambda I) y (the SpMV wrote q)
__global__ __launch_bounds__(WG) void k_cols_residual(int64_t n, const double* __restrict__ g, const double* __restrict__ q,
                                                      double* __restrict__ r) {
  const int64_t n2 = n / 2;
  const int64_t step = (int64_t)gridDim.x * WG;
  const double2* g2 = reinterpret_cast<const double2*>(g);
  const double2* q2 = reinterpret_cast<const double2*>(q);
  double2* r2 = reinterpret_cast<double2*>(r);
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n2; i += step) {
    const double2 a = g2[i], b = q2[i];
    r2[i] = make_double2(a.x - b.x, a.y - b.y);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) r[n - 1] = g[n - 1] - q[n - 1];
}

// y += d: the refinement step (d solves the system for the residual of y)
__global__ __launch_bounds__(WG) void k_cols_axpy(int64_t n, const double* __restrict__ d, double* __restrict__ y) {
  const int64_t n2 = n / 2;
  const int64_t step = (int64_t)gridDim.x * WG;
  const double2* d2 = reinterpret_cast<const double2*>(d);
  double2* y2 = reinterpret_cast<double2*>(y);
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n2; i += step) {
    const double2 a = y2[i], b = d2[i];
    y2[i] = make_double2(a.x + b.x, a.y + b.y);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) y[n - 1] += d[n - 1];
}

// The blocks a solved column contributes to: y is column `col` of the vertex whose blocks are numbered
// [first, first + count): block k of them is (rows[k], that vertex), stored column-major, so its column `col` is
// y[7 rows[k] .. + 7).  One lane per entry; consecutive lanes read seven consecutive doubles of y and write seven
// consecutive doubles of the output.
__global__ __launch_bounds__(WG) void k_cols_gather(int32_t first, int32_t count, int32_t col,
                                                    const int32_t* __restrict__ rows, const double* __restrict__ y,
                                                    double* __restrict__ blocks) {
  const int64_t total = (int64_t)7 * count;
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < total; i += (int64_t)gridDim.x * WG) {
    const int32_t k = first + (int32_t)(i / 7), r = (int32_t)(i % 7);
    blocks[(size_t)49 * k + 7 * col + r] = y[(size_t)7 * rows[k] + r];
  }
}
