// selinv_kernels.hpp -- device side of the block selected inversion (g2o's computeMarginals; included by
// direct_factor.hip after direct_kernels.hpp; lists from selinv.cpp, maths there).  Runs after k_ldl has
// factored (H + lambda I) = L L^T (its UP path) into the marginal context's own buffers.
//
// One workgroup owns one group of the factor's schedule and walks its levels TOP-DOWN: the top group in
// one launch, then every bottom group in a second launch (the kernel boundary makes the top group's blocks
// of Z visible to all of them).  A level is two phases with a workgroup barrier between: the off-diagonal
// blocks of its columns (reading only blocks of Z of ancestors, done in earlier levels or launches), then
// the diagonal blocks (reading the off-diagonal blocks of their own column).  A wavefront computes one
// target block at a time, blocks of a phase dealt out round-robin (within a column every block has |S_j|
// products, so the blocks of a phase cost about the same).
// Lane l holds entry l49 = l mod 49 of a column-major 7x7 block (lanes 49..63 mirror lanes 0..14: every lane
// issues a valid load).  The operands of a round of up to SEL_BATCH products are loaded together (one
// memory round trip), staged in the wavefront's slice of LDS and read back as broadcasts: entry (r, c) of
// op(Z) L is row r of the one block times column c of the other.  Lanes hand values over through LDS only
// behind wave_lds_sync (dev_common.hpp).  No atomics; every block sums its products in the plan's order
// with the same instructions under every schedule: bit-reproducible.
#pragma once
// (included inside namespace sim3opt)

constexpr int SEL_BATCH = 8;  // products whose operands a wavefront has in flight / in LDS at once

struct SelArgs {
  const int32_t* colptr;
  const int32_t* lrow;
  const int32_t* lcol;
  const int32_t* gptr;
  const int32_t* lcolp;
  const int32_t* zptr;
  const int32_t* za;
  const int32_t* zt;
  const int32_t* zl;
  const double* L;     // nL x 49, the factor
  const double* Dinv;  // nb x 49, L(j,j)^-1
  double* Z;           // nL x 49, the result
  int32_t nb;
  const unsigned long long* maxdiag_bits;  // the linearisation's max |H_dd|, as raw bits (read only)
  int32_t* singular;  // set by k_selinv_pivots (k_ldl flags a non-positive pivot in its own fail word)
};

// The 7x7 Cholesky of k_ldl flags a non-positive pivot only.  A singular H (no fixed vertex: the gauge
// directions) leaves pivots of the size of the rounding errors, of either sign; a positive one would turn
// into a covariance of 1e15 and more.  So a pivot below SEL_PIVOT_REL max |H_dd| counts as singular too:
// that is cond(H + lambda I) beyond ~1e13, where no double-precision inverse means anything.
constexpr double SEL_PIVOT_REL = 1e-13;
__global__ __launch_bounds__(WG) void k_selinv_pivots(SelArgs S) {
  const int t = blockIdx.x * WG + threadIdx.x;
  if (t >= 7 * S.nb) return;
  const int j = t / 7, r = t % 7;
  double maxdiag;
  const unsigned long long bits = *S.maxdiag_bits;
  __builtin_memcpy(&maxdiag, &bits, sizeof(double));
  const double l = S.L[(size_t)49 * S.colptr[j] + 8 * r];
  if (!(l * l > SEL_PIVOT_REL * maxdiag)) *S.singular = 1;  // (the same value from every writer)
}

// block s of Z (diag: the diagonal block of column j); `stz` / `stl` / `stt` are this wavefront's LDS
__device__ __forceinline__ void selinv_block(const SelArgs& S, int s, int j, bool diag, int lane, int l49,
                                             int r, int c, double (*stz)[49], double (*stl)[49],
                                             double* stt) {
  const int k0 = S.zptr[s], k1 = S.zptr[s + 1];
  double acc = 0.0;  // entry (r, c) of sum_k op(Z) L(k,j)
  for (int p0 = k0; p0 < k1; p0 += SEL_BATCH) {
    const int n = k1 - p0 < SEL_BATCH ? k1 - p0 : SEL_BATCH;
    int va = 0, vt = 0, vl = 0;
    if (lane < n) { va = S.za[p0 + lane]; vt = S.zt[p0 + lane]; vl = S.zl[p0 + lane]; }
    double zv[SEL_BATCH], lv[SEL_BATCH];
#pragma unroll
    for (int i = 0; i < SEL_BATCH; ++i)
      if (i < n) {
        const int zi = __builtin_amdgcn_readlane(va, i), ti = __builtin_amdgcn_readlane(vt, i);
        // op(Z) entry (r, c): Z(r, c), or Z(c, r) for a transposed operand
        zv[i] = S.Z[(size_t)49 * zi + (ti ? c + 7 * r : l49)];
        lv[i] = S.L[(size_t)49 * __builtin_amdgcn_readlane(vl, i) + l49];
      }
#pragma unroll
    for (int i = 0; i < SEL_BATCH; ++i)
      if (i < n && lane < 49) { stz[i][lane] = zv[i]; stl[i][lane] = lv[i]; }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < SEL_BATCH; ++i)
      if (i < n) {
#pragma unroll
        for (int m = 0; m < 7; ++m) acc += stz[i][r + 7 * m] * stl[i][m + 7 * c];
      }
    wave_lds_sync();  // (everybody has read the round before the next one overwrites it)
  }
  // Z = (Z0 - acc) L(j,j)^-1, Z0 = L(j,j)^-T on the diagonal
  const double* di = S.Dinv + (size_t)49 * j;
  const double t = (diag ? di[c + 7 * r] : 0.0) - acc;
  if (lane < 49) { stt[lane] = t; stt[49 + lane] = di[l49]; }
  wave_lds_sync();
  double z = 0.0;
#pragma unroll
  for (int m = 0; m < 7; ++m) z += stt[r + 7 * m] * stt[49 + m + 7 * c];
  if (diag) {  // the lower triangle, mirrored: exactly symmetric
    wave_lds_sync();
    if (lane < 49) stt[lane] = z;
    wave_lds_sync();
    if (r < c) z = stt[c + 7 * r];
  }
  if (lane < 49) S.Z[(size_t)49 * s + lane] = z;
  wave_lds_sync();  // (stt is reused by this wavefront's next block)
}

__global__ __launch_bounds__(LDL_WG_TOP) void k_selinv(SelArgs S, int g0) {
  __shared__ double st_z[LDL_NW][SEL_BATCH][49];
  __shared__ double st_l[LDL_NW][SEL_BATCH][49];
  __shared__ double st_t[LDL_NW][98];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nw = blockDim.x >> 6;
  const int l49 = lane < 49 ? lane : lane - 49;
  const int r = l49 % 7, c = l49 / 7;
  const int g = g0 + blockIdx.x;
  const int lv0 = S.gptr[g], lv1 = S.gptr[g + 1];
  for (int l = lv1 - 1; l >= lv0; --l) {
    const int c0 = S.lcolp[l], c1 = S.lcolp[l + 1];
    const int s0 = S.colptr[c0], s1 = S.colptr[c1];
    // phase 1: off-diagonal blocks of the level's columns (the diagonal ones are skipped in the deal)
    for (int s = s0 + wave; s < s1; s += nw) {
      const int j = __builtin_amdgcn_readfirstlane(S.lcol[s]);
      if (__builtin_amdgcn_readfirstlane(S.lrow[s]) == j) continue;
      selinv_block(S, s, j, false, lane, l49, r, c, st_z[wave], st_l[wave], st_t[wave]);
    }
    __syncthreads();
    // phase 2: diagonal blocks (they read their column's off-diagonal blocks)
    for (int j = c0 + wave; j < c1; j += nw)
      selinv_block(S, __builtin_amdgcn_readfirstlane(S.colptr[j]), j, true, lane, l49, r, c, st_z[wave],
                   st_l[wave], st_t[wave]);
    __syncthreads();
  }
}

// out[q] = Z(a, b) for the requested pairs: block slot[q] of Z, transposed where trans[q]
__global__ __launch_bounds__(WG) void k_selinv_pick(const double* Z, const int32_t* slot, const int32_t* trans,
                                                    int32_t n, double* out) {
  const int t = blockIdx.x * WG + threadIdx.x;
  if (t >= 49 * n) return;
  const int q = t / 49, e = t % 49, r = e % 7, c = e / 7;
  out[t] = Z[(size_t)49 * slot[q] + (trans[q] ? c + 7 * r : e)];
}
