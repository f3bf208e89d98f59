// cov_kernels.hpp -- blocks of Z = (H + lambda I)^-1 OUTSIDE the pattern of the factor (sim3opt_covariances; included
// by direct_factor.hip after selinv_kernels.hpp).  Runs after k_ldl has factored (H + lambda I) = L L^T.
//
// With W = L^-1:  Z(i,j) = sum_k W(k,i)^T W(k,j).  Column j of W is non-zero only on the root path of j in the
// elimination tree (the parent of column m is its first below-diagonal row); along it, ascending,
//   acc(j) = I, every other acc = 0;   W(m,j) = L(m,m)^-1 acc(m);   acc(k) -= L(k,m) W(m,j) for every stored L(k,m),
// and every such row k lies on the path again.  So Z(i,j) sums over the common ancestors of i and j (either one
// included when it is an ancestor of the other); without one -- two trees of a forest -- the block is exactly zero.
//
//   k_cov_paths  one wavefront per requested vertex j: walks the root path and leaves W(.,j) as depth(j) + 1 blocks
//                in the workspace, W(path[t], j) at block voff + t.  The workspace holds acc(k) until k's turn comes:
//                path position of an ancestor k is depth(j) - depth(k), no search.  A dependent chain of at most the
//                tree's height; the requests are independent, the grid is the parallelism.
//   k_cov_pairs  one wavefront per requested pair: sum of W(k,a)^T W(k,b) over the common suffix of the two paths.
// Lane l holds entry l49 = l mod 49 of a column-major 7x7 block (lanes 49..63 mirror lanes 0..14: every lane issues
// a valid load; only lanes < 49 hand values on).  Operands are staged in the wavefront's slice of LDS behind
// wave_lds_sync and read back as broadcasts.  A lane re-reads from the workspace only what the same lane stored
// (entry l49 of a block, lanes < 49): program order of one thread, no fence needed.  No atomics, plain vector stores.
// The order of summation is the path's (ascending in EVERY schedule: a schedule is a topological order of the same
// tree), so the bits depend neither on the schedule nor on which other vertices or pairs share the launch.
#pragma once
// (included inside namespace sim3opt)

constexpr int COV_BATCH = 8;  // blocks whose operands a wavefront has in flight / in LDS at once
constexpr int COV_NW = 4;     // wavefronts per workgroup (WG = 256)

struct CovArgs {
  const int32_t* colptr;
  const int32_t* lrow;
  const double* L;       // nL x 49, the factor
  const double* Dinv;    // nb x 49, L(j,j)^-1
  const int32_t* depth;  // nb: proper ancestors of column j in the elimination tree
  int32_t nb;
  double* W;             // workspace, blocks of 49
  int32_t wblocks;       // its size in blocks (the kernels store nothing beyond)
};

// vcol[v]: column of requested vertex v; voff[v]: first workspace block of its path (depth + 1 blocks)
__global__ __launch_bounds__(WG) void k_cov_paths(CovArgs A, const int32_t* __restrict__ vcol,
                                                  const int32_t* __restrict__ voff, int32_t nv) {
  __shared__ double st_l[COV_NW][COV_BATCH][49];
  __shared__ double st_w[COV_NW][49];
  __shared__ double st_t[COV_NW][98];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int l49 = lane < 49 ? lane : lane - 49;
  const int r = l49 % 7, c = l49 / 7;
  const int v = blockIdx.x * COV_NW + wave;
  if (v >= nv) return;  // (wavefront-uniform; no workgroup barrier below)
  const int j = __builtin_amdgcn_readfirstlane(vcol[v]);
  const int off = __builtin_amdgcn_readfirstlane(voff[v]);
  if (j < 0 || j >= A.nb || off < 0) return;
  const int d = __builtin_amdgcn_readfirstlane(A.depth[j]);
  if (d < 0 || (long long)off + d + 1 > (long long)A.wblocks) return;  // (never: the host sized the workspace)
  double* base = A.W + (size_t)49 * off;
  // acc(j) = I, acc(ancestors) = 0
  for (int t = 0; t <= d; ++t)
    if (lane < 49) base[(size_t)49 * t + lane] = (t == 0 && r == c) ? 1.0 : 0.0;
  int m = j;
  for (int t = 0; t <= d; ++t) {
    const int s0 = __builtin_amdgcn_readfirstlane(A.colptr[m]), s1 = __builtin_amdgcn_readfirstlane(A.colptr[m + 1]);
    // W(m,j) = L(m,m)^-1 acc(m)
    const double av = base[(size_t)49 * t + l49];
    const double dv = A.Dinv[(size_t)49 * m + l49];
    if (lane < 49) { st_t[wave][lane] = dv; st_t[wave][49 + lane] = av; }
    wave_lds_sync();
    double w = 0.0;
#pragma unroll
    for (int q = 0; q < 7; ++q) w += st_t[wave][r + 7 * q] * st_t[wave][49 + q + 7 * c];
    if (lane < 49) { base[(size_t)49 * t + lane] = w; st_w[wave][lane] = w; }
    wave_lds_sync();
    // acc(k) -= L(k,m) W(m,j) over the column's stored rows k (all of them ancestors of m)
    for (int sb = s0 + 1; sb < s1; sb += COV_BATCH) {
      const int n = s1 - sb < COV_BATCH ? s1 - sb : COV_BATCH;
      int vk = 0;
      if (lane < n) vk = d - A.depth[A.lrow[sb + lane]];  // path position of row k
      double lv[COV_BATCH], cv[COV_BATCH];
      int tk[COV_BATCH];
#pragma unroll
      for (int i = 0; i < COV_BATCH; ++i)
        if (i < n) {
          tk[i] = __builtin_amdgcn_readlane(vk, i);
          if (tk[i] <= t || tk[i] > d) tk[i] = -1;  // (never: a stored row of a path column is on the path)
          lv[i] = A.L[(size_t)49 * (sb + i) + l49];
          cv[i] = tk[i] >= 0 ? base[(size_t)49 * tk[i] + l49] : 0.0;
        }
#pragma unroll
      for (int i = 0; i < COV_BATCH; ++i)
        if (i < n && lane < 49) st_l[wave][i][lane] = lv[i];
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < COV_BATCH; ++i)
        if (i < n) {
          double u = 0.0;
#pragma unroll
          for (int q = 0; q < 7; ++q) u += st_l[wave][i][r + 7 * q] * st_w[wave][q + 7 * c];
          if (tk[i] >= 0 && lane < 49) base[(size_t)49 * tk[i] + lane] = cv[i] - u;
        }
      wave_lds_sync();  // (everybody has read the round before the next one overwrites it)
    }
    if (s1 - s0 < 2) break;  // a root (t == d)
    m = __builtin_amdgcn_readfirstlane(A.lrow[s0 + 1]);
    if (m < 0 || m >= A.nb) break;
  }
}

// out[p] = sum over t < plen[p] of W[pa[p] + t]^T W[pb[p] + t], t ascending (pa / pb: workspace blocks where the
// common suffix of the two paths starts)
__global__ __launch_bounds__(WG) void k_cov_pairs(CovArgs A, const int32_t* __restrict__ pa,
                                                  const int32_t* __restrict__ pb, const int32_t* __restrict__ plen,
                                                  int32_t np, double* __restrict__ out) {
  __shared__ double st_a[COV_NW][COV_BATCH][49];
  __shared__ double st_b[COV_NW][COV_BATCH][49];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int l49 = lane < 49 ? lane : lane - 49;
  const int r = l49 % 7, c = l49 / 7;
  const int p = blockIdx.x * COV_NW + wave;
  if (p >= np) return;
  const int oa = __builtin_amdgcn_readfirstlane(pa[p]), ob = __builtin_amdgcn_readfirstlane(pb[p]);
  int len = __builtin_amdgcn_readfirstlane(plen[p]);
  if (oa < 0 || ob < 0 || (long long)oa + len > (long long)A.wblocks || (long long)ob + len > (long long)A.wblocks)
    len = 0;  // (never: the host sized the workspace)
  double acc = 0.0;
  for (int t0 = 0; t0 < len; t0 += COV_BATCH) {
    const int n = len - t0 < COV_BATCH ? len - t0 : COV_BATCH;
    double av[COV_BATCH], bv[COV_BATCH];
#pragma unroll
    for (int i = 0; i < COV_BATCH; ++i)
      if (i < n) {
        av[i] = A.W[(size_t)49 * (oa + t0 + i) + l49];
        bv[i] = A.W[(size_t)49 * (ob + t0 + i) + l49];
      }
#pragma unroll
    for (int i = 0; i < COV_BATCH; ++i)
      if (i < n && lane < 49) { st_a[wave][i][lane] = av[i]; st_b[wave][i][lane] = bv[i]; }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < COV_BATCH; ++i)
      if (i < n) {
#pragma unroll
        for (int q = 0; q < 7; ++q) acc += st_a[wave][i][q + 7 * r] * st_b[wave][i][q + 7 * c];
      }
    wave_lds_sync();
  }
  if (lane < 49) out[(size_t)49 * p + lane] = acc;
}
