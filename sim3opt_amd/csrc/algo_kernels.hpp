// algo_kernels.hpp -- device side of the Gauss-Newton and dogleg algorithms (included by engine_algorithms.hip ONLY,
// inside namespace sim3opt): the fused per-iteration dots of the dogleg model and the dogleg update.  Reductions
// are fixed-order (per-workgroup partials, one final sum), like k_scale / k_final_sum_two.
#pragma once

// slots of the dogleg scalars, after the 4 x MAX_GRID partials in Engine::d_dl
enum DlSlot { DL_BB = 0, DL_BHB, DL_GG, DL_BG, DL_HBG, DL_GHG, DL_OUT = 8 };

// over j in [j0, j1): b.b, g.g, b.g and (Hb).g, one partial of each per workgroup (part[k * MAX_GRID + block])
__global__ __launch_bounds__(WG) void k_dl_dots(int j0, int j1, const double* __restrict__ b,
                                                const double* __restrict__ g, const double* __restrict__ hb,
                                                double* __restrict__ part) {
  __shared__ double sh[4];
  double bb = 0.0, gg = 0.0, bg = 0.0, hg = 0.0;
  for (int j = j0 + blockIdx.x * WG + threadIdx.x; j < j1; j += gridDim.x * WG) {
    const double bj = b[j], gj = g[j];
    bb += bj * bj;
    gg += gj * gj;
    bg += bj * gj;
    hg += hb[j] * gj;
  }
  const double s0 = block_sum(bb, sh);
  const double s1 = block_sum(gg, sh);
  const double s2 = block_sum(bg, sh);
  const double s3 = block_sum(hg, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s0;
    part[MAX_GRID + blockIdx.x] = s1;
    part[2 * MAX_GRID + blockIdx.x] = s2;
    part[3 * MAX_GRID + blockIdx.x] = s3;
  }
}

// one sum of n partials into *out (the SpMV's v.q partials: b^T H b)
__global__ __launch_bounds__(WG) void k_dl_sum(const double* __restrict__ p, int n, double* __restrict__ out) {
  __shared__ double sh[4];
  const double s = sum_partials(p, n, sh);
  if (threadIdx.x == 0) *out = s;
}

// the four dot partials (nd per dot) and the second SpMV's v.q partials (ns: h_gn^T H h_gn) into out[DL_*]
__global__ __launch_bounds__(WG) void k_dl_final(const double* __restrict__ part, int nd,
                                                 const double* __restrict__ spmv_part, int ns,
                                                 double* __restrict__ out) {
  __shared__ double sh[4];
  const double bb = sum_partials(part, nd, sh);
  const double gg = sum_partials(part + MAX_GRID, nd, sh);
  const double bg = sum_partials(part + 2 * MAX_GRID, nd, sh);
  const double hg = sum_partials(part + 3 * MAX_GRID, nd, sh);
  const double gh = sum_partials(spmv_part, ns, sh);
  if (threadIdx.x == 0) {
    out[DL_BB] = bb;
    out[DL_GG] = gg;
    out[DL_BG] = bg;
    out[DL_HBG] = hg;
    out[DL_GHG] = gh;
  }
}

// One dogleg trial's update: for every free vertex h = ca b + cg h_gn (its 7 entries), backup <- S (push),
// S <- exp(h) S (VertexSim3Expmap::oplusImpl).  sc != nullptr: the exact factorisation's verdict -- a solve that
// met a non-positive pivot (sc->fail == fail_token) leaves the estimates alone (the host never gets here then; the
// test keeps the kernel safe on its own, as k_oplus is).
__global__ __launch_bounds__(WG) void k_dogleg_oplus(int nv, const int32_t* __restrict__ hidx,
                                                     const double* __restrict__ b, const double* __restrict__ g,
                                                     double ca, double cg, Sim3* states, sim3::Opts opts,
                                                     const DevScalars* sc, Sim3* __restrict__ backup,
                                                     int fail_token) {
  const int v = blockIdx.x * WG + threadIdx.x;
  if (v >= nv) return;
  const double* s8 = reinterpret_cast<const double*>(states + v);
  double* b8 = reinterpret_cast<double*>(backup + v);
#pragma unroll
  for (int i = 0; i < 8; ++i) b8[i] = s8[i];
  if (sc && sc->fail == fail_token) return;
  const int h = hidx[v];
  if (h < 0) return;
  double xi[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) xi[i] = ca * b[(size_t)7 * h + i] + cg * g[(size_t)7 * h + i];
  const Sim3 P = sim3::exp(xi, opts);
  const Sim3 S = sim3::mul(P, load_sim3(states + v));
  double* d = reinterpret_cast<double*>(states + v);
  d[0] = S.q[0]; d[1] = S.q[1]; d[2] = S.q[2]; d[3] = S.q[3];
  d[4] = S.t[0]; d[5] = S.t[1]; d[6] = S.t[2]; d[7] = S.s;
}
