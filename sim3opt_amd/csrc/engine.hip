// engine.hip -- initialisation, linearisation, chi2, the iteration frame and the LM trial loop (g2o: SparseOptimizer::
// optimize -> OptimizationAlgorithmLevenberg::solve, kitti_surf.cpp:674-675); the C++ interface capi.cpp calls
#include "engine_impl.hpp"
#include "handle_device.hpp"
#include "lm_damping.hpp"
#include "robust.hpp"
#include "sim3_jac.hpp"

namespace sim3opt {

#include "lm_kernels.hpp"

EdgeArgs Engine::edge_args() const {
  return EdgeArgs{e_lo, e_hi, d_ev0, d_ev1, d_meas, has_info ? d_info : nullptr,
                  has_kernel ? d_kdelta : nullptr, has_kernel ? d_kkind : nullptr, d_states, mopts()};
}

void Engine::release() {
  // (the calling thread's current device may be another one by now: a second graph on another device,
  // a rank thread's parent -- the pools of devmem.cpp key on the creating device, the runtime calls
  // below on the current one)
  int dev_prev = -1;
  if (device_used >= 0 && hipGetDevice(&dev_prev) == hipSuccess && dev_prev != device_used)
    (void)hipSetDevice(device_used);
  else
    dev_prev = -1;
  release_under_device();
  if (dev_prev >= 0) (void)hipSetDevice(dev_prev);
}

void Engine::release_under_device() {
  // cached blocks are handed out again without the device-wide wait a hipFree implies
  if (stream) (void)hipStreamSynchronize(stream);
  mem.release();
  ranged.clear();
  d_vals = d_scratch = nullptr;
  parts.clear();
  n_sharded = 0;
  batch_release();
  cols_release();
  lm_factor.release();
  marg_factor.release();
  staged.release();
  if (h_sc) host_free(h_sc);
  if (h_ring) host_free(h_ring);
  h_ring = nullptr;
  if (ring_ev) event_release(ring_ev);
  ring_ev = nullptr;
  if (h_dl) host_free(h_dl);
  for (hipEvent_t e : pool) event_release(e);
  for (hipEvent_t e : rep_pool) event_release(e);
  rep_pool.clear();
  if (ev_a) event_release(ev_a);
  if (ev_b) event_release(ev_b);
  for (hipEvent_t& e : ev_ph) if (e) { event_release(e); e = nullptr; }
  if (pcg_graph) (void)hipGraphExecDestroy(pcg_graph);
  if (stream) stream_release(stream);  // (synchronised above; kept for the next engine on this device)
  comm.release();
}

int Engine::init(const HostGraph& g, const Structure& s, std::string& err) {
  if (int rc = select_device(opt.device, err)) return rc;
  HIPCHK(hipGetDevice(&device_used));
  if (const char* ev = std::getenv("SIM3OPT_SPMV")) {
    int a = 0, b = 0;
    if (std::sscanf(ev, "%d,%d", &a, &b) == 2) { spmv_chunk = a; spmv_nt = b; }
  }
  HIPCHK(stream_acquire(&stream));
  phase_timing = opt.time_kernels != 0 || opt.verbose != 0 || s.nb > 4096;
  st = s;
  nv = g.nv(); ne = g.ne(); nb = s.nb; n = 7 * nb; nnzb = s.nnzb;
  // row partition (world == 1: everything is local)
  row_begin.assign(comm.world + 1, 0);
  partition_rows_equal(nb, comm.world, row_begin.data());
  r0 = row_begin[comm.rank];
  r1 = row_begin[comm.rank + 1];
  offs.resize(comm.world + 1);
  for (int r = 0; r <= comm.world; ++r) offs[r] = 7 * (int64_t)row_begin[r];
  if (comm.active()) {
    parts.assign(1, LevelPart());
    n_sharded = 1;
    int rc = level_part_init(0, nb, s.rowptr.data(), s.colidx.data(), row_begin, err);
    if (rc) return rc;
  }
  e_lo = (int32_t)((int64_t)ne * comm.rank / comm.world);
  e_hi = (int32_t)((int64_t)ne * (comm.rank + 1) / comm.world);
  // this rank linearises the edges incident to its rows and writes only its rows' blocks
  std::vector<int32_t> l_active, l_s01 = s.slot01, l_s10 = s.slot10, l_i0 = s.inc0, l_i1 = s.inc1;
  if (comm.world > 1) {
    for (int32_t k : s.active) {
      const int32_t a = s.hidx[g.ev0[k]], b = s.hidx[g.ev1[k]];
      const bool la = a >= r0 && a < r1, lb = b >= r0 && b < r1;
      if (!la) { l_s01[k] = -1; l_i0[k] = -1; }
      if (!lb) { l_s10[k] = -1; l_i1[k] = -1; }
      if (la || lb) l_active.push_back(k);
    }
  } else {
    l_active = s.active;
  }
  n_active = (int32_t)l_active.size();
  has_info = g.has_info;
  has_kernel = g.has_kernel;
  const bool itrace = std::getenv("SIM3OPT_INIT_TRACE") != nullptr;
  auto inow = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double it0 = inow();
  HIPCHK(event_acquire(&ev_a));
  HIPCHK(event_acquire(&ev_b));
  for (hipEvent_t& e : ev_ph) HIPCHK(event_acquire(&e));
  HIPCHK(upload(d_states, g.states));
  HIPCHK(mem.raw(d_backup, (size_t)nv));
  HIPCHK(upload(d_meas, g.meas));
  HIPCHK(upload(d_ev0, g.ev0));
  HIPCHK(upload(d_ev1, g.ev1));
  HIPCHK(upload(d_hidx, s.hidx));
  HIPCHK(upload(d_active, l_active));
  if (has_info) HIPCHK(upload(d_info, g.info));
  if (has_kernel) HIPCHK(upload(d_kdelta, g.kdelta));
  if (has_kernel) HIPCHK(upload(d_kkind, g.kkind));
  HIPCHK(upload(d_rowptr, s.rowptr));
  HIPCHK(upload(d_colidx, s.colidx));
  HIPCHK(upload(d_incptr, s.incptr));
  {  // span SpMV: contiguous row span per wavefront, balanced by stored blocks
    const int nloc = r1 - r0;
    // 3x the resident set (256 CUs x 8 workgroups of 4 wavefronts): shorter spans make the
    // addresses in flight a window that moves through the matrix instead of 8192 streams spread
    // over all of it (measured: 2048 -> 0.172 ms, 4096 -> 0.164, 6144 -> 0.1626, 8192 -> 0.1627,
    // 16384 -> 0.179 on config 3); small systems get one block row per wavefront
    // rule: ~4 block rows per wavefront (16 per workgroup), but never fewer workgroups than the
    // resident set as long as every wavefront still gets a row
    span_grid = std::max(std::min(2048, (nloc + 3) / 4), (nloc + 15) / 16);
    // tuning knob (options.span_grid; SIM3OPT_SPAN_GRID reaches it through sim3opt_initialize)
    if (opt.span_grid > 0) span_grid = std::min(opt.span_grid, (nloc + 3) / 4);
    span_grid = std::max(8, std::min(SPAN_GRID_MAX, span_grid));
    const int nw = span_grid * 4;
    std::vector<int32_t> wrow(nw + 1);
    partition_rows(nloc, s.rowptr.data() + r0, nw, wrow.data());
    for (int32_t& w : wrow) w += r0;
    HIPCHK(upload(d_wrow, wrow));
  }
  HIPCHK(upload(d_slot01, l_s01));
  HIPCHK(upload(d_slot10, l_s10));
  HIPCHK(upload(d_inc0, l_i0));
  HIPCHK(upload(d_inc1, l_i1));
  // H and the assembly scratch: this rank's rows only (alloc_ranged; one rank: everything)
  {
    int rc = alloc_ranged(d_vals, 49 * (int64_t)s.rowptr[r0], 49 * (int64_t)s.rowptr[r1], 49 * (int64_t)nnzb, err);
    if (rc) return rc;
    rc = alloc_ranged(d_scratch, 35 * (int64_t)s.incptr[r0], 35 * (int64_t)s.incptr[r1], 35 * (int64_t)s.incptr[nb], err);
    if (rc) return rc;
  }
  HIPCHK(mem.raw(d_Minv, 49 * (size_t)nb));
  // preconditioner choice: chain segments for chain-like graphs (few blocks per row)
  // automatic: chain segments only when almost every edge is a chain link (KITTI with one loop:
  // 3963 PCG iterations per 30 LM iterations instead of 621642); with many loops the low-rank
  // argument is gone and the sequential apply costs more than it saves (measured)
  int64_t chain_links = 0;
  for (int32_t i = 1; i < nb; ++i)
    for (int32_t k = s.rowptr[i] + 1; k < s.rowptr[i + 1]; ++k)
      if (s.colidx[k] == i - 1) { ++chain_links; break; }
  const int64_t off_chain_edges = (nnzb - nb) / 2 - chain_links;
  // Automatic choice: the exact factorisation where it is cheap (KITTI-00, chain-like graphs); else
  // the multigrid hierarchy whenever the graph coarsens like a low-dimensional one (level-1 blocks
  // <= 0.3 x level-0 blocks: chains, Manhattan worlds -- not expanders such as config 2, where
  // block-Jacobi converges in tens of iterations) -- in either arithmetic (round 3: with the
  // coefficient as written the hierarchy sets up without a failing pivot on config 3 and every solve
  // converges, 11 ... 690 iterations, where block-Jacobi stops at its 1000-iteration cap from the
  // sixth LM iteration on; scripts/gpu_refarith_amg.py); graphs too small for a hierarchy
  // (<= 256 rows) get chain segments if they are nearly pure chains -- in the well-posed arithmetic
  // only: as written cond(H + lambda I) reaches 1e12 on a chain and the recursive residual of so
  // strongly preconditioned a CG drifts from the true one --; block-Jacobi otherwise.
  // (naming a preconditioner asks for the PCG)
  const double it1 = inow();
  if (opt.linear_solver == 1 || (opt.linear_solver < 0 && opt.preconditioner < 0)) {
    int rc = direct_init(s, err);
    if (rc) return rc;
  }
  const double it2 = inow();
  if (!use_direct &&
      (opt.preconditioner == 2 || opt.preconditioner < 0)) {
    int rc = amg_init(s, opt.preconditioner < 0, err);
    if (rc) return rc;
  }
  use_chain = !use_amg && !use_direct &&
              (opt.preconditioner == 1 ||
               (opt.preconditioner < 0 && comm.world == 1 && opt.fix_small_angle_b != 0 &&
                off_chain_edges <= std::max<int64_t>(2, nb / 64)));
  chain_seg = std::max(2, std::min(opt.chain_segment > 0 ? opt.chain_segment : 256, CHAIN_SEG_MAX));
  if (use_chain) {
    std::vector<int32_t> sf(nb, -1), scnt(nb, 0);
    for (int32_t i = 1; i < nb; ++i)
      for (int32_t k = s.rowptr[i] + 1; k < s.rowptr[i + 1]; ++k)  // sorted by column after the diagonal
        if (s.colidx[k] == i - 1) {
          if (sf[i] < 0) sf[i] = k;
          ++scnt[i];
        }
    HIPCHK(upload(d_sub_first, sf));
    HIPCHK(upload(d_sub_cnt, scnt));
    HIPCHK(mem.raw(d_Gm, 49 * (size_t)nb));
  }
  double** vecs[] = {&d_b, &d_x, &d_r, &d_z, &d_p, &d_q, &d_s};
  for (double** v : vecs) {
    // padded to world x (7 x rows per rank) so the all-gather can run in place with equal counts
    int64_t padded = 0;
    (void)allgather_equal_plan(offs.data(), comm.world, nullptr, &padded);
    const size_t n_alloc = std::max<size_t>((size_t)n, (size_t)padded);
    HIPCHK(mem.alloc(*v, n_alloc, nullptr));
  }
  HIPCHK(mem.raw(d_part_a, SPAN_GRID_MAX));
  HIPCHK(mem.raw(d_part_b, SPAN_GRID_MAX));
  HIPCHK(mem.alloc(d_sc, 1, nullptr));
  HIPCHK(host_malloc((void**)&h_sc, sizeof(DevScalars)));
  HIPCHK(host_malloc((void**)&h_ring, sizeof(DevScalars) * KB));
  HIPCHK(event_acquire(&ring_ev));
  if (use_amg) {  // level 0 aliases the system's own arrays, vectors, scalars and partial sums
    int rc = amg_bind(s, err);
    if (rc) return rc;
  }
  // the one-system solve's view: the engine's own vectors, scalars and partial sums
  pv_one = PcgView();
  pv_one.x = d_x; pv_one.r = d_r; pv_one.z = d_z; pv_one.p = d_p; pv_one.q = d_q; pv_one.s = d_s; pv_one.az = d_az;
  pv_one.Minv = d_Minv;
  pv_one.b = d_b;
  pv_one.sc = d_sc;
  pv_one.h_sc = h_sc;
  pv_one.part_a = d_part_a;
  pv_one.part_b = d_part_b;
  pv_one.cv = &cv_one;
  // Gram task tables
  GramTables tab;
  int t = 0;
  for (int a = 0; a < 14; ++a)
    for (int b = a; b < 15; ++b) { tab.ga[t] = (unsigned char)a; tab.gb[t] = (unsigned char)b; ++t; }
  t = 0;
  for (int c = 0; c < 7; ++c)
    for (int r = 0; r <= c; ++r) { tab.tr[t] = (unsigned char)r; tab.tc[t] = (unsigned char)c; ++t; }
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_tab), &tab, sizeof(tab)));
  HIPCHK(hipDeviceSynchronize());
  staged.release();
  if (itrace)
    std::fprintf(stderr, "sim3opt engine init: uploads %.2f ms, factorisation plan + its uploads %.2f ms, rest %.2f ms\n",
                 it1 - it0, it2 - it1, inow() - it2);
  return SIM3OPT_OK;
}

int Engine::fetch_scalars(PcgView& V, std::string& err) {
  HIPCHK(hipMemcpyAsync(V.h_sc, V.sc, sizeof(DevScalars) * V.nsc, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (comm.timing && comm.ev_used) return comm.drain(err);
  return SIM3OPT_OK;
}

int Engine::poll_async(const DevScalars* src, int nsc, std::string& err) {
  HIPCHK(hipMemcpyAsync(h_ring, src, sizeof(DevScalars) * nsc, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipEventRecord(ring_ev, stream));
  return SIM3OPT_OK;
}

int Engine::poll_wait(DevScalars* dst, int nsc, std::string& err) {
  HIPCHK(hipEventSynchronize(ring_ev));
  std::memcpy(dst, h_ring, sizeof(DevScalars) * nsc);
  sched_stats[3] += 1;
  return SIM3OPT_OK;
}

// ---- timing helpers ----
// Phase times of an iteration are event stamps on the stream (ev_ph[0] linearise | 1 solve | 2 update | 3), read
// after the trial's chi2 fetch: ONE host round trip per trial; waiting on every phase's end event left the GPU idle
// a quarter of the time on the small graphs.
int Engine::phase_ms(int a, int b, double& acc, std::string& err) {
  if (!phase_timing) return SIM3OPT_OK;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, ev_ph[a], ev_ph[b]));
  acc += ms;
  return SIM3OPT_OK;
}

int Engine::pool_get(hipEvent_t& a, hipEvent_t& b, std::string& err) {
  if (pool_used + 2 > pool.size()) {
    hipEvent_t e0, e1;
    HIPCHK(event_acquire(&e0));
    HIPCHK(event_acquire(&e1));
    pool.push_back(e0);
    pool.push_back(e1);
  }
  a = pool[pool_used];
  b = pool[pool_used + 1];
  pool_used += 2;
  return SIM3OPT_OK;
}

int Engine::pool_drain(std::string& err) {
  if (pool_used > 0) {
    kt.n_spmv += (int64_t)std::max<long long>(0, h_sc->n_spmv_work - spmv_work_seen);
    spmv_work_seen = h_sc->n_spmv_work;
  }
  for (size_t i = 0; i + 1 < pool_used; i += 2) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, pool[i], pool[i + 1]));
    kt.ms_spmv += ms;
  }
  pool_used = 0;
  for (size_t i = 0; i + 1 < rep_used; i += 2) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, rep_pool[i], rep_pool[i + 1]));
    kt.ms_replicated_levels += ms;
    kt.n_replicated_visits += 1;
  }
  rep_used = 0;
  return SIM3OPT_OK;
}

// ---- building blocks ----
// scale_parts > 0: d_part_b holds that many partial sums of the trial's scale (k_scale): summed in the
// same launch as chi2's
// grid > 0 (sim3opt_debug_update only): that many workgroups instead of the rule's
int Engine::chi2(double* out, std::string& err, hipEvent_t before_fetch, int scale_parts, int grid) {
  const int g = grid > 0 ? grid : grid_for(e_hi - e_lo, WG);
  if (has_kernel) hipLaunchKernelGGL(k_chi2<true>, dim3(g), dim3(WG), 0, stream, edge_args(), d_part_a);
  else hipLaunchKernelGGL(k_chi2<false>, dim3(g), dim3(WG), 0, stream, edge_args(), d_part_a);
  // (exact solver on one GPU: small systems, where the copy of the scalar block is a visible share of a trial)
  const bool mirror = scale_parts > 0 && use_direct && !comm.active() && !opt.time_kernels;
  if (scale_parts > 0)
    hipLaunchKernelGGL(k_final_sum_two, dim3(1), dim3(WG), 0, stream, (const double*)d_part_a, g, &d_sc->chi2,
                       (const double*)d_part_b, scale_parts, &d_sc->scale, mirror ? h_sc : (DevScalars*)nullptr,
                       (const DevScalars*)d_sc);
  else
    hipLaunchKernelGGL(k_final_sum, dim3(1), dim3(WG), 0, stream, d_part_a, g, &d_sc->chi2);
  HIPCHK(hipGetLastError());
  int rc = SIM3OPT_OK;
  if (comm.active()) {  // chi2 and scale are adjacent: one 2-double all-reduce per LM trial
    rc = comm.allreduce(&d_sc->chi2, 2, 0, stream, err);
    if (rc) return rc;
  }
  if (before_fetch) HIPCHK(hipEventRecord(before_fetch, stream));
  if (mirror) HIPCHK(hipStreamSynchronize(stream));  // the kernel wrote h_sc's chi2 / scale / fail itself
  else rc = fetch_scalars(err);
  if (rc) return rc;
  *out = h_sc->chi2;
  kt.n_chi2 += 1;
  return SIM3OPT_OK;
}

// debug_full_arrays: nothing outside this rank's ranges may have been written (reads show as NaN in the results)
int Engine::check_foreign_ranges(std::string& err) {
  if (!opt.debug_full_arrays || ranged.empty()) return SIM3OPT_OK;
  DevBuf<unsigned long long> d_cnt;
  HIPCHK(d_cnt.alloc(ranged.size()));
  HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * ranged.size(), stream));
  for (size_t i = 0; i < ranged.size(); ++i) {
    const RangedArray& a = ranged[i];
    const char* base = static_cast<const char*>(a.alloc);
    const size_t head = (size_t)a.lo * a.elem / 4, tail0 = (size_t)a.hi * a.elem, tail = ((size_t)a.total * a.elem - tail0) / 4;
    if (head) hipLaunchKernelGGL(k_count_unpoisoned, dim3(1024), dim3(WG), 0, stream, reinterpret_cast<const uint32_t*>(base), head, d_cnt + i);
    if (tail) hipLaunchKernelGGL(k_count_unpoisoned, dim3(1024), dim3(WG), 0, stream, reinterpret_cast<const uint32_t*>(base + tail0), tail, d_cnt + i);
  }
  std::vector<unsigned long long> h(ranged.size(), 0);
  const hipError_t e1 = hipMemcpyAsync(h.data(), d_cnt, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, stream);
  HIPCHK(hipStreamSynchronize(stream));  // (whatever the copy said: the launches above are behind it before d_cnt goes)
  HIPCHK(e1);
  for (size_t i = 0; i < h.size(); ++i)
    if (h[i]) {
      err = "debug_full_arrays: " + std::to_string(h[i]) + " words outside this rank's range of ranged array " +
            std::to_string(i) + " were written (rank " + std::to_string(comm.rank) + ")";
      return SIM3OPT_ERR_STATE;
    }
  return SIM3OPT_OK;
}

// the eight instantiations of the linearisation (DUMP: their read-out twins, lm_kernels.hpp)
template <bool DUMP>
static void launch_linearize(bool analytic, bool has_info, bool has_kernel, int g, hipStream_t stream, const LinArgs& A) {
  if (analytic) {
    if (has_info && has_kernel)
      hipLaunchKernelGGL((k_linearize_analytic<true, true, DUMP>), dim3(g), dim3(WG), 0, stream, A);
    else if (has_info)
      hipLaunchKernelGGL((k_linearize_analytic<true, false, DUMP>), dim3(g), dim3(WG), 0, stream, A);
    else if (has_kernel)
      hipLaunchKernelGGL((k_linearize_analytic<false, true, DUMP>), dim3(g), dim3(WG), 0, stream, A);
    else
      hipLaunchKernelGGL((k_linearize_analytic<false, false, DUMP>), dim3(g), dim3(WG), 0, stream, A);
  } else {
    if (has_info && has_kernel)
      hipLaunchKernelGGL((k_linearize_numeric<true, true, DUMP>), dim3(g), dim3(WG), 0, stream, A);
    else if (has_info)
      hipLaunchKernelGGL((k_linearize_numeric<true, false, DUMP>), dim3(g), dim3(WG), 0, stream, A);
    else if (has_kernel)
      hipLaunchKernelGGL((k_linearize_numeric<false, true, DUMP>), dim3(g), dim3(WG), 0, stream, A);
    else
      hipLaunchKernelGGL((k_linearize_numeric<false, false, DUMP>), dim3(g), dim3(WG), 0, stream, A);
  }
}

int Engine::linearize(std::string& err) {
  const sim3::Opts mo = mopts();
  const bool analytic = opt.jacobians == 1;  // closed form: no perturbation table
  if (!analytic && !d_ptab) HIPCHK(mem.raw(d_ptab, 14));
  if (!analytic && (ptab_delta != opt.fd_delta || ptab_opts.eps != mo.eps ||
                    ptab_opts.small_rot_half != mo.small_rot_half || ptab_opts.fix_small_b != mo.fix_small_b)) {
    hipLaunchKernelGGL(k_perturbation_table, dim3(1), dim3(64), 0, stream, opt.fd_delta, mo, d_ptab);
    ptab_delta = opt.fd_delta;
    ptab_opts = mo;
  }
  LinArgs A{n_active, d_active, d_ev0, d_ev1, d_meas, d_info, d_kdelta, d_kkind, d_states,
            d_slot01, d_slot10, d_inc0, d_inc1, d_vals, d_scratch, opt.fd_delta, mo,
            (const Sim3*)d_ptab, opt.dof_mask, d_sc};
  const int g = (n_active + EPB - 1) / EPB;
  if (g == 0) HIPCHK(hipMemsetAsync(&d_sc->maxdiag_bits, 0, sizeof(unsigned long long), stream));
  if (g > 0) {
    if (lin_dump) launch_linearize<true>(analytic, has_info, has_kernel, g, stream, A);  // (sim3opt_debug_linearization)
    else launch_linearize<false>(analytic, has_info, has_kernel, g, stream, A);
  }
  const int gdr = grid_for(r1 - r0, 4);
  hipLaunchKernelGGL(k_diag_reduce, dim3(gdr), dim3(WG), 0, stream, r0, r1,
                     d_incptr, d_rowptr, d_scratch, d_vals, d_b, d_sc, d_part_a, d_part_b);
  hipLaunchKernelGGL(k_final_trace_max, dim3(1), dim3(WG), 0, stream, (const double*)d_part_a,
                     (const double*)d_part_b, gdr, &d_sc->trace, &d_sc->maxdiag_bits);
  HIPCHK(hipGetLastError());
  if (comm.active()) {  // non-negative doubles order like their bit patterns
    int rc = comm.allreduce(reinterpret_cast<double*>(&d_sc->maxdiag_bits), 1, 1, stream, err);
    if (rc) return rc;
    rc = comm.allreduce(&d_sc->trace, 1, 0, stream, err);  // (every rank must take the same decisions)
    if (rc) return rc;
  }
  if (use_direct) lm_factor.gather(d_vals, d_b, stream);  // the factorisation's starting blocks (k_ldl_gather)
  linearized = true;
  amg_stale = true;
  trace_stale = true;
  kt.n_linearize += 1;
  return SIM3OPT_OK;
}

// ---- the iteration frame of LM, Gauss-Newton and dogleg (the other two: engine_algorithms.hip) ----
int Engine::iter_begin(sim3opt_iter_stats& T, double& chi, std::string& err) {
  if (phase_timing) HIPCHK(hipEventRecord(ev_ph[0], stream));
  // computeActiveErrors at the start of an iteration: the estimates are those the last trial
  // evaluated (accepted) or restored (rejected), and the evaluation is deterministic, so the
  // value is already here -- one host round trip less per iteration
  if (chi_known) chi = chi_cache;
  else {
    int rc = chi2(&chi, err);
    if (rc) return rc;
  }
  T.chi2_before = chi;
  return linearize(err);
}

void Engine::iter_end(sim3opt_iter_stats& T, double chi, std::vector<sim3opt_iter_stats>& stats) {
  kt.ms_linearize += T.ms_linearize;
  kt.ms_update += T.ms_update;
  chi_known = true;
  chi_cache = chi;
  T.chi2_after = chi;
  stats.push_back(T);
}

// pcg() reports success on the exact path: a non-positive pivot comes back in the scalars of the caller's next
// fetch (k_oplus left the estimates alone then)
bool Engine::direct_rejected() const { return use_direct && h_sc->fail == fail_token; }

void Engine::apply_step(const double* x, bool push) {
  hipLaunchKernelGGL(k_oplus, dim3((nv + WG - 1) / WG), dim3(WG), 0, stream, nv, d_hidx, x, d_states, mopts(),
                     use_direct ? (const DevScalars*)d_sc : nullptr, push ? d_backup : (Sim3*)nullptr, fail_token);
}

void Engine::pop_states() {
  hipLaunchKernelGGL(k_copy_states, dim3((8 * nv + WG - 1) / WG), dim3(WG), 0, stream, nv, (const Sim3*)d_backup,
                     d_states);
}

int Engine::optimize(int32_t max_iters, std::vector<sim3opt_iter_stats>& stats, std::string& err) {
  stats.clear();
  tr_stats.clear();
  chi_known = false;  // (options or estimates may have changed since the last call)
  if (opt.algorithm == SIM3OPT_ALGORITHM_GAUSS_NEWTON) return optimize_gauss_newton(max_iters, stats, err);
  if (opt.algorithm == SIM3OPT_ALGORITHM_DOGLEG) return optimize_dogleg(max_iters, stats, err);
  LmDamping damp;
  bool ok = true;
  int iters = 0;
  for (int it = 0; it < max_iters && ok; ++it) {
    sim3opt_iter_stats T{};
    double currentChi = 0.0;
    int rc = iter_begin(T, currentChi, err);
    if (rc) return rc;
    if (it == 0) {  // lambda_0: one host round trip more
      rc = fetch_scalars(err);
      if (rc) return rc;
      double maxdiag;
      std::memcpy(&maxdiag, &h_sc->maxdiag_bits, sizeof(double));
      damp.start(opt.user_lambda_init, opt.tau, maxdiag);
    }
    double rho = 0.0;
    int qmax = 0;
    do {
      if (phase_timing) HIPCHK(hipEventRecord(ev_ph[1], stream));  // (push(): k_oplus keeps the old estimates itself)
      const double* xsol = d_x;  // the step of this trial
      int32_t pit = 0;
      double rres = 0.0;
      bool ok2 = true;
      rc = lm_trial_solve(qmax, damp.lambda, damp.ni, &xsol, &pit, &rres, &ok2, err);
      if (rc) return rc;
      if (phase_timing) HIPCHK(hipEventRecord(ev_ph[2], stream));
      T.pcg_iters += pit;
      T.pcg_rel_res = rres;
      if (last_capped) T.pcg_capped += 1;
      if (opt.verbose >= 2)
        std::fprintf(stderr, "  trial %d: lambda %.6g, %d PCG iterations (rel %.2e)\n", qmax, damp.lambda, pit, rres);
      double tempChi = DBL_MAX, scale = 0.0;  // (solver failed: g2o forces rejection)
      if (ok2) {
        apply_step(xsol, true);
        const int ge = grid_for(7 * (int64_t)(r1 - r0), WG);
        hipLaunchKernelGGL(k_scale, dim3(ge), dim3(WG), 0, stream, 7 * r0, 7 * r1, xsol, d_b,
                           damp.lambda, d_part_b);
        HIPCHK(hipGetLastError());
        rc = chi2(&tempChi, err, phase_timing ? ev_ph[3] : nullptr, ge);  // also sums and brings back scale (and the factorisation's verdict)
        if (rc) return rc;
        rc = phase_ms(2, 3, T.ms_update, err);
        if (rc) return rc;
        scale = h_sc->scale;
        kt.n_update += 1;
        if (direct_rejected()) {  // not positive definite: g2o's solver returns false
          tempChi = DBL_MAX;
          scale = 0.0;
        }
      } else {
        if (phase_timing) HIPCHK(hipEventSynchronize(ev_ph[2]));
        else HIPCHK(hipStreamSynchronize(stream));
      }
      rc = phase_ms(1, 2, T.ms_solve, err);
      if (rc) return rc;
      if (qmax == 0 && (rc = phase_ms(0, 1, T.ms_linearize, err))) return rc;
      if (damp.update(currentChi, tempChi, scale, opt.good_step_lower, opt.good_step_upper, rho))
        currentChi = tempChi;  // discardTop
      else if (ok2)
        pop_states();  // (a failed solve never touched the estimates -- nor the backup)
      ++qmax;
    } while (rho < 0 && qmax < opt.max_trials);
    T.lambda = damp.lambda;
    T.rho = rho;
    T.trials = qmax;
    iter_end(T, currentChi, stats);
    ++iters;
    if (opt.verbose)
      std::fprintf(stderr,
                   "iteration= %d\t chi2= %.9g\t lambda= %.6g\t levenbergIter= %d\t pcg= %d "
                   "(rel %.2e)\t ms lin/solve/upd= %.3f/%.3f/%.3f\n",
                   it, currentChi, damp.lambda, qmax, T.pcg_iters, T.pcg_rel_res, T.ms_linearize,
                   T.ms_solve, T.ms_update);
    if (damp.terminate(qmax, opt.max_trials, rho)) ok = false;
  }
  HIPCHK(hipStreamSynchronize(stream));
  return iters;
}

// ------------------------------------------------------------------------------------------
// C++ interface used by capi.cpp
// ------------------------------------------------------------------------------------------
Engine* engine_create(const HostGraph& g, const Structure& s, const sim3opt_options& opt,
                      Comm* comm, std::string& err, int& status) {
  Engine* e = new Engine();
  e->opt = opt;
  if (comm) {  // the engine takes the communicator over
    e->comm = *comm;
    *comm = Comm();
  }
  e->comm.timing = opt.time_kernels != 0;
  status = e->init(g, s, err);
  if (status != SIM3OPT_OK) {
    delete e;
    return nullptr;
  }
  return e;
}

void engine_destroy(Engine* e) { delete e; }

void engine_take_comm(Engine* e, Comm* out) {
  *out = e->comm;   // the caller owns the communicator again (re-initialisation keeps the ranks)
  e->comm = Comm();
}

int engine_set_options(Engine* e, const sim3opt_options& opt) {
  const int dev = e->opt.device, full = e->opt.debug_full_arrays;  // (fixed at initialisation)
  e->opt = opt;
  e->opt.device = dev;
  e->opt.debug_full_arrays = full;
  e->comm.timing = opt.time_kernels != 0;
  // (the events exist in any case: the flags may be set after sim3opt_initialize)
  e->phase_timing = opt.time_kernels != 0 || opt.verbose != 0 || e->nb > 4096;
  return SIM3OPT_OK;
}

int engine_optimize(Engine* e, int32_t max_iters, std::vector<sim3opt_iter_stats>& stats,
                    std::string& err) {
  int rc = e->optimize(max_iters, stats, err);
  if (rc) return rc;
  return e->check_foreign_ranges(err);
}

void engine_trust_region_stats(const Engine* e, std::vector<sim3opt_tr_stats>& out) { out = e->tr_stats; }

int engine_chi2(Engine* e, double* chi2, std::string& err) { return e->chi2(chi2, err); }

int engine_get_states(Engine* e, Sim3* out, std::string& err) {
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, e->d_states, sizeof(Sim3) * (size_t)e->nv, hipMemcpyDeviceToHost));
  return SIM3OPT_OK;
}

int engine_set_states(Engine* e, const Sim3* in, std::string& err) {
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(e->d_states, in, sizeof(Sim3) * (size_t)e->nv, hipMemcpyHostToDevice));
  e->linearized = false;
  e->chi_known = false;
  return SIM3OPT_OK;
}

int engine_edge_errors(Engine* e, double* out, std::string& err) {
  DevBuf<double> d_out;
  HIPCHK(d_out.alloc(7 * std::max<size_t>((size_t)e->ne, 1)));
  EdgeArgs ea = e->edge_args();
  ea.e_lo = 0;
  ea.e_hi = e->ne;
  hipLaunchKernelGGL(k_edge_errors, dim3(grid_for(e->ne, WG)), dim3(WG), 0, e->stream, ea, d_out.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, d_out, sizeof(double) * 7 * (size_t)e->ne, hipMemcpyDeviceToHost));
  return SIM3OPT_OK;
}

int engine_edge_chi2(Engine* e, double* chi2, double* rho, double* weight, std::string& err) {
  const size_t m = (size_t)e->ne;
  DevBuf<double> d_out;
  HIPCHK(d_out.alloc(3 * std::max<size_t>(m, 1)));
  EdgeArgs ea = e->edge_args();  // (replicated states: every rank evaluates every edge)
  ea.e_lo = 0;
  ea.e_hi = e->ne;
  hipLaunchKernelGGL(k_edge_chi2, dim3(grid_for(e->ne, WG)), dim3(WG), 0, e->stream, ea,
                     chi2 ? d_out.get() : nullptr, rho ? d_out + m : nullptr, weight ? d_out + 2 * m : nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  if (chi2) HIPCHK(hipMemcpy(chi2, d_out, sizeof(double) * m, hipMemcpyDeviceToHost));
  if (rho) HIPCHK(hipMemcpy(rho, d_out + m, sizeof(double) * m, hipMemcpyDeviceToHost));
  if (weight) HIPCHK(hipMemcpy(weight, d_out + 2 * m, sizeof(double) * m, hipMemcpyDeviceToHost));
  return SIM3OPT_OK;
}

int engine_set_kernels(Engine* e, const HostGraph& g, std::string& err) {
  const size_t m = (size_t)e->ne;
  if (g.kdelta.size() != m || g.kkind.size() != m) {
    err = "set_edge_kernels: host arrays out of step with the engine";
    return SIM3OPT_ERR_STATE;
  }
  HIPCHK(hipStreamSynchronize(e->stream));  // (a launch in flight may still read the old arrays)
  if (!e->d_kdelta) HIPCHK(e->mem.raw(e->d_kdelta, m));
  if (!e->d_kkind) HIPCHK(e->mem.raw(e->d_kkind, m));
  if (m) {
    HIPCHK(hipMemcpy(e->d_kdelta, g.kdelta.data(), sizeof(double) * m, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->d_kkind, g.kkind.data(), sizeof(uint8_t) * m, hipMemcpyHostToDevice));
  }
  e->has_kernel = true;
  e->linearized = false;  // the next chi2 / linearize / optimize sees the new kernels
  e->chi_known = false;
  return SIM3OPT_OK;
}

int engine_edge_jacobians(Engine* e, double* e_out, double* J_out, std::string& err) {
  const size_t m = (size_t)e->ne;
  DevBuf<double> d_out;
  HIPCHK(d_out.alloc(105 * std::max<size_t>(m, 1)));
  EdgeArgs ea = e->edge_args();
  ea.e_lo = 0;
  ea.e_hi = e->ne;
  hipLaunchKernelGGL(k_edge_jacobians, dim3(grid_for(e->ne, WG)), dim3(WG), 0, e->stream, ea, e->opt.dof_mask,
                     d_out.get(), d_out + 7 * m);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(e_out, d_out, sizeof(double) * 7 * m, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(J_out, d_out + 7 * m, sizeof(double) * 98 * m, hipMemcpyDeviceToHost));
  return SIM3OPT_OK;
}

int engine_linearize(Engine* e, std::string& err) {
  int rc = e->linearize(err);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return e->check_foreign_ranges(err);
}

// ---- diagnostic read-outs of the LM set-up and update kernels (include/sim3opt.h, "Diagnostic.") ----
void engine_debug_linearization_dims(const Engine* e, int32_t* n_active, int32_t* n_incidences) {
  if (n_active) *n_active = e->n_active;
  if (n_incidences) *n_incidences = e->st.incptr[e->nb];
}

int engine_debug_linearization(Engine* e, double* J, double* w, int32_t* active, double* scratch, int32_t* incptr,
                               int32_t* inc0, int32_t* inc1, int32_t* slot01, int32_t* slot10, double* trace,
                               double* maxdiag, std::string& err) {
  if (e->comm.active()) {
    err = "debug_linearization: a partitioned graph holds this rank's share only (one GPU, please)";
    return SIM3OPT_ERR_STATE;
  }
  const size_t na = (size_t)e->n_active, ninc = (size_t)e->st.incptr[e->nb], m = (size_t)e->ne;
  DevBuf<double> d_dump;
  HIPCHK(d_dump.alloc(106 * std::max<size_t>(na, 1)));
  const LinDump dump{d_dump, d_dump + 105 * std::max<size_t>(na, 1)};
  HIPCHK(hipStreamSynchronize(e->stream));  // (the symbol is written outside the stream)
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(d_lin_dump), &dump, sizeof(LinDump)));
  const sim3opt_kernel_times kt0 = e->kt;
  e->lin_dump = true;
  const int rc = e->linearize(err);  // the launches of sim3opt_linearize, the linearisation kernel in its DUMP instantiation
  e->lin_dump = false;
  e->kt = kt0;
  const hipError_t es = hipStreamSynchronize(e->stream);  // (whatever it said: its launches are done before d_dump goes)
  if (rc) return rc;
  HIPCHK(es);
  if (na) {
    HIPCHK(hipMemcpy(J, dump.J, sizeof(double) * 105 * na, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(w, dump.w, sizeof(double) * na, hipMemcpyDeviceToHost));
  }
  if (ninc) HIPCHK(hipMemcpy(scratch, e->d_scratch, sizeof(double) * 35 * ninc, hipMemcpyDeviceToHost));
  unsigned long long bits = 0;
  HIPCHK(hipMemcpy(trace, &e->d_sc->trace, sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&bits, &e->d_sc->maxdiag_bits, sizeof(bits), hipMemcpyDeviceToHost));
  std::memcpy(maxdiag, &bits, sizeof(double));
  // the index arrays as uploaded (one rank: the structure's own)
  if (na) std::memcpy(active, e->st.active.data(), sizeof(int32_t) * na);
  std::memcpy(incptr, e->st.incptr.data(), sizeof(int32_t) * ((size_t)e->nb + 1));
  if (m) {
    std::memcpy(inc0, e->st.inc0.data(), sizeof(int32_t) * m);
    std::memcpy(inc1, e->st.inc1.data(), sizeof(int32_t) * m);
    std::memcpy(slot01, e->st.slot01.data(), sizeof(int32_t) * m);
    std::memcpy(slot10, e->st.slot10.data(), sizeof(int32_t) * m);
  }
  return SIM3OPT_OK;
}

int engine_debug_update(Engine* e, const double* x, double lambda, bool with_fail, int32_t grid, double* states_out,
                        double* backup_out, double* chi2, double* scale, std::string& err) {
  if (e->comm.active()) {
    err = "debug_update: a partitioned graph holds this rank's share only (one GPU, please)";
    return SIM3OPT_ERR_STATE;
  }
  if (!e->linearized) {
    err = "debug_update: call sim3opt_linearize (or optimize) first: the scale needs b";
    return SIM3OPT_ERR_STATE;
  }
  if (with_fail && !e->use_direct) {
    err = "debug_update: with_fail needs the exact solver (only its failure token reaches k_oplus)";
    return SIM3OPT_ERR_STATE;
  }
  if (grid < 0 || grid > MAX_GRID) {
    err = "debug_update: grid out of range";
    return SIM3OPT_ERR_ARG;
  }
  // everything a trial's launches overwrite that a later call could see
  SolverSnapshot snap;
  int rc = snap.take(*e, err);
  if (rc) return rc;
  DevBuf<double> d_step;  // (outlives the put-back's synchronisation)
  double chi = 0.0, sc = 0.0;
  bool pushed = false;
  auto body = [&]() -> int {
    HIPCHK(d_step.alloc(std::max<size_t>((size_t)e->n, 1)));
    HIPCHK(hipMemcpy(d_step, x, sizeof(double) * (size_t)e->n, hipMemcpyHostToDevice));
    if (with_fail) {
      const int32_t token = e->fail_token;  // what the factorisation of the current solve stores on a bad pivot
      HIPCHK(hipMemcpy(&e->d_sc->fail, &token, sizeof(int32_t), hipMemcpyHostToDevice));
    }
    // the launches of an LM trial after its solve (Engine::optimize)
    pushed = true;
    e->apply_step(d_step, true);
    const int ge = grid > 0 ? grid : grid_for(7 * (int64_t)(e->r1 - e->r0), WG);
    hipLaunchKernelGGL(k_scale, dim3(ge), dim3(WG), 0, e->stream, 7 * e->r0, 7 * e->r1, (const double*)d_step,
                       (const double*)e->d_b, lambda, e->d_part_b);
    HIPCHK(hipGetLastError());
    const int rc2 = e->chi2(&chi, err, nullptr, ge, grid);
    if (rc2) return rc2;
    sc = e->h_sc->scale;
    HIPCHK(hipStreamSynchronize(e->stream));
    if (states_out) HIPCHK(hipMemcpy(states_out, e->d_states, sizeof(Sim3) * (size_t)e->nv, hipMemcpyDeviceToHost));
    if (backup_out) HIPCHK(hipMemcpy(backup_out, e->d_backup, sizeof(Sim3) * (size_t)e->nv, hipMemcpyDeviceToHost));
    return SIM3OPT_OK;
  };
  rc = body();
  if (pushed) e->pop_states();  // (the backup was taken whatever followed it)
  rc = snap.put_back(rc, err);
  if (rc) return rc;
  if (chi2) *chi2 = chi;
  if (scale) *scale = sc;
  return SIM3OPT_OK;
}

int engine_get_system(Engine* e, int32_t* rowptr, int32_t* colidx, double* values, double* b,
                      std::string& err) {
  if (!e->linearized) {
    err = "get_system: call sim3opt_linearize (or optimize) first";
    return SIM3OPT_ERR_STATE;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  if (rowptr) std::memcpy(rowptr, e->st.rowptr.data(), sizeof(int32_t) * (size_t)(e->nb + 1));
  if (colidx) std::memcpy(colidx, e->st.colidx.data(), sizeof(int32_t) * (size_t)e->nnzb);
  if (values) {  // (a partitioned run holds this rank's rows only: the other rows' blocks read zero)
    const size_t k0 = (size_t)49 * e->st.rowptr[e->r0], k1 = (size_t)49 * e->st.rowptr[e->r1];
    std::memset(values, 0, sizeof(double) * 49 * (size_t)e->nnzb);
    if (k1 > k0) HIPCHK(hipMemcpy(values + k0, e->d_vals + k0, sizeof(double) * (k1 - k0), hipMemcpyDeviceToHost));
  }
  if (b) HIPCHK(hipMemcpy(b, e->d_b, sizeof(double) * (size_t)e->n, hipMemcpyDeviceToHost));
  return SIM3OPT_OK;
}

int engine_solve(Engine* e, double lambda, double* x, int32_t* iters, double* rel_res,
                 std::string& err) {
  if (!e->linearized) {
    err = "solve: call sim3opt_linearize (or optimize) first";
    return SIM3OPT_ERR_STATE;
  }
  int32_t it = 0;
  double rr = 0.0;
  bool ok = true;
  int rc = e->pcg(lambda, &it, &rr, &ok, err);
  if (rc) return rc;
  if (e->use_direct) {  // the factorisation reports a non-positive pivot through the scalars
    rc = e->fetch_scalars(err);
    if (rc) return rc;
    ok = !e->direct_rejected();
  }
  if (iters) *iters = it;
  if (rel_res) *rel_res = rr;
  if (x) HIPCHK(hipMemcpy(x, e->d_x, sizeof(double) * (size_t)e->n, hipMemcpyDeviceToHost));
  if (!ok) {
    err = "solve: PCG breakdown (system not positive definite)";
    return SIM3OPT_ERR_STATE;
  }
  return SIM3OPT_OK;
}

void engine_local_rows(const Engine* e, int32_t* begin, int32_t* end) {
  if (begin) *begin = e->r0;
  if (end) *end = e->r1;
}

int engine_preconditioner(const Engine* e) { return e->use_amg ? 2 : (e->use_chain ? 1 : 0); }

int engine_linear_solver(const Engine* e) { return e->use_direct ? 1 : 0; }

int engine_span_grid(const Engine* e) { return e->span_grid; }
void engine_spmv_variant(const Engine* e, int32_t* chunk, int32_t* non_temporal) {  // (as spmv_raw branches)
  *chunk = e->spmv_chunk <= 4 ? 4 : 8;
  *non_temporal = e->spmv_nt ? 1 : 0;
}

void engine_device_bytes(const Engine* e, int64_t bytes[2]) {
  bytes[0] = e->ranged_bytes();
  bytes[1] = 0;
  for (const Engine::RangedArray& a : e->ranged) bytes[1] += (int64_t)a.elem * a.total;
}

void engine_amg_in_use(const Engine* e, int32_t* n_levels, int32_t* n_partitioned, int32_t visits[4]) {
  if (n_levels) *n_levels = e->use_amg ? (int32_t)e->amg.size() : 0;
  if (n_partitioned) *n_partitioned = e->use_amg ? e->n_sharded : 0;
  if (visits)
    for (int l = 0; l < 4; ++l) visits[l] = e->use_amg ? e->amg_visits[l + 1] : 0;
}

int engine_kernel_times(Engine* e, sim3opt_kernel_times* out, bool reset) {
  if (out) *out = e->kt;
  if (reset) {
    e->kt = sim3opt_kernel_times{};
    e->comm.times = sim3opt_comm_times{};
    for (int64_t& v : e->sched_stats) v = 0;
  }
  return SIM3OPT_OK;
}

void engine_pcg_schedule_stats(Engine* e, int64_t out[4], bool reset) {
  for (int i = 0; i < 4; ++i) {
    if (out) out[i] = e->sched_stats[i];
    if (reset) e->sched_stats[i] = 0;
  }
}

int engine_comm_times(Engine* e, sim3opt_comm_times* out) {
  std::string err;
  if (e->comm.ev_used) {  // pairs recorded since the last synchronisation
    if (hipStreamSynchronize(e->stream) != hipSuccess) return SIM3OPT_ERR_HIP;
    int rc = e->comm.drain(err);
    if (rc) return rc;
  }
  *out = e->comm.times;
  return SIM3OPT_OK;
}

// ---- diagnostic read-outs of the in-process transport (sim3opt_comm_apply_*, tests/test_gpu_comm_operators.py) ----
// One collective of this rank's own Comm on this rank's own stream, on an operand the caller supplies.  The operand
// lives in a scratch block of its own between guard doubles: COMM_GUARD of them either side (plus `phase` more in
// front, which puts the operand on an even or an odd double of a 16-byte aligned block), all of one bit pattern that
// no copy and no fold produces.  After the collective the whole block comes back and every guard is compared.
namespace {

constexpr int64_t COMM_GUARD = 4;
constexpr uint64_t COMM_GUARD_BITS = 0x7ff4c0dedbadf00dull;  // (a signalling-NaN payload)

struct GuardedOperand {
  DevBuf<double> dev;
  std::vector<double> host;
  int64_t n = 0, lead = 0;
  double* ptr() const { return dev.get() + lead; }
  int upload(const double* src, int64_t n_, int phase, hipStream_t stream, std::string& err) {
    n = n_;
    lead = COMM_GUARD + phase;
    double guard;
    std::memcpy(&guard, &COMM_GUARD_BITS, sizeof(double));
    host.assign((size_t)(lead + n + COMM_GUARD), guard);
    if (n) std::memcpy(host.data() + lead, src, sizeof(double) * (size_t)n);
    HIPCHK(dev.alloc(host.size()));
    HIPCHK(hipMemcpyAsync(dev.get(), host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, stream));
    return SIM3OPT_OK;
  }
  // (the caller has synchronised the stream after the collective)
  int download(double* dst, int rank, const char* what, std::string& err) {
    HIPCHK(hipMemcpy(host.data(), dev.get(), sizeof(double) * host.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < (int64_t)host.size(); ++i) {
      if (i >= lead && i < lead + n) continue;
      uint64_t bits;
      std::memcpy(&bits, &host[(size_t)i], sizeof(bits));
      if (bits != COMM_GUARD_BITS) {
        err = std::string(what) + ": rank " + std::to_string(rank) + " wrote the guard double at index " +
              std::to_string(i - lead) + " of its operand of " + std::to_string(n) + " doubles";
        return SIM3OPT_ERR_STATE;
      }
    }
    if (n) std::memcpy(dst, host.data() + lead, sizeof(double) * (size_t)n);
    return SIM3OPT_OK;
  }
};

// the stream is quiet and the timing pairs of the collective are folded in, as after the engine's own look at its scalars
int comm_apply_finish(Engine* e, std::string& err) {
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->comm.timing && e->comm.ev_used) return e->comm.drain(err);
  return SIM3OPT_OK;
}

// (a failed collective: whatever it queued on the scratch blocks is behind us before they go back to the cache)
int comm_apply_failed(Engine* e, int rc) {
  (void)hipStreamSynchronize(e->stream);
  return rc;
}

}  // namespace

int engine_comm_apply_allreduce(Engine* e, int32_t n, int32_t op, int32_t phase, const double* in, double* out,
                                std::string& err) {
  GuardedOperand a;
  int rc = a.upload(in, n, phase, e->stream, err);
  if (rc) return rc;
  rc = e->comm.allreduce(a.ptr(), n, op, e->stream, err);
  if (rc) return comm_apply_failed(e, rc);
  rc = comm_apply_finish(e, err);
  if (rc) return rc;
  return a.download(out, e->comm.rank, "comm_apply_allreduce", err);
}

int engine_comm_apply_allgatherv(Engine* e, const int64_t* offs, int32_t phase, const double* in, double* out,
                                 std::string& err) {
  const std::vector<int64_t> o(offs, offs + e->comm.world + 1);
  GuardedOperand a;
  int rc = a.upload(in, o.back(), phase, e->stream, err);
  if (rc) return rc;
  rc = e->comm.allgatherv(a.ptr(), o, e->stream, err);
  if (rc) return comm_apply_failed(e, rc);
  rc = comm_apply_finish(e, err);
  if (rc) return rc;
  return a.download(out, e->comm.rank, "comm_apply_allgatherv", err);
}

int engine_comm_apply_exchange(Engine* e, const int64_t* soffs, const int64_t* roffs, int32_t send_phase,
                               int32_t recv_phase, const double* send, double* recv, std::string& err) {
  const std::vector<int64_t> so(soffs, soffs + e->comm.world + 1), ro(roffs, roffs + e->comm.world + 1);
  GuardedOperand s, r;
  int rc = s.upload(send, so.back(), send_phase, e->stream, err);
  if (rc) return rc;
  rc = r.upload(recv, ro.back(), recv_phase, e->stream, err);
  if (rc) return rc;
  rc = e->comm.exchange(s.ptr(), so, r.ptr(), ro, e->stream, err);
  if (rc) return comm_apply_failed(e, rc);
  rc = comm_apply_finish(e, err);
  if (rc) return rc;
  std::vector<double> sent((size_t)so.back());  // (the send buffer is an input: it must come back as it went)
  rc = s.download(sent.data(), e->comm.rank, "comm_apply_exchange (send buffer)", err);
  if (rc) return rc;
  if (so.back() && std::memcmp(sent.data(), send, sizeof(double) * sent.size()) != 0) {
    err = "comm_apply_exchange: rank " + std::to_string(e->comm.rank) + " changed its send buffer";
    return SIM3OPT_ERR_STATE;
  }
  return r.download(recv, e->comm.rank, "comm_apply_exchange (receive buffer)", err);
}

bool engine_comm_local_state(const Engine* e, int64_t out[2]) {
  if (e->comm.kind != 3 || !e->comm.local) return false;
  const LocalRank& r0 = e->comm.local->ranks[0];
  out[0] = r0.cap;
  out[1] = (int64_t)r0.seq;
  return true;
}


}  // namespace sim3opt
