// engine_impl.hpp -- the Engine class shared by the translation units of the device-resident LM:
//   engine.hip         initialisation, linearisation, chi2, the iteration frame of LM, Gauss-Newton and dogleg, the
//                      LM trial loop (OptimizationAlgorithmLevenberg::solve; its damping rule: lm_damping.hpp)
//   engine_pcg.hip     the preconditioned CG (LinearSolverEigen's role on graphs too large to factor) -- one driver for
//                      one system and for the systems of a batch: PcgView --, the batch's buffers, an LM trial's solve
//                      (lm_trial_solve) and the halo exchange
//   engine_amg.hip     the aggregation-multigrid preconditioner: set-up per linearisation / per trial, the cycle
//                      (one driver for one system and for the systems of a batch: CycleView)
//   engine_direct.hip  when the LM factorises exactly (LinearSolverEigen's role on KITTI-00-like graphs) and the
//                      marginal covariances: policy over two BlockLdl (direct_factor.hpp, direct_factor.hip)
//   engine_algorithms.hip  Gauss-Newton and Powell's dogleg (options.algorithm = 1 / 2)
//   engine_columns.hip  blocks of (H + lambda I)^-1 by columns of the inverse (options.cov_solver)
// Every kernel header belongs to ONE translation unit (lm_kernels.hpp -> engine.hip, pcg_kernels.hpp ->
// engine_pcg.hip, amg_kernels.hpp -> engine_amg.hip, algo_kernels.hpp -> engine_algorithms.hip, gate_kernels.hpp -> engine_direct.hip, col_kernels.hpp -> engine_columns.hip, direct_ / selinv_ / cov_kernels.hpp -> direct_factor.hip); only
// the SpMV template (spmv_kernel.hpp) is shared.  A kernel another unit needs is reached through a method.
#pragma once
// (formerly all of engine.hip) -- device-resident Levenberg-Marquardt on a Sim(3) pose graph, gfx950 (MI355X).
//
// What it replaces in the reference (all third-party g2o code reached from
// optimizer.optimize(100), kitti_surf.cpp:675; restated per SURVEY.md 3.3 / App. C):
//   EdgeSim3::computeError                     -> k_chi2, k_edge_errors, k_linearize_numeric
//   BaseBinaryEdge::linearizeOplus (numeric)   -> k_linearize_numeric (lane = one +-delta evaluation)
//   BaseBinaryEdge::constructQuadraticForm     -> k_linearize_numeric (Gram phase) + k_diag_reduce
//   (options.jacobians = 1: closed-form J)     -> k_linearize_analytic (sim3_jac.hpp; same Gram phase)
//   BlockSolverX::buildSystem / setLambda      -> block-CSR values in HBM; lambda folded into SpMV
//   LinearSolverEigen::solve (SimplicialLDLT)  -> preconditioned CG: k_spmv_span, k_pcg_*; block-Jacobi
//                                                 (k_jacobi), chain segments (k_chain_*) or aggregation
//                                                 multigrid (amg.cpp, amg_kernels.hpp, Engine::amg_*)
//   VertexSim3Expmap::oplusImpl, push/pop      -> k_oplus + device-to-device backup copies
//   OptimizationAlgorithmLevenberg::solve      -> Engine::optimize (host control, 3 scalars per trial)
//
// HBM layout (all FP64, indices int32):
//   states   V x 8   AoS, 64 B per vertex (one gather = one half-line)
//   meas     E x 8   AoS, 64 B per edge; ev0/ev1 SoA int32; info E x 49 only if some edge is not I7
//   vals     nnzb x 49, column-major 7x7 blocks, block row = free vertex, diagonal block first
//   scratch  (#incidences) x 35: per (edge, endpoint) upper triangle of J^T W J (28) and -J^T W e (7)
//   PCG vectors x r z p q b: 7*nb each; Minv nb x 49 row-major
//   multigrid   P nb x 49 (Ad(S_v)), per coarse level its own block-CSR + diagH/W/Minv + 3 vectors,
//               dense inverse of the coarsest level (two n x n buffers, n <= 1792)
// Assembly is atomic-free and reduction orders are fixed, so results are bitwise reproducible.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "amg.hpp"
#include "comm.hpp"
#include "devmem.hpp"
#include "direct_factor.hpp"
#include "engine.hpp"

namespace sim3opt {

using sim3::Sim3;

constexpr int COARSE_CH = 8;    // blocks per pipeline step of the coarse levels' passes (one-system cycle; tuning: 16)
constexpr int F32_CH = 8;       // blocks per pipeline step of the level-0 FP32 passes (tuning: 16)
constexpr int WG = 256;         // 4 wavefronts of 64
constexpr int KB = 4;            // most right-hand sides one PCG solves together (the batch's view)
constexpr int CHAIN_SEG_MAX = 256;  // rows per segment of the chain preconditioner (LDS of k_chain_apply)
constexpr int PCG_GRAPH_ITERS = 16;  // PCG iterations per captured hipGraph (even: parity returns)
constexpr int MAX_GRID = 2048;  // grid cap of the streaming kernels = number of reduction partials
constexpr int SPAN_GRID_MAX = 65536;  // workgroups of the span SpMV (its partials: one pair each)
                                // (256 CUs x 8 workgroups of 4 waves = full occupancy)

// a kernel templated on the number of right-hand sides is instantiated for 1 ... KB: a batch of three must not
// pay for four
#define BATCH_DISPATCH(NS, ...) \
  do {                          \
    if ((NS) == 1) { constexpr int KS = 1; __VA_ARGS__; } \
    else if ((NS) == 2) { constexpr int KS = 2; __VA_ARGS__; } \
    else if ((NS) == 3) { constexpr int KS = 3; __VA_ARGS__; } \
    else { constexpr int KS = 4; __VA_ARGS__; } \
  } while (0)

// Scalars that live in HBM so the PCG loop needs no host round trip per iteration.
struct DevScalars {
  double rz[2];    // gamma = r.z of the previous PCG iteration (ping-pong by parity)
  double alpha[2]; // step length of the previous PCG iteration (ping-pong by parity)
  double rz0;      // r.z at PCG start
  double chi2;     // sum of (robustified) edge chi2
  double scale;    // x.(lambda x + b)
  unsigned long long maxdiag_bits;  // max |H_dd| as raw bits (non-negative doubles order as integers)
  int32_t iter;      // PCG iterations executed
  int32_t max_iter;  // PCG iteration cap
  int32_t done;      // PCG finished (converged, cap reached or breakdown)
  int32_t stop;      // set by the last allowed update; turned into `done` by the next launch
  int32_t fail;      // PCG breakdown (p.q <= 0 or non-finite) or non-SPD diagonal block
  double tol2;       // squared relative tolerance on ||r||_Minv
  double tmp_pq;     // multi-GPU: w.z summed over ranks  } adjacent: ONE 2-double all-reduce
  double tmp_rz;     // multi-GPU: r.z summed over ranks  } per PCG iteration
  double gam_last;   // r.z seen by the last executed step (reported relative residual)
  double lambda;     // damping of the current solve (read by the captured PCG launches)
  long long n_spmv_work;  // PCG SpMV launches that did their work (launches after `done` return at once)
  double trace;           // sum of the scalar diagonal of H (mean |H_dd|: when is a system damping-dominated?)
  // (host) after a solve: ||r||_Minv against the first, by the r.z the last executed step saw, i.e. of the residual
  // BEFORE that step's update; ||r||_2 / ||b||_2 where norms2 left the pair in tmp_pq, tmp_rz; stopped by the cap
  double rel_res() const { return rz0 > 0 ? std::sqrt(std::fabs(gam_last) / rz0) : 0.0; }
  double true_rel() const { return tmp_rz > 0 ? std::sqrt(tmp_pq / tmp_rz) : 0.0; }
  bool capped(double tol) const { return !fail && iter >= max_iter && rel_res() > tol; }
};

// What the host has seen of one system's r.z at its looks into DevScalars, and what that predicts (host only; it
// sizes the chunks of the PCG loop and decides nothing else).  A look after `iter` executed steps carries gam_last =
// r.z of the residual BEFORE step `iter`, i.e. after iter - 1 updates; rz0 is the same quantity before step 1.
struct PcgRate {
  static constexpr int NL = 8, SPAN = 4;
  int k[NL];
  double g[NL];
  int n = 0;
  void look(int iter, double rz0, double gam) {
    if (iter < 1) return;
    if (n == 0) { k[0] = 1; g[0] = std::fabs(rz0); n = 1; }
    if (iter <= k[n - 1]) return;
    if (n == NL) {
      for (int i = 1; i < NL; ++i) { k[i - 1] = k[i]; g[i - 1] = g[i]; }
      --n;
    }
    k[n] = iter; g[n] = std::fabs(gam); ++n;
  }
  // Launches still needed after the last look until the step that sees r.z <= target and raises `done` (that step
  // included), at the reduction per iteration between the last look and the latest one at least SPAN iterations
  // before it (r.z of CG is not monotone: a rate over one or two iterations is noise).  < 0: no rate yet, or none.
  double remaining(double target) const {
    if (n < 2) return -1.0;
    int a = 0;
    for (int i = n - 2; i > 0; --i)
      if (k[i] <= k[n - 1] - SPAN) { a = i; break; }
    const double gb = g[n - 1];
    while (a > 0 && !(g[a] > gb)) --a;  // (r.z went up in between: the rate over a longer stretch)
    const double ga = g[a];
    if (!(ga > 0.0) || !(gb > 0.0) || !(gb < ga) || !(target > 0.0)) return -1.0;
    if (gb <= target) return 0.0;
    const double x = (double)(k[n - 1] - k[a]) * std::log(target / gb) / std::log(gb / ga);
    return std::isfinite(x) ? std::max(x, 0.0) : -1.0;
  }
};

#include "dev_common.hpp"
struct EdgeArgs;  // lm_kernels.hpp

// ------------------------------------------------------------------------------------------
// Engine
// ------------------------------------------------------------------------------------------
static inline int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }
static inline int grid_for(int64_t items, int per_block) {
  const int64_t g = (items + per_block - 1) / per_block;
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, MAX_GRID));
}

class Engine {
 public:
  sim3opt_options opt;
  Structure st;  // host copy of the pattern
  int32_t nv = 0, ne = 0, nb = 0, n = 0, n_active = 0;
  int64_t nnzb = 0;
  bool has_info = false, has_kernel = false;
  hipStream_t stream = nullptr;
  // every device block of init() and of what it calls (the hierarchy, the exchange plans, the ranged arrays), and the
  // few allocated at their first use (d_ptab, d_dl, the kernels' arrays): given back by release_under_device()
  DevArena mem;
  // (small arrays: staged in pinned memory and enqueued; init synchronises once at its end)
  template <typename T>
  hipError_t upload(T*& dptr, const std::vector<T>& h) { return mem.upload(dptr, h, stream, &staged); }
  // graph
  Sim3 *d_states = nullptr, *d_backup = nullptr, *d_meas = nullptr;
  int32_t *d_ev0 = nullptr, *d_ev1 = nullptr, *d_hidx = nullptr, *d_active = nullptr;
  double *d_info = nullptr, *d_kdelta = nullptr;
  uint8_t* d_kkind = nullptr;  // per-edge SIM3OPT_KERNEL_*, allocated with d_kdelta
  // system
  int32_t *d_rowptr = nullptr, *d_colidx = nullptr, *d_incptr = nullptr, *d_wrow = nullptr;
  int span_grid = 0;  // workgroups of the span SpMV
  int32_t *d_slot01 = nullptr, *d_slot10 = nullptr, *d_inc0 = nullptr, *d_inc1 = nullptr;
  double *d_vals = nullptr, *d_scratch = nullptr, *d_b = nullptr, *d_Minv = nullptr;
  // Arrays indexed by a GLOBAL position (block, incidence) of which a rank touches one contiguous range -- the
  // blocks / incidences of its own rows: H, its FP32 copy, the partitioned coarse levels, the assembly scratch --
  // are allocated for that range only (what makes N ranks hold N times the graph): the pointer the kernels index
  // is the virtual base `allocation - lo`; positions outside [lo, hi) are never dereferenced.
  // options.debug_full_arrays: the whole array, everything outside the range filled with 0xFF bytes (NaN as
  // float and as double); check_foreign_ranges() finds a write there, a read shows up as NaN in the results --
  // the test of the ranges (tests/test_distributed_gpu.py).  One rank: lo = 0, hi = total.
  struct RangedArray { void* alloc; size_t elem; int64_t total, lo, hi; };  // (alloc: a block of `mem`)
  std::vector<RangedArray> ranged;
  template <typename T>
  int alloc_ranged(T*& virt, int64_t lo, int64_t hi, int64_t total, std::string& err) {
    total = std::max<int64_t>(total, 1);
    lo = std::max<int64_t>(0, std::min(lo, total));
    hi = std::max(lo, std::min(hi, total));
    T* p = nullptr;
    if (opt.debug_full_arrays) {
      HIPCHK(mem.raw(p, (size_t)total));
      HIPCHK(hipMemset(p, 0xFF, sizeof(T) * (size_t)total));
      if (hi > lo) HIPCHK(hipMemset(p + lo, 0, sizeof(T) * (size_t)(hi - lo)));
      virt = p;
    } else {
      HIPCHK(mem.alloc(p, (size_t)(hi - lo), nullptr));
      virt = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) - sizeof(T) * (size_t)lo);
    }
    ranged.push_back({p, sizeof(T), total, lo, hi});
    return SIM3OPT_OK;
  }
  int check_foreign_ranges(std::string& err);  // (debug_full_arrays only; else a no-op)
  int64_t ranged_bytes() const {               // device bytes of the ranged arrays as allocated
    int64_t b = 0;
    for (const RangedArray& a : ranged) b += (int64_t)a.elem * (opt.debug_full_arrays ? a.total : std::max<int64_t>(a.hi - a.lo, 1));
    return b;
  }
  double *d_x = nullptr, *d_r = nullptr, *d_z = nullptr, *d_p = nullptr, *d_q = nullptr, *d_s = nullptr;
  double *d_part_a = nullptr, *d_part_b = nullptr;
  // chain-segment preconditioner (Sinv lives in d_Minv)
  int32_t *d_sub_first = nullptr, *d_sub_cnt = nullptr;
  double* d_Gm = nullptr;
  bool use_chain = false;
  int chain_seg = 256;
  // aggregation multigrid preconditioner (amg.hpp, amg_kernels.hpp); level 0 aliases the system
  struct AmgLevel {
    int32_t nb = 0;
    int64_t nnzb = 0;
    int32_t *rowptr = nullptr, *colidx = nullptr, *wrow = nullptr;
    int span_grid = 0;
    double *vals = nullptr, *diagH = nullptr, *W = nullptr, *Minv = nullptr;
    float* vals32 = nullptr;  // FP32 copy of vals for the cycle's matrix passes (amg_fp32)
    int32_t *agg = nullptr, *mptr = nullptr, *mem = nullptr, *gptr = nullptr, *gblk = nullptr, *grow = nullptr;
    double *r = nullptr, *x = nullptr, *t = nullptr;  // level right-hand side, iterate, residual / result
    int32_t lo = 0, hi = 0;          // rows this rank's kernels work on: its own (partitioned level) or all
    int32_t own_lo = 0, own_hi = 0;  // rows whose Galerkin blocks / restricted residual this rank forms from the
    int64_t own_b0 = 0, own_b1 = 0;  //   level above (aggregates of its own rows there, or all) and their blocks
  };
  // spans (per rank) of a level's vectors / block values: set where a partitioned level meets a replicated one
  std::vector<std::vector<int64_t>> lvl_offs, lvl_blk_offs;
  std::vector<AmgLevel> amg;
  double *d_P = nullptr, *d_Ainv = nullptr, *d_Ainv2 = nullptr, *d_piv = nullptr, *d_az = nullptr;
  int32_t* d_row2v = nullptr;
  bool use_amg = false, amg_stale = true;
  double amg_omega = 0.9;  // damping of the block-Jacobi smoother: eig(D^-1 A) <= 2 on every level
  int amg_visits[AMG_MAX_LEVELS + 1];  // cycles spent on level l per visit of level l-1 (1 = V, 2 = W)
  bool amg_additive = false;           // level 0 additive: no fine-level matrix pass in the cycle
  bool amg_fp32 = true;                // the cycle's matrix passes stream FP32 copies of the blocks
  // over-correction: the coarse correction prolonged INTO level l is scaled by amg_over_l[l]
  // (piecewise-constant prolongation under-estimates the correction; Stueben / Blaheta)
  double amg_over_l[AMG_MAX_LEVELS + 1];
  double amg_over = 1.0;               // (the factor of the launch being issued)
  bool amg_over_on = true;             // cleared when an over-corrected cycle made the PCG break down
  int amg_pivot = 14;                  // pivot block of the dense coarsest inverse (14 or 28 rows: the same
                                       // total time -- the in-wavefront pivot inverse is what costs)
  // Damping-dominated systems (round 3): when lambda is of the order of the diagonal of H -- the LM
  // trials at the noise floor of the delta = 1e-9 Jacobians, lambda 2e2 ... 8e3 on config 3 -- plain
  // block-Jacobi PCG converges in 3-11 iterations of 0.2 ms, while a multigrid solve pays 2 ms for the
  // dense coarsest inverse plus 0.75 ms per iteration (measured from the same states and lambdas: 1.0-8.6
  // ms against 7.5-35 ms per LM iteration, chi2 equal to the last digit; scripts/gpu_easy_solves.py).  A
  // solve with lambda >= bj_gate therefore starts with block-Jacobi; after 8 iterations the observed
  // reduction says how many it would need, and beyond `bj_budget` the solve starts again with the
  // hierarchy.  The gate follows the outcomes (deterministic: same decisions in every run).
  bool adaptive_prec = true;
  double bj_gate = -1.0;   // lambda from which block-Jacobi is tried first (< 0: 0.05 x mean |H_dd|)
  int bj_budget = 48;      // predicted iterations above which the probe is abandoned
  int n_bj_solves = 0, n_bj_abandoned = 0;
  bool trace_stale = true;
  double mean_diag = 0.0;
  int amg_status = 0;                  // first collective error inside a cycle
  std::string amg_err;
  // ---- whose vectors a multigrid cycle works on: ONE driver (engine_amg.hip) for one and for several systems ----
  struct CycleLevel {
    double *Minv = nullptr, *r = nullptr, *x = nullptr, *t = nullptr;  // per system, strides ms / vs
    float* diag32 = nullptr;  // coarse levels of a batch: every system's damped diagonal blocks, [row][49]
    int64_t vs = 0, ms = 0;   // (one system: the level's own damped blocks, no strides)
  };
  struct CycleView {
    int nsys = 1;            // systems the launches carry (a batch: the first `nsys` of its KB)
    bool batch = false;      // storage for KB systems: per-system diagonals on coarse levels, FP32 passes only
    std::vector<CycleLevel> lv;
    DevScalars* sc = nullptr;     // the systems' scalars (level-0 launches test `done`)
    double* Ainv = nullptr;       // dense inverse(s) of the coarsest level, stride as
    int64_t as = 0;
    double* rz_part = nullptr;    // where the cycle's last level-0 pass leaves the partials of r.z, stride part
    int part = 0;
  };
  CycleView cv_one;    // aliases the AmgLevel arrays (amg_bind)
  CycleView cv_batch;  // the buffers of batch_alloc
  // ---- which system or systems a PCG solve works on: ONE driver (pcg_run, engine_pcg.hip); nsys = 1 on the engine's
  // own vectors is the one-system solve ----
  struct PcgView {
    int nsys = 1;          // systems of this solve: the first `nsys` of the view's nsc
    int nsc = 1;           // scalar slots (and vector slots) the view has: 1, or KB
    bool batch = false;    // the buffers of batch_alloc: the K-system SpMV launch, partials always summed before the step
    double *x = nullptr, *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr, *s = nullptr, *az = nullptr;
    int64_t vs = 0;        // between the systems' vectors
    double* Minv = nullptr;  // level-0 smoother inverses (chain: its factors), stride ms
    int64_t ms = 0;
    const double* b = nullptr;  // right-hand side(s), stride bstride (0: one, shared by the systems)
    int64_t bstride = 0;
    double tol[KB] = {0, 0, 0, 0}, lam[KB] = {0, 0, 0, 0};  // per slot: relative tolerance on ||r||_Minv, damping
    DevScalars *sc = nullptr, *h_sc = nullptr;  // nsc each; h_sc pinned
    double *part_a = nullptr, *part_b = nullptr;  // the SpMV's partials of w.z and r.z, stride pstride
    int pstride = 0;
    CycleView* cv = nullptr;  // the multigrid cycle's view of the same systems
  };
  PcgView pv_one;    // d_x ... d_az, d_sc / h_sc, d_b (init)
  PcgView pv_batch;  // b_x ... b_az, d_bsc / h_bsc (batch_alloc)
  // ---- several right-hand sides at once (engine_pcg.hip): the rejected trials of an LM iteration ----
  DevArena batch_mem;
  double *b_x = nullptr, *b_r = nullptr, *b_z = nullptr, *b_p = nullptr, *b_q = nullptr, *b_s = nullptr, *b_az = nullptr;
  double *b_Ainv = nullptr, *b_diag64 = nullptr, *b_part_a = nullptr, *b_part_b = nullptr;
  int64_t b_vs = 0, b_as = 0;
  DevScalars *d_bsc = nullptr, *h_bsc = nullptr;
  bool batch_ready = false;
  int64_t b_slice_blocks = 100000;  // levels with at most this many blocks run one system per grid slice
  int batch_alloc(std::string& err);
  void batch_release();
  // per system s < nsetup of the batch's view: damped diagonal blocks, smoother inverses, dense coarsest inverse
  void batch_prepare(int nsetup);
  // per-system right-hand sides of a batch (the columns of the inverse): g + s * stride, tolerance tol[s]; one damping
  // for all, so one set-up serves them -- run by the first batch of a call only (setup)
  struct BatchRhs { const double* g; int64_t stride; const double* tol; bool setup; };
  int pcg_batch(const double* lams, int nsys, int32_t* iters, double* rel_res, bool* capped, bool* usable,
                std::string& err, const BatchRhs* cols = nullptr);
  // the solve of LM trial q at damping lambda (ni: the rule's next factor); *x: d_x or its system of a batch
  int lm_trial_solve(int q, double lambda, double ni, const double** x, int32_t* iters, double* rel_res, bool* ok,
                     std::string& err);
  struct TrialBatch {  // the current LM iteration's batch (systems n, the next to hand out) and previous trial's solve
    int n = 0, next = 0;
    double lam[KB], rel[KB];
    int32_t iters[KB], prev_pit = 0;
    bool capped[KB], prev_ok = false, prev_capped = false;
  } trial_batch;
  // most systems a batch may hold for this graph and these options (0: no batching)
  int batch_capacity() const {
    if (!use_amg || use_direct || comm.active() || !amg_fp32 || amg_additive || opt.pcg_batch == 1) return 0;
    return opt.pcg_batch > 1 ? std::min(opt.pcg_batch, KB) : KB;
  }
  // exact sparse block Cholesky (direct_factor.hpp): LinearSolverEigen's role on graphs whose factorisation
  // is cheap (KITTI-00 and other chain-like graphs)
  BlockLdl lm_factor;
  bool use_direct = false;
  int fail_token = 1;  // number of the current exact solve (>= 2): see direct_solve
  // chi2 of the current estimates when it is already known (the last accepted trial computed it)
  bool chi_known = false;
  double chi_cache = 0.0;
  double last_true_rel = 0.0;  // ||r||_2 / ||b||_2 at the end of the last multigrid-preconditioned solve
  bool last_capped = false;    // the last solve stopped at its iteration cap short of the tolerance
  // hipGraph of `graph_iters` PCG iterations (single GPU, untimed runs): replayed per chunk
  hipGraphExec_t pcg_graph = nullptr;
  int pcg_graph_kind = -1;
  int graph_iters = PCG_GRAPH_ITERS;
  DevScalars* d_sc = nullptr;
  DevScalars* h_sc = nullptr;  // pinned
  StagedUploads staged;        // small uploads of init() go through one pinned block, on `stream`
  bool linearized = false;
  // multi-GPU row partition: this rank owns block rows [r0, r1); offs = 7 * row_begin
  Comm comm;
  int32_t r0 = 0, r1 = 0, e_lo = 0, e_hi = 0;
  std::vector<int32_t> row_begin;
  std::vector<int64_t> offs;
  // Row partition of a multigrid level over the ranks (level 0 = the LM system; coarse levels with more than
  // options.amg_shard_rows rows are partitioned too -- aggregates never straddle two ranks, so a rank's coarse
  // rows are the aggregates of its own fine rows).  Vectors of a partitioned level are full-length on every
  // rank; a kernel writes its own rows and reads its own rows plus the rows its blocks' columns name, which
  // exchange_level() refreshes: neighbour-only (grouped send / receive of exactly the rows the other side
  // reads) where the transport can, else the all-gather of the whole vector.
  struct LevelPart {
    int32_t lo = 0, hi = 0;               // rows of this rank
    std::vector<int32_t> row_begin;       // world + 1
    std::vector<int64_t> offs;            // 7 * row_begin (doubles): spans of the whole-vector all-gather
    std::vector<int64_t> blk_offs;        // 49 * rowptr[row_begin]: spans of the level's block values
    bool neighbour = false;               // the neighbour-only plan below is in use
    bool self_test = false;               // one rank, forced collectives: the plan sends a few rows to itself
    int32_t n_send = 0, n_recv = 0;       // rows this rank sends / receives per exchange
    int32_t *d_send = nullptr, *d_recv = nullptr;  // row lists, grouped by peer
    std::vector<int64_t> send_offs, recv_offs;     // world + 1, doubles, into the buffers
    double *d_sbuf = nullptr, *d_rbuf = nullptr;
  };
  std::vector<LevelPart> parts;  // parts[l] for l < n_sharded (world > 1 or forced collectives; else empty)
  int n_sharded = 0;             // multigrid levels [0, n_sharded) are partitioned, the rest replicated
  bool sharded(int l) const { return l < n_sharded; }
  int level_part_init(int l, int32_t nb_l, const int32_t* rowptr_l, const int32_t* colidx_l,
                      const std::vector<int32_t>& row_begin_l, std::string& err);
  // refreshes, on level l, this rank's copy of the foreign rows its own rows read (no-op on one rank)
  int exchange_level(int l, double* vec, std::string& err);
  // timing
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  // phase stamps of an iteration (linearise | solve | update; phase_ms): recorded without waiting, read after
  // the trial's one host round trip (the chi2 fetch)
  hipEvent_t ev_ph[4] = {nullptr, nullptr, nullptr, nullptr};
  // per-iteration phase times (IterStats::ms_*): three event markers per LM trial, ~5.6 us of idle stream each --
  // nothing next to a 25 ms iteration, 7 % of a KITTI-00 one: measured on request (time_kernels, verbose) and
  // on systems of more than 4096 block rows, reported as 0 otherwise
  bool phase_timing = true;
  std::vector<hipEvent_t> pool;  // pairs (start, stop) for per-launch SpMV timing
  size_t pool_used = 0;
  std::vector<hipEvent_t> rep_pool;  // pairs around every visit of the first replicated multigrid level
  size_t rep_used = 0;
  int rep_level = 0;  // first multigrid level a partition over part_world() ranks replicates (0: no hierarchy)
  sim3opt_kernel_times kt{};

  ~Engine() { release(); }

  int device_used = -1;  // the device this engine lives on (init); release() runs under it
  void release();
  void release_under_device();

  // ranks of the row partition the multigrid hierarchy is built for: the communicator's, or -- on one rank --
  // options.amg_virtual_ranks (the hierarchy an N-rank run builds, for comparisons)
  int part_world() const { return comm.world > 1 ? comm.world : std::max(1, opt.amg_virtual_ranks); }
  sim3::Opts mopts() const { return sim3::Opts{opt.exp_eps, opt.small_rot_half, opt.fix_small_angle_b}; }

  EdgeArgs edge_args() const;

  int init(const HostGraph& g, const Structure& s, std::string& err);

  int fetch_scalars(std::string& err) { return fetch_scalars(pv_one, err); }  // the LM's own
  int fetch_scalars(PcgView& V, std::string& err);  // a look with nothing queued behind it: V.h_sc is fresh

  // ---- the PCG loop's schedule (pcg_run) ----
  // The stopping decision is the device's; the host only chooses how many iterations to enqueue before it looks
  // again.  From two looks it has the reduction of r.z per iteration and from that the iterations still needed
  // (PcgRate); chunks are sized by it, and while more than one chunk is predicted the look at chunk k is an
  // asynchronous copy into a pinned slot + an event, waited for with chunk k + 1 already in the queue.  Only one
  // such look is ever outstanding, so there is one slot and one event.
  DevScalars* h_ring = nullptr;  // pinned, KB
  hipEvent_t ring_ev = nullptr;
  // longest multigrid chunk once a rate is known, and the share of the predicted remainder that is enqueued: the
  // prediction is a straight line through a curve that bends either way, and what an iteration too many costs
  // against a look too many is measured in DESIGN.md section 5 (neither value has been tuned)
  static constexpr int sched_cap_mg = 8;
  static constexpr double sched_frac = 0.85;
  // iterations to enqueue now when `rem` more are predicted (rem < 0: no rate -> `fixed`), at most cap
  int sched_chunk(double rem, int fixed, int cap) const {
    if (rem < 0.0) return fixed;
    return std::max(1, std::min(cap, (int)std::floor(sched_frac * rem)));
  }
  // ... and behind them, before the look at them is waited for (0: that look synchronises): half of what is
  // predicted beyond the chunk -- these are enqueued on a rate one chunk older
  int sched_ahead(double left, int cap) const {
    const int c = std::min(cap, (int)std::floor(0.5 * left));
    return c >= 2 ? c : 0;
  }
  // enqueues the copy of nsc DevScalars from `src` into the slot and its event
  int poll_async(const DevScalars* src, int nsc, std::string& err);
  // waits for that event and copies the slot to dst (h_sc or h_bsc)
  int poll_wait(DevScalars* dst, int nsc, std::string& err);
  // since the last reset: {iterations enqueued, enqueued after `done` (enqueued - executed), polls that synchronised
  // with nothing queued behind them, polls waited for with the next chunk queued}
  int64_t sched_stats[4] = {0, 0, 0, 0};

  // ---- timing helpers ----
  int phase_ms(int a, int b, double& acc, std::string& err);  // acc += stamp ev_ph[a] -> ev_ph[b] (both complete)
  int pool_get(hipEvent_t& a, hipEvent_t& b, std::string& err);
  // after a stream sync: fold the recorded SpMV event pairs into the accumulators
  // (h_sc must be fresh).  Launches enqueued after the solve finished return at once; they are
  // left out of the launch count -- their few microseconds stay in the sum, so the average errs on
  // the slow side -- otherwise the per-launch figure would be flattered by up to pcg_check_every - 1
  // empty launches per solve.
  long long spmv_work_seen = 0;
  int pool_drain(std::string& err);

  // ---- aggregation multigrid ----
  // structure of the hierarchy (once per initialize); leaves use_amg false when the graph does
  // not coarsen (block-Jacobi is used then)
  std::vector<AmgLevelHost> amg_host;  // kept between amg_init and amg_bind
  int amg_init(const Structure& s, bool automatic, std::string& err);

  int amg_bind(const Structure& s, std::string& err);

  // numbers of the hierarchy: once per linearisation (P = Ad(S_v) at the linearisation point)
  int amg_setup(std::string& err);

  // per trial: damped diagonal blocks, smoother inverses, dense inverse of the coarsest level
  void amg_prepare(double lambda);

  // The cycle (every step on the view's vectors; launch choices: spmv_mode)
  // a matrix pass of level `level` against its right-hand side: mode 1 out = r - A v, mode 2 out = v + Minv (r - A v),
  // mode 3 (coarse levels): mode 2 on v + xc[agg], the coarser level's correction prolonged on the fly
  void spmv_mode(const CycleView& V, int level, int mode, const double* v, double* out, const double* xc = nullptr);

  void amg_restrict(const CycleView& V, int l, const double* t);
  void amg_prolong(const CycleView& V, int l, const double* xc, const double* xin, double* xout);

  // Solves the level-(l+1) problem approximately (right-hand side lv[l+1].r, first iterate
  // lv[l+1].x = Minv r already there) by amg_visits[l+1] cycles; returns the buffer with the result.
  double* amg_coarse(const CycleView& V, int l);
  double* amg_coarse_body(const CycleView& V, int l);
  void amg_exchange(int l, double* vec);

  // One multigrid cycle on level l from the iterate `cur`; `other` is scratch; returns the buffer
  // that holds the new iterate (always `other`):
  //   t = r - A cur;  coarse correction;  cur += P x_c;  other = cur + Minv (r - A cur)
  double* amg_cycle(const CycleView& V, int l, double* cur, double* other);

  // d_az = M^-1 d_r; on entry d_z = Minv_0 d_r (written by the PCG step).  Multiplicative: one
  // V(1,1) (or W) cycle from that iterate.  Additive on level 0 (no fine-level matrix pass in the
  // preconditioner): M^-1 = D^-1 + P (coarse cycle) P^T.
  // Multi-GPU: level 0 is row-partitioned like the PCG (its matrix passes need the whole iterate:
  // one all-gather of d_z before, one of d_az after; the restricted residual is all-reduced), the
  // coarse levels are replicated and every rank runs the same coarse cycle.
  int amg_apply(std::string& err);

  // ---- exact sparse block Cholesky ----
  // plan (host, once per initialize) + buffers; leaves use_direct false when the factorisation
  // would be too expensive (the PCG takes over) unless the caller insists
  int direct_init(const Structure& s, std::string& err);

  // (H + lambda I) x = b, exactly; x in d_x.  A non-positive pivot raises d_sc->fail (read by the
  // caller together with the trial's chi2: no extra round trip).
  int direct_solve(double lambda, std::string& err);

  // Diagnostic (sim3opt_debug_factor): gather, factor and, when asked, the selected inversion of context 0 (lm_factor)
  // or 1 (marg_factor) on the last linearisation or on injected values, read out; see include/sim3opt.h
  int debug_factor(int32_t context, double lambda, const double* vals, const double* b, bool with_solve,
                   bool with_selinv, double* Aperm, double* bp, double* L, double* Dinv, double* y, double* xp, double* x,
                   int32_t* fail, double* Z, int32_t* singular, int32_t* bord, int32_t* brow, std::string& err);

  // ---- marginal covariances: blocks of (H + lambda I)^-1 by a selected inversion (selinv.cpp,
  // selinv_kernels.hpp) ----
  // A context of its own -- plan, factor, flag -- whatever linear solver the LM uses, built at the first
  // call: the LM's buffers and scalars are never written, so a call between two optimize() calls leaves
  // the second one as it was (the relinearisation it does is repeated by every LM iteration anyway).
  BlockLdl marg_factor;
  std::vector<int32_t> mpos;  // block row of H -> column of L
  std::string marg_refused;  // why the plan was refused (the call fails the same way every time)
  int marginal_init(std::string& err);
  // cov[q] (column-major 7x7) = block (row_a[q], row_b[q]) of (H + lambda I)^-1, H linearised at the current
  // estimates; rows are block rows of H (free vertices)
  int marginals(double lambda, int32_t n, const int32_t* row_a, const int32_t* row_b, double* cov,
                std::string& err);
  // the same for marginals (any_pair false), covariances (any pair) and the gate (fixed_zero: row -1 = zero block)
  int cov_blocks(const char* who, bool any_pair, bool fixed_zero, double lambda, int32_t n, const int32_t* row_a,
                 const int32_t* row_b, double* cov, std::string& err);
  // of the last cov_blocks: chunks, root paths walked, distinct pairs outside the pattern, pairs on it, workspace
  // bytes, selected inversion run (sim3opt_covariance_stats)
  int64_t cov_stats[6] = {0, 0, 0, 0, 0, 0};
  int gate_edges(double lambda, int32_t n, const int32_t* v0, const int32_t* v1, const int32_t* row0,
                 const int32_t* row1, const Sim3* meas, const double* infoinv, double* e_out, double* S_out,
                 double* d2_out, std::string& err);  // gate_kernels.hpp
  // ---- the same blocks by columns of the inverse (engine_columns.hip, col_kernels.hpp): graphs too large to factor ----
  // options.cov_solver = 1, or 2 where the marginal plan is refused: block (a, b) is rows a of the seven solutions
  // (H + lambda I) y = e_{7 b + c}, by the PCG the graph was initialised with -- on a multigrid graph up to KB columns
  // per pass over the blocks (pcg_batch with per-system right-hand sides and ONE set-up), else one at a time
  // (pcg_attempt) -- each checked on the device by its TRUE residual in the 2-norm against options.cov_rel_tol and
  // refined at most twice.  The solver's state is put back as the diagnostic read-outs do (SolverSnapshot).
  DevArena cols_mem;
  double *c_g = nullptr, *c_y = nullptr, *c_r = nullptr, *c_d = nullptr;  // KB right-hand sides, solutions, residuals, refinement right-hand sides
  double* c_nrm = nullptr;  // [||r||^2, ||g||^2] per system
  int64_t c_vs = 0;
  int cols_alloc(std::string& err);
  void cols_release();
  // columns a solve carries: KB (or options.pcg_batch) through the batch on a multigrid graph that admits one, else 0
  int cols_batch_width() const {
    if (!use_amg || amg.empty() || comm.active() || !amg_fp32 || amg_additive) return 0;
    return opt.pcg_batch >= 1 ? std::min(opt.pcg_batch, KB) : KB;
  }
  // solves nsys systems for the right-hand sides g + s * c_vs to the tolerances tol[s] (||r||_Minv); x[s]: where the
  // solution of system s is; failed[s]: breakdown or a failed set-up pivot
  int cols_solve(double lambda, int nsys, const double* g, const double* tol, bool setup, const double** x,
                 int32_t* iters, bool* failed, std::string& err);
  // ||g_s - (H + lambda I) y_s||_2 / ||g_s||_2 of the systems listed, by the SpMV (the residual itself: c_r)
  int cols_true_residuals(double lambda, int cnt, const int* sys, double* rel, std::string& err);
  // The columns of block rows vertices[0 .. nvert): vertex v contributes the blocks [first[v], first[v + 1]), block k =
  // (blk_row[k], vertices[v]) of the inverse, column-major, into blocks (host, 49 doubles each).  Nothing is written
  // unless every column met options.cov_rel_tol.
  int inverse_columns(double lambda, int32_t nvert, const int32_t* vertices, const int32_t* first,
                      const int32_t* blk_row, double* blocks, std::string& err);
  int cov_blocks_columns(const std::string& pre, bool fixed_zero, double lambda, int32_t n, const int32_t* row_a,
                         const int32_t* row_b, double* cov, std::string& err);
  // of the last column call: {vertices solved, columns, PCG iterations summed over the columns, refinement rounds,
  // batches}, {largest true relative residual, cov_rel_tol used}; the vertex (index) of a column that failed, or -1
  int64_t col_counts[5] = {0, 0, 0, 0, 0};
  double col_res[2] = {0.0, 0.0};
  int32_t col_fail_vertex = -1;
  // block-Jacobi inverses Minv = omega (D + lambda W)^-1 of rows [lo, hi) (k_jacobi; engine_pcg.hip)
  void jacobi(int lo, int hi, const int32_t* rowptr, double* vals, double lambda, double* Minv, double omega,
              const double* diagH, const double* W, float* vals32, DevScalars* sc = nullptr,
              double* diag64_out = nullptr, float* diag32_out = nullptr);
  void norms2(const double* r, const double* b, double* part_a, double* part_b, double* out2);  // engine_pcg.hip
  void dense_inverse(const double* diag64, double* Aout, DevScalars* sc);                         // engine_amg.hip

  // every rank's copy of `vec` gets the entries of the rows its own rows' blocks refer to: the boundary
  // rows only (halo exchange) where the partition has locality, the whole vector otherwise
  int exchange_rows(double* vec, std::string& err) { return exchange_level(0, vec, err); }

  // ---- building blocks ----
  // scale_parts > 0: d_part_b holds that many partial sums of the trial's scale (k_scale): summed in the
  // same launch as chi2's
  int chi2(double* out, std::string& err, hipEvent_t before_fetch = nullptr, int scale_parts = 0, int grid = 0);

  // the perturbation table of the numeric Jacobians, re-evaluated when delta or the arithmetic options change
  Sim3* d_ptab = nullptr;
  double ptab_delta = 0.0;
  sim3::Opts ptab_opts{0.0, -1, -1};

  int linearize(std::string& err);

  // SpMV variant (tuning knob, env SIM3OPT_SPMV="chunk,nt"; defaults chosen by measurement,
  // scripts/gpu_spmv_ab.py: 8 blocks per pipeline step, non-temporal block stream)
  int spmv_chunk = 8, spmv_nt = 1;

  int spmv_grid() const { return span_grid; }

  // q = (H + lambda I) v; partials of v.q in d_part_a and, with rvec, of rvec.v in d_part_b
  // With a start/stop event pair the dispatch itself is timestamped (hipExtLaunchKernelGGL):
  // no extra barrier packets, so the figure agrees with rocprofv3's kernel trace.
  void spmv_raw(double lambda, const double* v, double* q, const double* rvec, DevScalars* scp,
                hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

  // the PCG's SpMV on a view's first `live` systems: V.q = (H + lambda_s I) v, partials of v.q and, with rvec, of
  // rvec.v in V.part_a / V.part_b (timed: one system with options.time_kernels takes an event pair from the pool)
  int pcg_spmv(const PcgView& V, int live, const double* v, const double* rvec, bool timed, std::string& err);

  // Preconditioned CG on (H + lambda I) x = b in the single-reduction form (k_pcg_step); the
  // result stays in d_x.  Two launches and one reduction point per iteration; the host only polls
  // a 100-byte struct every `pcg_check_every` iterations.
  int agree_on_fail(std::string& err);

  int pcg(double lambda, int32_t* iters, double* rel_res, bool* ok, std::string& err);

  // prec: 0 block-Jacobi, 1 chain segments, 2 aggregation multigrid
  // probe_budget > 0 (block-Jacobi tried first on a damping-dominated system): after 8 iterations the
  // reduction reached so far predicts the total; if that exceeds the budget -- or the budget runs out --
  // *abandoned is set and the caller solves again with the hierarchy
  int pcg_attempt(double lambda, int prec, int32_t* iters, double* rel_res, bool* ok,
                  bool* chain_broke, std::string& err, int probe_budget = 0, bool* abandoned = nullptr,
                  const double* rhs = nullptr, double rel_tol = 0.0);
  int pcg_setup(PcgView& V, int prec, int nsetup, std::string& err);
  // The solve itself, on the systems of V (V.lam, V.tol, V.b set by the caller): scalars reset, set-up of
  // preconditioner `prec` (a batch: of its first nsetup systems), first residual, the look at the set-up's pivots
  // (*setup_broke: a non-positive one, nothing was iterated), the loop, with check_true the 2-norm of every residual
  // against its right-hand side's (the pair in tmp_pq, tmp_rz), and V.h_sc holds the systems' last state.  What only one system does -- graph replay, several
  // ranks, the probe, timed launches, partials summed inside the step -- is keyed on the view.
  int pcg_run(PcgView& V, int prec, int nsetup, bool check_true, bool* setup_broke, std::string& err,
              int probe_budget = 0, bool* abandoned = nullptr);

  // ---- diagnostic read-outs of the preconditioners (tests/test_gpu_preconditioners.py; one GPU only) ----
  // They run the set-up a PCG solve runs between SolverSnapshot::take and put_back (below).  Everything else they
  // touch -- the level numbers for a lambda, d_Minv, the PCG vectors -- is rewritten by every solve before it is
  // read, and amg_setup is a function of the linearisation alone, so a solve or optimize() that follows is bit for
  // bit the one without the read-out.
  // the PCG fields of a view's V.nsc scalars as a solve sets them: the first nrhs not done, at lambda[k], the rest
  // finished (after a take(): `from` is the snapshot's device copy of them)
  int diag_begin(PcgView& V, const double* lambda, int nrhs, const DevScalars* from, std::string& err);
  // amg_setup if stale, amg_prepare(lambda) -- as a solve -- and, unlike it, a failed pivot is SIM3OPT_ERR_STATE
  int amg_numbers(double lambda, std::string& err);                                      // engine_amg.hip
  int amg_level_readout(double lambda, int32_t level, int32_t* rowptr, int32_t* colidx, double* vals, float* vals32,
                        double* W, double* diagH, double* Minv, double* P, std::string& err);  // engine_amg.hip
  int amg_coarsest_inverse(double lambda, double* Ainv, std::string& err);                // engine_amg.hip
  // z[q] = M^-1 r[q] for nrhs right-hand sides with ONE set-up: the launches of a PCG iteration (engine_pcg.hip)
  int precond_apply(int prec, double lambda, int32_t nrhs, const double* r, double* z, std::string& err);
  // ---- ... and of the PCG's own operator (tests/test_gpu_pcg_operator.py) ----
  // the span table as the device holds it (a copy: nothing is written)
  int spmv_spans(int32_t* n_spans, int32_t* wrow, std::string& err);                      // engine_pcg.hip
  // q = (H + lambda I) p with p.q and rvec.p: the SpMV launch of a PCG iteration (pcg_spmv) and the sum of its partials,
  // on the one-system view or, nrhs > 1, on the batch's.  The partials are added by k_final_sum2: the FUNCTION a solve
  // adds them with (sum_partials on the same arrays, count and block size), not always the launch -- up to MAX_GRID
  // partials the one-system k_pcg_step adds them in-step.  With rvec the K-system launch takes a path a batched solve
  // never takes (its r.z comes from the cycle): diagnostic only.  The vectors staged in are rewritten by every solve.
  int operator_apply(int32_t nrhs, const double* lambda, const double* p, const double* rvec, double* q, double* pq,
                     double* rp, std::string& err);                                      // engine_pcg.hip

  // ---- the iteration frame of LM, Gauss-Newton and dogleg (engine.hip) ----
  int iter_begin(sim3opt_iter_stats& T, double& chi, std::string& err);  // stamp 0, chi2 (cached or not), linearise
  void iter_end(sim3opt_iter_stats& T, double chi, std::vector<sim3opt_iter_stats>& stats);  // cache chi, record T
  bool direct_rejected() const;  // after the caller's fetch: the exact factorisation met a non-positive pivot
  bool lin_dump = false;  // linearize() launches the DUMP instantiation (sim3opt_debug_linearization sets d_lin_dump first)
  void apply_step(const double* x, bool push);  // k_oplus; push: the old estimates into d_backup first
  void pop_states();                            // k_copy_states from d_backup

  int optimize(int32_t max_iters, std::vector<sim3opt_iter_stats>& stats, std::string& err);

  // ---- Gauss-Newton and Powell's dogleg (engine_algorithms.hip) ----
  // optimize() clears the stats and the chi2 cache, then hands options.algorithm = 1 / 2 to these
  int optimize_gauss_newton(int32_t max_iters, std::vector<sim3opt_iter_stats>& stats, std::string& err);
  int optimize_dogleg(int32_t max_iters, std::vector<sim3opt_iter_stats>& stats, std::string& err);
  // g2o's Fail: iteration `it` is recorded with the estimates it started from; optimize() returns 0
  int fail_iteration(int it, sim3opt_iter_stats& T, double chi, std::vector<sim3opt_iter_stats>& stats,
                     const char* why, std::string& err);
  // the six per-iteration scalars of the dogleg model from b (d_b) and h_gn (d_x): two SpMVs with lambda = 0 and
  // one fused dot kernel, all-reduced over the ranks; left on the device in d_dl (no host round trip here)
  // grid > 0: that many workgroups (= partials per dot) for k_dl_dots instead of the rule's; j1 >= 0: its entries
  // [j0, j1) instead of this rank's rows' (both for sim3opt_debug_dogleg only)
  int dogleg_dots(std::string& err, int grid = 0, int64_t j0 = 0, int64_t j1 = -1);
  int dogleg_alloc(std::string& err);       // d_dl / h_dl at their first use; refuses without the SpMV's launch state
  void dogleg_step(double ca, double cg);   // k_dogleg_oplus: backup <- S, S <- exp(ca b + cg h_gn) S
  // Diagnostic (sim3opt_debug_dogleg): the launches of a dogleg iteration after its solve on a caller's h_gn
  int debug_dogleg(const double* h_gn, double ca, double cg, bool with_fail, int32_t grid, int64_t j0, int64_t j1,
                   double* scalars, double* states_out, double* backup_out, std::string& err);
  // Diagnostic (sim3opt_debug_column_vectors): one of the four column kernels on a caller's data (engine_columns.hip)
  int debug_column_vectors(int32_t op, int32_t grid, int64_t nvec, int32_t K, const int64_t* at, int32_t sys,
                           const double* a, const double* b, int32_t first, int32_t count, int32_t col,
                           const int32_t* rows, int32_t n_blocks, double* out, std::string& err);
  std::vector<sim3opt_tr_stats> tr_stats;  // per iteration of the last dogleg run
  double* d_dl = nullptr;  // dogleg: 4 x MAX_GRID dot partials, then the 8 scalars (DL_OUT), DL_DOUBLES in all
  double* h_dl = nullptr;  // pinned copy of the scalars
};
constexpr size_t DL_DOUBLES = 4 * MAX_GRID + 16;

// What a read-out that runs the solver's own launches puts back, so that the next solve or optimize() is the one
// without it: the one-system scalars on the device and in h_sc, the batch's KB scalars on both sides once the batch
// exists, and the host's counters and caches -- kt, sched_stats, spmv_work_seen, last_true_rel, last_capped, chi_known,
// chi_cache.  With `vectors` also what the dogleg's launches write outside the scalars: d_x, d_p, d_q, the SpMV's
// partials d_part_a and, once allocated, d_dl (a solve rewrites the first four before it reads them; the read-out
// that stages a caller's h_gn in d_x puts them back all the same).  (engine_pcg.hip)
struct SolverSnapshot {
  int take(Engine& e, std::string& err, bool vectors = false);  // synchronises the stream first
  DevBuf<double> vec;  // the saved vectors, in the order above
  // rc: what happened in between; returned unless it was fine and the restoring failed
  int put_back(int rc, std::string& err);
  Engine* eng = nullptr;
  bool batch = false, has_dl = false;
  DevScalars d_one, h_one, d_batch[KB], h_batch[KB];
  sim3opt_kernel_times kt;
  int64_t sched[4];
  long long work_seen;
  double true_rel, chi_cache;
  bool capped, chi_known;
};

}  // namespace sim3opt
