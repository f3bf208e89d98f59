/*
 * sim3opt.h -- C-ABI of libsim3opt: MI355X-native Sim(3) pose-graph LM optimiser.
 *
 * Drop-in boundary for the path  optimizer.initializeOptimization();
 * optimizer.optimize(100);  of the reference (kitti_surf.cpp:674-675, :1044-1045)
 * on graphs of vio::VertexSim3Expmap / vio::EdgeSim3.  Each entry point names the
 * g2o call of the reference it replaces.  Plain pointers and sizes only; the
 * library copies everything it is given (the caller keeps no pointers into it).
 *
 * Conventions crossing the boundary:
 *   Sim3 state      8 doubles [qx qy qz qw tx ty tz s]   (Eigen coeffs() order, kitti_surf.cpp:698)
 *   tangent order   [omega(3), upsilon(3), sigma]        (g2o)
 *   information     7x7 double, column-major, NULL = identity (kitti_surf.cpp:592, :637, :667)
 *   vertex ids      arbitrary int32 (g2o allows any), mapped internally
 *   errors          int status codes, no exceptions, no abort(); text via sim3opt_last_error
 *
 * All computation runs on the GPU (HIP, gfx950).  There is no CPU fallback: if no
 * HIP device is usable, sim3opt_initialize returns SIM3OPT_ERR_NO_DEVICE.
 *
 * Several GPUs: one process per GPU with a communicator handed in (sim3opt_comm_init,
 * sim3opt_comm_init_callbacks), or one single-threaded caller and the ranks inside the library
 * (sim3opt_set_devices, sim3opt_rank_count, sim3opt_local_rows_of_rank, sim3opt_device_bytes_of_rank).
 */
#ifndef SIM3OPT_H
#define SIM3OPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sim3opt_graph sim3opt_graph;

enum {
  SIM3OPT_OK = 0,
  SIM3OPT_ERR_ARG = -1,        /* bad argument (null, unknown id, duplicate id, ...) */
  SIM3OPT_ERR_STATE = -2,      /* call order (e.g. optimize before initialize)       */
  SIM3OPT_ERR_NO_DEVICE = -3,  /* no usable HIP device                               */
  SIM3OPT_ERR_HIP = -4,        /* a HIP runtime call failed                          */
  SIM3OPT_ERR_IO = -5,         /* file could not be read / parsed                    */
  SIM3OPT_ERR_COMM = -6        /* communicator failure (RCCL, or a rank of the process) */
};

/* Robust kernels of an edge (g2o RobustKernel*, robust_kernel_impl.cpp).  rho(e2) and w = rho'(e2) at
 * e2 = e^T Omega e, d = the kernel's delta:
 *   NONE           e2                                              1
 *   HUBER          e2 <= d^2: e2;  else 2 d sqrt(e2) - d^2          1;  d / sqrt(e2)
 *   PSEUDO_HUBER   2 d^2 (sqrt(1 + e2/d^2) - 1)                    1 / sqrt(1 + e2/d^2)
 *   CAUCHY         d^2 log(1 + e2/d^2)                             1 / (1 + e2/d^2)
 *   GEMAN_MCCLURE  d e2 / (d + e2)                                 d^2 / (d + e2)^2
 *   WELSCH         d^2 (1 - exp(-e2/d^2))                          exp(-e2/d^2)
 *   FAIR           2 d^2 (a - log(1 + a)),  a = sqrt(e2) / d       1 / (1 + a)
 *   TUKEY          e2 <= d^2: d^2/3 (1 - (1 - e2/d^2)^3); else d^2/3   (1 - e2/d^2)^2;  0
 *   SATURATED      e2 <= d^2: e2;  else d^2                        1;  0
 *   DCS            s = 2d / (d + e2);  s >= 1: e2;  else s^2 e2    1;  s^2
 * Geman-McClure and DCS take d unsquared (as g2o); DCS's rho is not the integral of its w (g2o's definition).
 * First order, as g2o: an edge contributes w J^T Omega J and -w J^T Omega e, chi2 sums rho, rho'' is ignored.
 * Every kind but NONE needs a finite delta > 0. */
enum { SIM3OPT_KERNEL_NONE = 0, SIM3OPT_KERNEL_HUBER = 1, SIM3OPT_KERNEL_PSEUDO_HUBER = 2,
       SIM3OPT_KERNEL_CAUCHY = 3, SIM3OPT_KERNEL_GEMAN_MCCLURE = 4, SIM3OPT_KERNEL_WELSCH = 5,
       SIM3OPT_KERNEL_FAIR = 6, SIM3OPT_KERNEL_TUKEY = 7, SIM3OPT_KERNEL_SATURATED = 8,
       SIM3OPT_KERNEL_DCS = 9 };

/* Solver configuration.  Replaces the reference's
 *   OptimizationAlgorithmLevenberg(BlockSolverX(LinearSolverEigen))   kitti_surf.cpp:552-558
 * and g2o's setUserLambdaInit / setMaxTrialsAfterFailure            kittiDetector.h:730, 779-782.
 * Defaults (sim3opt_options_default) are g2o's. */
typedef struct sim3opt_options {
  double tau;               /* 1e-5  lambda0 = tau * max|H_dd|                           */
  double user_lambda_init;  /* 0     > 0 overrides the tau rule                          */
  double good_step_lower;   /* 1/3                                                       */
  double good_step_upper;   /* 2/3                                                       */
  int32_t max_trials;       /* 10    maxTrialsAfterFailure                               */
  double fd_delta;          /* 1e-9  central-difference step of the numeric Jacobians (g2o's
                                        BaseBinaryEdge default; 1e-6 gives 1e-10-accurate Jacobians) */
  double exp_eps;           /* 1e-5  branch threshold of exp/log (sim3_rv.h:133)         */
  int32_t small_rot_half;   /* 0     R = I+W+W^2 (sim3_rv.h:151); 1: I+W+W^2/2           */
  int32_t fix_small_angle_b;/* 0     B coefficient as written in sim3_rv.h:166/:290 (reference
                                        behaviour); 1: exact small-theta limit               */
  int32_t dof_mask;         /* 127   bit d set = tangent component d ([w0 w1 w2 u0 u1 u2 s]) is
                                        optimised; cleared bits freeze it (0x78 = rotations frozen:
                                        the scale+translation stage, kitti_surf.cpp:1020-1024)    */
  int32_t pcg_max_iters;    /* 0 = automatic: 2n for n = 7*free vertices <= 50000, else 1000 */
  double pcg_rel_tol;       /* 1e-10 stop when ||r||_Minv <= tol * ||b||_Minv            */
  int32_t pcg_check_every;  /* 16    most PCG iterations between two looks of the host at the solver's state (the
                                        first chunk of a multigrid solve: at most 4, its iterations are ~1 ms
                                        each); later chunks are sized by the iterations still predicted
                                        (sim3opt_pcg_schedule_stats).  1 = one iteration per look, no prediction */
  int32_t pcg_graph;        /* 1     replay the PCG iterations from a captured hipGraph (single GPU,
                                        time_kernels = 0); 0 = enqueue every launch               */
  int32_t preconditioner;   /* -1    0 = 7x7 block-Jacobi, 1 = block-tridiagonal chain segments,
                                       2 = aggregation multigrid (pairwise-matched aggregates,
                                       Ad(S_v)-transported prolongation, dense coarsest level),
                                       -1 = automatic: multigrid when the graph has more than 256
                                       free vertices and coarsens like a low-dimensional graph
                                       (level-1 blocks <= 0.3 x level-0 blocks: chains, chains with
                                       loops, Manhattan worlds -- not expanders), chain segments for
                                       smaller nearly pure chains (well-posed arithmetic only), else
                                       block-Jacobi                                                */
  int32_t chain_segment;    /* 256   rows per chain segment (2..256)                             */
  int32_t device;           /* -1    HIP device ordinal; -1 = current device             */
  int32_t verbose;          /* 0     1: one stderr line per LM iteration (setVerbose)    */
  int32_t time_kernels;     /* 0     1: bracket every SpMV / linearise launch with HIP events
                                        (sim3opt_get_kernel_times); small launch-gap cost    */
  int32_t linear_solver;    /* -1    how (H + lambda I) dx = b is solved (LinearSolverEigen's role,
                                        kitti_surf.cpp:553-554):
                                        1 = exact sparse block Cholesky on the GPU (nested-dissection
                                            order, level-scheduled; the reference's SimplicialLDLT),
                                        0 = preconditioned CG (see `preconditioner`),
                                       -1 = automatic: the exact factorisation when it is cheap (single
                                            GPU, at most ~3e5 7x7x7 block products per factorisation:
                                            KITTI-00 and other chain-like graphs) and no
                                            `preconditioner` was named, else the PCG                */
  /* ---- tuning of the PCG path that changes its NUMERICS (iteration counts, summation orders; the
   * solution it converges to is the same).  Read by sim3opt_initialize.  0 / negative = the default
   * rule where stated.  A SIM3OPT_* environment variable of the same name overrides the field at
   * sim3opt_initialize (debug aid); sim3opt_get_options then reports the value that was used. ---- */
  int32_t amg_cycle[4];     /* 0,..  visits of multigrid level 1, 2, 3, >= 4 per visit of the level above
                                        (1 = V, 2 = W, 3); all 0 = automatic: {2,3,3,3}, or {1,2,2,2} when level 0
                                        is partitioned over the ranks (the coarse cycle is what stays
                                        latency-bound when level 0 is sharded)  [SIM3OPT_AMG_CYCLE] */
  int32_t amg_passes[3];    /* 0,..  pairwise-matching passes on level 0, 1, >= 2 (aggregates of 2^passes rows);
                                        0 = automatic: 3, or 2 on level 0 of a graph that reaches the dense level
                                        that way                                              [SIM3OPT_AMG_PASSES] */
  int32_t amg_additive;     /* 0     1: additive level 0 (no level-0 matrix pass in the cycle) [SIM3OPT_AMG_ADDITIVE] */
  int32_t amg_fp32;         /* 1     the cycle's matrix passes stream FP32 copies of the blocks [SIM3OPT_AMG_FP32] */
  int32_t amg_pivot;        /* 14    pivot rows of the dense coarsest inverse (14 or 28)       [SIM3OPT_AMG_PIVOT] */
  int32_t amg_coarsest;     /* 256   most block rows of the dense coarsest level (8..256)      [SIM3OPT_AMG_COARSEST] */
  int32_t adaptive_prec;    /* 1     automatic preconditioner only: damping-dominated solves start with
                                        block-Jacobi (DESIGN.md 5a')                           [SIM3OPT_ADAPTIVE_PREC] */
  int32_t row_order;        /* -1    block-row order: 0 = insertion (g2o's hessianIndex), 1 = breadth-first
                                        locality order, -1 = automatic (insertion on one rank, locality order
                                        when partitioned)                                      [SIM3OPT_ROW_ORDER=insertion|bfs] */
  int32_t halo_exchange;    /* 1     partitioned runs exchange boundary rows only; 0 = whole-vector all-gather
                                                                                               [SIM3OPT_NO_HALO] */
  int32_t span_grid;        /* 0     workgroups of the span SpMV (four row spans each); 0 or less = automatic (so is
                                        SIM3OPT_SPAN_GRID=0); a positive value is a REQUEST, clamped at every
                                        sim3opt_initialize to 8 .. min((rows + 3) / 4, 65536) of that graph (of this
                                        rank's rows when partitioned).  sim3opt_get_options reports the value in use;
                                        the request is kept, and handing the reported value back to
                                        sim3opt_set_options leaves it as it was                [SIM3OPT_SPAN_GRID] */
  int32_t force_collectives;/* 0     1: run every collective of the partitioned path even with one rank
                                        (transport self-test)                                  [SIM3OPT_FORCE_COMM] */
  int32_t amg_shard_rows;   /* 4096  partitioned runs: multigrid levels with more block rows than this are
                                        partitioned by owner like level 0 (aggregates never straddle ranks), smaller
                                        ones are replicated                                  [SIM3OPT_AMG_SHARD_ROWS] */
  int32_t amg_virtual_ranks;/* 0     > 1 on ONE rank: build the hierarchy as an N-rank partition would (aggregates
                                        inside N equal row spans): what a partitioned run is compared with
                                                                                               [SIM3OPT_AMG_VIRTUAL_RANKS] */
  int32_t pcg_batch;        /* 0     most right-hand sides solved together when LM trials are rejected in a row
                                        (DESIGN.md 5d); 0 = automatic, 1 = one at a time          [SIM3OPT_PCG_BATCH] */
  double amg_omega;         /* 0.9   damping of the block-Jacobi smoother (0.1..0.95)          [SIM3OPT_AMG_OMEGA] */
  double amg_over[2];       /* 1.8, 1.6  over-correction of the coarse correction prolonged into level 0 / into
                                        deeper levels                                          [SIM3OPT_AMG_OVER=a0,a1] */
  int64_t direct_max_pairs; /* 0     most 7x7x7 block products of a factorisation the automatic rule accepts;
                                        0 = 300000 (3e7 with linear_solver = 1)               [SIM3OPT_DIRECT_MAX_PAIRS] */
  int32_t debug_full_arrays;/* 0     partitioned runs allocate the block arrays (H, its FP32 copy, the partitioned
                                        coarse levels, the assembly scratch) for the rank's own rows only; 1: whole
                                        arrays with everything outside the rank's range poisoned (0xFF = NaN) and
                                        checked after every linearisation / optimize -- a write there is an error,
                                        a read shows as NaN (the test of the ranges)          [SIM3OPT_DEBUG_FULL_ARRAYS] */
  int32_t jacobians;        /* 0     how the linearisation differentiates EdgeSim3's residual: 0 = central differences
                                        with step fd_delta (g2o's BaseBinaryEdge default: the reference's arithmetic),
                                        1 = closed form, J = +-J_l(e)^-1 Ad (DESIGN.md "Analytic Jacobians"); needs
                                        fix_small_angle_b = 1 (sim3opt_set_options refuses it with the as-written B) */
  /* nonlinear algorithm (g2o's OptimizationAlgorithm* behind SparseOptimizer::setAlgorithm) */
  int32_t algorithm;        /* 0     SIM3OPT_ALGORITHM_LM (Levenberg), _GAUSS_NEWTON, _DOGLEG (Powell)           */
  int32_t dl_max_trials;    /* 100   dogleg: trials per iteration (maxTrialsAfterFailure)                        */
  double dl_delta_init;     /* 1e4   dogleg: trust radius at the first iteration of an optimize() (setUserDeltaInit) */
  double dl_lambda_init;    /* 1e-7  dogleg: first damping once H has not been positive definite (initialLambda)  */
  double dl_lambda_factor;  /* 10    dogleg: factor of that damping (setLamdbaFactor)                            */
  double cov_workspace_mb;  /* 256   sim3opt_covariances / sim3opt_gate_edges: most device memory [MiB], at least 1, for
                                     the root paths of L^-1 behind the blocks outside the factor's pattern; a larger
                                     request is worked off in chunks (same bits)  [SIM3OPT_COV_WORKSPACE_MB]          */
  int32_t cov_solver;       /* 0     how sim3opt_covariances / sim3opt_gate_edges obtain blocks of (H + lambda I)^-1:
                                     0 = the exact factorisation (refused on graphs too large to factor), 1 = columns
                                     of the inverse by PCG (needs a graph on the PCG path, linear_solver 0), 2 = exact
                                     where the marginal plan is accepted, columns where it is refused.  sim3opt_marginals
                                     and sim3opt_marginal_covariances are always exact            [SIM3OPT_COV_SOLVER] */
  double cov_rel_tol;       /* 1e-8  cov_solver 1 / 2: every solved column y of a right-hand side g satisfies
                                     ||g - (H + lambda I) y||_2 <= cov_rel_tol ||g||_2 (true residual, checked on the
                                     device), else SIM3OPT_ERR_STATE; finite, in (0, 1e-2]       [SIM3OPT_COV_REL_TOL] */
} sim3opt_options;

/* options.algorithm */
enum {
  SIM3OPT_ALGORITHM_LM = 0,
  SIM3OPT_ALGORITHM_GAUSS_NEWTON = 1,
  SIM3OPT_ALGORITHM_DOGLEG = 2
};

/* dogleg step types, numbered as g2o's OptimizationAlgorithmDogleg enum */
enum {
  SIM3OPT_STEP_UNDEFINED = 0,
  SIM3OPT_STEP_SD = 1,  /* steepest descent, cut to the trust radius */
  SIM3OPT_STEP_GN = 2,  /* the Gauss-Newton step                     */
  SIM3OPT_STEP_DL = 3   /* between the two, on the trust radius      */
};

/* Per-iteration record of a dogleg run (options.algorithm = SIM3OPT_ALGORITHM_DOGLEG). */
typedef struct sim3opt_tr_stats {
  double delta_before;  /* trust radius at the start of the iteration */
  double delta_after;   /* ... and after its last trial               */
  double alpha;         /* b.b / (b^T H b): h_sd = alpha b            */
  double norm_sd;       /* ||h_sd||                                   */
  double norm_gn;       /* ||h_gn||                                   */
  double norm_dl;       /* ||h_dl|| of the last trial                 */
  int32_t step;         /* SIM3OPT_STEP_* of the last trial           */
  int32_t was_pd;       /* 1: every GN solve so far, this one included, succeeded without damping */
} sim3opt_tr_stats;

/* Per-iteration record (g2o G2OBatchStatistics role; bal_example.cpp:55-56). */
typedef struct sim3opt_iter_stats {
  double chi2_before;
  double chi2_after;
  double lambda;        /* after the iteration's policy update */
  double rho;           /* last gain ratio                     */
  int32_t trials;       /* LM trials used                      */
  int32_t pcg_iters;    /* PCG iterations summed over trials   */
  double pcg_rel_res;   /* last achieved relative residual     */
  double ms_linearize;  /* device time, HIP events; measured when options.time_kernels or .verbose is set
                         * or the system has more than 4096 block rows, 0 otherwise (the three event
                         * markers per trial are 7 % of a KITTI-00 iteration) */
  double ms_solve;
  double ms_update;     /* oplus + chi2 + scale                */
  int32_t pcg_capped;   /* PCG solves of this iteration that stopped at pcg_max_iters without reaching
                         * pcg_rel_tol.  LinearSolverEigen (kitti_surf.cpp:553-554) has no such state; a
                         * capped solve is an INEXACT LM step, not a failed one: CG iterates from x0 = 0 are
                         * descent directions of the damped model and satisfy x.(lambda x + b) = x.(H+lambda I)x,
                         * so g2o's gain ratio stays meaningful and decides the trial.  Exact
                         * solver: always 0 */
  int32_t reserved_;
} sim3opt_iter_stats;

/* Device time of the dominant kernels accumulated since initialize / reset
 * (HIP events on the library's own stream; used by bench.py's roofline). */
typedef struct sim3opt_kernel_times {
  double ms_spmv;      int64_t n_spmv;
  double ms_pcg_vec;   int64_t n_pcg_vec;
  double ms_linearize; int64_t n_linearize;
  double ms_chi2;      int64_t n_chi2;
  double ms_update;    int64_t n_update;
  /* multigrid cycles: device time spent on the levels a rank partition REPLICATES (every rank runs them whole:
   * the part of a PCG iteration that does not shrink with the number of ranks) and the number of visits of the
   * first such level; on one rank with options.amg_virtual_ranks = N: what an N-rank run would replicate */
  double ms_replicated_levels; int64_t n_replicated_visits;
  /* batched solves of rejected LM trials (options.pcg_batch): batches run, systems they held */
  int64_t n_batches; int64_t n_batched_solves;
} sim3opt_kernel_times;

/* Device time of the collectives of the row-partitioned path accumulated since initialize / reset
 * (HIP event pairs on the library's stream around every collective when options.time_kernels is set;
 * a pair includes the wait for the slowest rank).  bytes: payload of the whole vector / buffer. */
typedef struct sim3opt_comm_times {
  double ms_allreduce;  int64_t n_allreduce;  int64_t bytes_allreduce;
  double ms_allgather;  int64_t n_allgather;  int64_t bytes_allgather;
  /* neighbour exchanges (grouped send / receive pairs); bytes: what THIS rank sent plus what it received */
  double ms_exchange;   int64_t n_exchange;   int64_t bytes_exchange;
} sim3opt_comm_times;

int sim3opt_version(void);
void sim3opt_options_default(sim3opt_options* o);

/* g2o::SparseOptimizer ctor + setAlgorithm                         kitti_surf.cpp:552-558 */
sim3opt_graph* sim3opt_create(void);
void sim3opt_destroy(sim3opt_graph* g);
/* May be called at any time.  device, linear_solver, preconditioner and chain_segment are read by
 * sim3opt_initialize; every other field takes effect at the next call that uses it. */
int sim3opt_set_options(sim3opt_graph* g, const sim3opt_options* o);
int sim3opt_get_options(const sim3opt_graph* g, sim3opt_options* o);
const char* sim3opt_last_error(const sim3opt_graph* g);

/* new VertexSim3Expmap; setEstimate; setFixed; setId; addVertex    kitti_surf.cpp:602-620 */
int sim3opt_add_vertex(sim3opt_graph* g, int32_t id, const double state[8], int32_t fixed);
/* bulk form for graphs too large for per-element calls */
int sim3opt_add_vertices(sim3opt_graph* g, int32_t n, const int32_t* ids /*NULL: 0..n-1 appended*/,
                         const double* states /*n x 8*/, const uint8_t* fixed /*NULL: none*/);

/* new EdgeSim3; setVertex(0,v0); setVertex(1,v1); setMeasurement; information(); [setRobustKernel];
 * addEdge                                                            kitti_surf.cpp:633-638, :663-668 */
int sim3opt_add_edge(sim3opt_graph* g, int32_t id_v0, int32_t id_v1, const double meas[8],
                     const double* info77 /*NULL = I7*/, int32_t kernel, double kernel_delta);
int sim3opt_add_edges(sim3opt_graph* g, int32_t m, const int32_t* id_v0, const int32_t* id_v1,
                      const double* meas /*m x 8*/, const double* info /*NULL or m x 49*/,
                      int32_t kernel, double kernel_delta);

/* e->setRobustKernel(rk) for n edges (edge insertion indices; NULL = 0..n-1); before or after initialize;
 * later entries win; validated as a whole before anything changes (SIM3OPT_ERR_ARG: unknown kind, delta not
 * finite and > 0 for a kind other than NONE, index outside 0..m-1).  After initialize the next chi2 /
 * linearize / optimize uses the new kernels; the graph does not need sim3opt_initialize again.
 * Partitioned runs: every rank makes the same call, as with add_edges. */
int sim3opt_set_edge_kernels(sim3opt_graph* g, int32_t n, const int32_t* edges, const int32_t* kinds,
                             const double* deltas);
/* kind and delta of every edge (NONE edges: delta 0); NULL outputs skipped */
int sim3opt_get_edge_kernels(const sim3opt_graph* g, int32_t* kinds /*m*/, double* deltas /*m*/);
/* the kernel formulas above on the host, no GPU needed: rho[0] = rho(e2), rho[1] = rho'(e2) (e2 >= 0) */
int sim3opt_robustify(int32_t kind, double delta, double e2, double rho[2]);

int32_t sim3opt_num_vertices(const sim3opt_graph* g);
int32_t sim3opt_num_edges(const sim3opt_graph* g);
/* edges()[k]: endpoint ids and measurement of the k-th edge added   (g2o OptimizableGraph::edges) */
int sim3opt_get_edge(const sim3opt_graph* g, int32_t k, int32_t* id_v0, int32_t* id_v1,
                     double meas[8]);

/* SparseOptimizer::initializeOptimization()                        kitti_surf.cpp:674
 * Builds the index mapping and the block-CSR pattern, uploads the graph to HBM. */
int sim3opt_initialize(sim3opt_graph* g);

/* SparseOptimizer::optimize(n)                                     kitti_surf.cpp:675
 * Returns iterations executed (>0), -1 if nothing to optimise, 0 on failure
 * (g2o convention; details via sim3opt_last_error). */
int sim3opt_optimize(sim3opt_graph* g, int32_t max_iters);

/* vertex(id)->estimate()                                           kitti_surf.cpp:688-689 */
int sim3opt_get_vertex(sim3opt_graph* g, int32_t id, double state[8]);
/* vertex(id)->setEstimate() after construction (warm start)        kitti_surf.cpp:1037-1038 */
int sim3opt_set_vertex(sim3opt_graph* g, int32_t id, const double state[8]);
/* all estimates in insertion order */
int sim3opt_get_vertices(sim3opt_graph* g, double* states /*n x 8*/);
int sim3opt_set_vertices(sim3opt_graph* g, const double* states /*n x 8*/);

/* computeActiveErrors(); activeRobustChi2()                        kittiDetector.h:786-787 */
int sim3opt_chi2(sim3opt_graph* g, double* chi2);

/* statistics of the last optimize() */
int32_t sim3opt_num_iterations(const sim3opt_graph* g);
int sim3opt_get_stats(const sim3opt_graph* g, int32_t iter, sim3opt_iter_stats* out);
/* trust-region record of iteration `iter` of the last optimize(); SIM3OPT_ERR_STATE when that run was not a
 * dogleg run, SIM3OPT_ERR_ARG for an iteration out of range.  (For Gauss-Newton and dogleg the fields of
 * sim3opt_iter_stats read: lambda = damping added to the GN solve (0 while H stayed positive definite),
 * rho = last gain ratio, trials = g2o's numTries, pcg_* = the GN solve(s) of the iteration.) */
int sim3opt_get_trust_region_stats(const sim3opt_graph* g, int32_t iter, sim3opt_tr_stats* out);
int sim3opt_get_kernel_times(sim3opt_graph* g, sim3opt_kernel_times* out);
int sim3opt_reset_kernel_times(sim3opt_graph* g);   /* (also clears the collectives' times) */
int sim3opt_get_comm_times(sim3opt_graph* g, sim3opt_comm_times* out);
/* How the PCG loops were scheduled since initialize / the last reset (reset != 0 here, or sim3opt_reset_kernel_times):
 * out[0] iterations enqueued, out[1] of them enqueued after the device had raised `done` (enqueued - executed),
 * out[2] looks at the solver's scalars in the iteration loops that synchronised with an empty queue behind them,
 * out[3] looks that were waited for with the next chunk already queued.  The host sizes its chunks from the
 * reduction per iteration it has seen (options.pcg_check_every caps them; 1: one iteration per look, no prediction);
 * the stopping iteration is the device's decision, so none of this shows in a result.  out may be NULL. */
int sim3opt_pcg_schedule_stats(sim3opt_graph* g, int64_t out[4], int32_t reset);

/* ---- kernel-level access (parity tests against the CPU oracle, bench roofline) ---- */
/* per-edge residuals e (m x 7), edge insertion order                EdgeSim3::computeError */
int sim3opt_edge_errors(sim3opt_graph* g, double* e_out);
/* e->chi2() (e^T Omega e) of every edge, and rho / rho' of its kernel at the current estimates, edge insertion
 * order (NULL outputs skipped); partitioned runs: every rank gets every edge            Edge::chi2, robustify */
int sim3opt_edge_chi2(sim3opt_graph* g, double* chi2 /*m*/, double* rho /*m*/, double* weight /*m*/);
/* closed-form Jacobians (options.jacobians = 1) of every edge at the current estimates, edge insertion order:
 * e (m x 7) as sim3opt_edge_errors, J (m x 7 x 14, row-major per edge: J[98 k + 14 r + c]; columns 0..6 = de/dd0,
 * 7..13 = de/dd1 for the updates S <- exp(d) S; options.dof_mask zeroes frozen columns), evaluated on the
 * device by the functions the linearisation uses.  Needs fix_small_angle_b = 1.          EdgeSim3::linearizeOplus */
int sim3opt_edge_jacobians(sim3opt_graph* g, double* e_out, double* J_out);
/* the same for one edge, on the host (no GPU needed): e[7], J[98] as above; o NULL = defaults, which are refused
 * (fix_small_angle_b = 0) */
int sim3opt_sim3_edge_jacobian(const double meas[8], const double s0[8], const double s1[8],
                               const sim3opt_options* o, double e[7], double J[98]);
/* runs the linearisation kernels once on the current estimates     BlockSolver::buildSystem */
int sim3opt_linearize(sim3opt_graph* g);
/* ---- read-outs of the LM set-up and update kernels, for tests ----
 * Contract of both: nothing in the solver uses them; they run the launch code of sim3opt_linearize / of an LM trial on
 * the current estimates, copy device buffers to the host and leave the estimates, every solver scalar, the cached chi2,
 * the statistics and sim3opt_get_kernel_times -- hence every later sim3opt_optimize -- bit for bit what they are
 * without the call.  One GPU: SIM3OPT_ERR_STATE on a partitioned graph (a rank holds its rows' share only) and before
 * sim3opt_initialize; SIM3OPT_ERR_ARG for a NULL pointer that is not marked optional; the message is in
 * sim3opt_last_error.  (sim3opt_version is unchanged: diagnostics are not part of the versioned interface.) */
/* Diagnostic.  Sizes of the arrays below: the edges the linearisation runs on (at least one free endpoint) and the
 * incidences (free endpoints of edges) of all block rows. */
int sim3opt_debug_linearization_dims(sim3opt_graph* g, int32_t* n_active, int32_t* n_incidences);
/* Diagnostic.  Linearises as sim3opt_linearize does, in either Jacobian mode, with the linearisation kernel in an
 * instantiation that also stores what its Gram phase consumed; sim3opt_get_system afterwards returns what
 * sim3opt_linearize produces, bit for bit.  J (n_active x 15 x 7): per active edge the 14 Jacobian columns (de/dd0,
 * then de/dd1; 7 residual rows each) and e, as they lie in LDS; w (n_active): the robust weight the phase used;
 * active (n_active): the edges' indices; scratch (n_incidences x 35): per incidence the upper triangle of its
 * diagonal contribution (column-major: (0,0) (0,1) (1,1) (0,2) ...) and its 7 entries of b; incptr (block rows + 1),
 * inc0 / inc1 / slot01 / slot10 (edges each; -1: a fixed endpoint): the incidence slots and off-diagonal blocks an
 * edge owns; *trace and *maxdiag: sum and largest magnitude of the scalar diagonal of H (lambda_0's input). */
int sim3opt_debug_linearization(sim3opt_graph* g, double* J, double* w, int32_t* active, double* scratch,
                                int32_t* incptr, int32_t* inc0, int32_t* inc1, int32_t* slot01, int32_t* slot10,
                                double* trace, double* maxdiag);
/* Diagnostic.  What an LM trial makes of a caller's step x (7 per block row, any numbers) at damping lambda: the
 * estimates k_oplus produces (states_out, 8 per vertex) and the backup it takes (backup_out), the robustified chi2
 * there (k_chi2) and scale = x . (lambda x + b) (k_scale), both summed by k_final_sum_two; then the estimates are
 * restored from the backup.  Needs a linearisation (b).  with_fail != 0 presents the exact solver's failure token:
 * nothing may move (SIM3OPT_ERR_STATE unless the exact solver is in use).  grid = 0: the workgroup counts of a trial;
 * 1 .. 2048: that many workgroups, hence partial sums, for both k_chi2 and k_scale.  The four outputs may be NULL,
 * not all of them. */
int sim3opt_debug_update(sim3opt_graph* g, const double* x, double lambda, int32_t with_fail, int32_t grid,
                         double* states_out, double* backup_out, double* chi2, double* scale);
/* ---- read-outs of the dogleg's kernels and of the column kernels of the inverse, for tests ----
 * Same contract as the read-outs above (sim3opt_version unchanged): they run the launch code of a dogleg iteration
 * after its solve / the vector kernels of a column solve on the caller's data and leave the estimates, every solver
 * vector and scalar, the cached chi2, the statistics and sim3opt_get_kernel_times bit for bit what they are without
 * the call.  SIM3OPT_ERR_STATE on a partitioned graph, before sim3opt_initialize, without a linearisation, and for
 * with_fail unless the exact solver is in use; SIM3OPT_ERR_ARG for a NULL input, a grid outside 0 .. 2048, a range or
 * an index out of bounds. */
/* Diagnostic.  h_gn (7 per block row, any numbers) goes where the solve leaves its solution.  scalars[6]: b.b, b^T H b,
 * g.g, b.g, (Hb).g, g^T H g for g = h_gn, as k_dl_dots, k_dl_sum and k_dl_final leave them and the host reads them;
 * the SpMVs' partial count is options.span_grid as sim3opt_initialize clamped it (sim3opt_get_options).  grid = 0:
 * k_dl_dots' own workgroup count, 1 .. 2048: that many (= partial sums per dot); [j0, j1) the entries the four dots run
 * over (0 <= j0 <= j1 <= 7 x block rows; both 0: all of them; the two quadratic forms always cover every row).
 * states_out / backup_out (8 per vertex): the estimates after k_dogleg_oplus with h_dl = ca b + cg h_gn and the backup
 * it takes; then the estimates are restored.  with_fail != 0 presents the exact solver's failure token: nothing may
 * move.  The three outputs may be NULL, not all of them. */
int sim3opt_debug_dogleg(sim3opt_graph* g, const double* h_gn, double ca, double cg, int32_t with_fail, int32_t grid,
                         int64_t j0, int64_t j1, double* scalars, double* states_out, double* backup_out);
/* The dogleg's step rule on the host (no GPU needed; the function sim3opt_optimize calls per trial): from the six
 * scalars above and the trust radius delta, model = {alpha, ||h_sd||, ||h_gn||} and trial = {ca, cg, ||h_dl||,
 * linearGain} of h_dl = ca b + cg h_gn, *step = SIM3OPT_STEP_*.  SIM3OPT_ERR_ARG for a NULL pointer. */
int sim3opt_dogleg_rule(const double scalars[6], double delta, double model[3], double trial[4], int32_t* step);
/* Diagnostic.  One of the vector kernels of the columns of the inverse (options.cov_solver) on the caller's data, at a
 * vector length 1 <= n <= 7 x block rows, staged in the buffers a column solve uses: systems lie vs = 7 x block rows
 * rounded up to a multiple of 64 doubles apart.  Also refused (SIM3OPT_ERR_STATE) where the columns are: on a graph
 * that factorises exactly.  grid = 0: the workgroups a solve launches, 1 .. 2048: that many.  `out` is read and written:
 * on entry what the kernel's output buffer holds before the launch.
 *   kernel 0, k_cols_rhs<K>: K = 1 .. 4 systems, at[K] their unit entries (< 0: none; must be < n); out: K x vs.
 *   kernel 1, k_cols_residual: r = a - b on system `system` (0 .. 3); a, b: n each; out: vs (r and what follows it).
 *   kernel 2, k_cols_axpy: y += a on system `system`; out: vs, on entry y.
 *   kernel 3, k_cols_gather: column `col` (0 .. 6) of blocks first .. first + count - 1 of out (n_blocks x 49) from
 *     a = y (n) at the block rows rows[first .. first + count) (7 rows[k] + 7 <= n; rows has first + count entries). */
int sim3opt_debug_column_vectors(sim3opt_graph* g, int32_t kernel, int32_t grid, int64_t n, int32_t K, const int64_t* at,
                                 int32_t system, const double* a, const double* b, int32_t first, int32_t count,
                                 int32_t col, const int32_t* rows, int32_t n_blocks, double* out);
/* ---- read-out of the exact block Cholesky, its solve and the selected inversion, for tests ----
 * Same contract as the read-outs above: nothing in the solver uses it; it runs the launches that exist (k_ldl_gather,
 * k_ldl, k_selinv_pivots, k_selinv) and copies their buffers out; the system H / b, every solver scalar (the LM's fail
 * word and its token included), the cached chi2, the statistics and sim3opt_get_kernel_times are bit for bit what they
 * are without the call.  Refused with SIM3OPT_ERR_STATE before sim3opt_initialize, on a partitioned graph, for
 * context 0 where the LM solves by PCG, and without a linearisation unless vals and b are both given; with
 * SIM3OPT_ERR_ARG for a NULL output that the call would fill, another context, with_selinv on context 0, a lambda
 * that is negative or not finite.  (sim3opt_version is unchanged.) */
/* Diagnostic.  Sizes: block columns, blocks of L (and Z) of the context's plan, blocks of the system.  Context 1 is
 * built here at first use, as sim3opt_marginals builds it. */
int sim3opt_debug_factor_dims(sim3opt_graph* g, int32_t context, int32_t* n_block_rows, int64_t* n_blocks_L,
                              int64_t* n_blocks);
/* Diagnostic.  context 0: the LM solver's factorisation; 1: the marginals' (plan of sim3opt_direct_plan with the limit
 * of sim3opt_marginal_plan, lists of the latter).  (H + lambda I) = L L^T from the last linearisation, or from vals
 * (n_blocks x 49, layout and order of sim3opt_get_system) and / or b (7 per block row) where not NULL: they go to
 * scratch device buffers, and afterwards the context gathers the real system again.  Outputs, in the plan's numbering,
 * blocks column-major: Aperm (n_blocks_L x 49; the gathered blocks, no damping), bp (7 nb), L (n_blocks_L x 49), Dinv
 * (nb x 49; L(j,j)^-1), y (7 nb; L y = bp), *fail_word (non-zero: a pivot that is not positive and finite); with_solve
 * also xp (7 nb; L^T xp = y) and x (7 nb, by block rows of the system); with_selinv (context 1) also Z (n_blocks_L x 49,
 * (H + lambda I)^-1 on the pattern of L) and *singular (a pivot below 1e-13 max |H_dd|; with injected vals the
 * largest scalar diagonal entry of their diagonal blocks).  bord / brow (n_blocks_L each, may be NULL): per column the
 * order in which the backward solve and the selected inversion take its blocks, and those blocks' rows. */
int sim3opt_debug_factor(sim3opt_graph* g, int32_t context, double lambda, const double* vals, const double* b,
                         int32_t with_solve, int32_t with_selinv, double* Aperm, double* bp, double* L, double* Dinv,
                         double* y, double* xp, double* x, int32_t* fail_word, double* Z, int32_t* singular,
                         int32_t* bord, int32_t* brow);
/* dimensions of the block-CSR system: free block rows, stored 7x7 blocks */
int sim3opt_system_dims(const sim3opt_graph* g, int32_t* n_block_rows, int64_t* n_blocks);
/* the block-CSR pattern alone (host only, no GPU needed, may be called before initialize): two
 * calls, arrays NULL to size them.  Row k = k-th free vertex in insertion order: its diagonal block,
 * then one block per incident edge whose other endpoint is free, sorted by (column, edge). */
int sim3opt_system_pattern(sim3opt_graph* g, int32_t* n_block_rows, int64_t* n_blocks,
                           int32_t* rowptr, int32_t* colidx);
/* copies the block-CSR Hessian (rowptr nb+1, colidx nnzb, values nnzb x 49 column-major per
 * block) and b (7 nb) to the host; block row k = k-th free vertex in insertion order.  A partitioned run
 * assembles and holds the blocks (and the entries of b) of this rank's rows only (sim3opt_local_rows): the
 * other rows' blocks read zero */
int sim3opt_get_system(sim3opt_graph* g, int32_t* rowptr, int32_t* colidx, double* values,
                       double* b);
/* (a graph that is row-partitioned over several ranks numbers its block rows in locality order
 * instead: sim3opt_partition_plan(..., locality = 1, vertex_of_row, ...) gives the mapping) */
/* solves (H + lambda I) x = b with the block-Jacobi PCG on the last linearisation */
int sim3opt_solve(sim3opt_graph* g, double lambda, double* x /*7 nb*/, int32_t* iters,
                  double* rel_res);
/* Preconditioner the PCG of this (initialized) graph uses: 0 block-Jacobi, 1 chain segments,
 * 2 aggregation multigrid (what `preconditioner = -1` resolved to); negative = error code. */
int sim3opt_preconditioner_in_use(const sim3opt_graph* g);
/* Linear solver of this (initialized) graph: 1 exact sparse block Cholesky, 0 PCG (what
 * `linear_solver = -1` resolved to); negative = error code. */
int sim3opt_linear_solver_in_use(const sim3opt_graph* g);
/* What the automatic multigrid choices resolved to on this (initialized) graph: levels of the hierarchy
 * (0: none), how many of them are partitioned over the ranks (0 on one rank), visits of levels 1, 2, 3, >= 4 per
 * visit of the level above (options.amg_cycle = 0 picks {2,3,3,3}, or {1,2,2,2} on a partitioned run).  Any
 * pointer may be NULL. */
int sim3opt_amg_in_use(const sim3opt_graph* g, int32_t* n_levels, int32_t* n_partitioned, int32_t visits[4]);
/* Device memory of the block arrays of this (initialized) graph on this rank -- H, its FP32 copy, the coarse levels'
 * blocks, the assembly scratch: bytes[0] as allocated (a partitioned run holds its own rows only), bytes[1] what one
 * rank holding the whole graph allocates for them.  (Vectors, edges and index arrays -- about a tenth of the total --
 * are replicated and not counted.) */
int sim3opt_device_bytes(const sim3opt_graph* g, int64_t bytes[2]);
/* Plan of the exact sparse block Cholesky (LinearSolverEigen's role, kitti_surf.cpp:553-554) for this
 * graph: host only, no GPU needed, may be called before initialize.  Block column j of L is block row
 * perm[j] of the system (nested-dissection order); its stored 7x7 blocks are colptr[j]..colptr[j+1]
 * (diagonal first, rows lrow[] ascending).  Block s of L starts from the sum of the system's blocks
 * src[srcptr[s]..srcptr[s+1]) (indices into the block-CSR values of sim3opt_get_system) and subtracts
 * L[pa[k]] L[pb[k]]^T for k in pairptr[s]..pairptr[s+1].  Schedule: group q runs levels
 * gptr[q]..gptr[q+1], level l is columns lcolp[l]..lcolp[l+1]; groups but the last are independent.
 * Work split of the kernel: level l runs in rounds rptr[l]..rptr[l+1]; round q is 18 ints at
 * cells[18 q]: wavefront w owns blocks cells[18 q + w]..cells[18 q + w + 1] (at most 8) and the
 * products cells[18 q + 9 + w]..cells[18 q + 9 + w + 1] (4 wavefronts in the bottom groups, 8 in
 * the last one).
 * dims = {columns, blocks of L, block products per factorisation, elimination-tree height, groups,
 * levels, entries of src, rounds}.  Two calls: arrays NULL to size them, then filled.  max_pairs <= 0:
 * the automatic limit.  SIM3OPT_ERR_STATE when a factorisation needs more block products than that. */
int sim3opt_direct_plan(sim3opt_graph* g, int64_t max_pairs, int64_t dims[8], int32_t* perm,
                        int32_t* colptr, int32_t* lrow, int32_t* srcptr, int32_t* src,
                        int32_t* pairptr, int32_t* pa, int32_t* pb, int32_t* gptr, int32_t* lcolp,
                        int32_t* rptr, int32_t* cells);
/* ---- marginal covariances (g2o SparseOptimizer::computeMarginals) ----
 * Blocks of (H + lambda I)^-1, H linearised at the CURRENT estimates, rows/cols in the tangent order
 * [omega upsilon sigma] of the oplus increment; cov is n x 49, column-major 7x7 blocks, rows = id_a's
 * tangent, cols = id_b's.  Pairs: a vertex with itself, or the two ends of any edge (anything else in the
 * factor's pattern works too; outside it, or a fixed vertex: SIM3OPT_ERR_ARG).  Computed by a selected
 * inversion on the pattern of the exact block Cholesky, in a context of its own
 * built at the first call (at most options.direct_max_pairs block products, else 3e7; a refused plan:
 * SIM3OPT_ERR_STATE with the reason in sim3opt_last_error).  The LM's solver choice and state are left
 * as they are: optimize() after this call runs exactly as without it.  A singular H + lambda I (lambda = 0
 * without a fixed vertex, or with a cleared dof_mask bit): SIM3OPT_ERR_STATE.  One GPU only
 * (world > 1: SIM3OPT_ERR_STATE). */
int sim3opt_marginals(sim3opt_graph* g, double lambda, int32_t n, const int32_t* id_a,
                      const int32_t* id_b, double* cov);
/* All free vertices' diagonal blocks, insertion order (nfree x 49); as sim3opt_marginals. */
int sim3opt_marginal_covariances(sim3opt_graph* g, double lambda, double* cov);
/* Blocks of (H + lambda I)^-1 for ANY pairs of free vertices -- two keyframes no edge joins yet, say; layout,
 * lambda, errors and the one-GPU rule as sim3opt_marginals (a fixed or unknown vertex: SIM3OPT_ERR_ARG).  Pairs on
 * the factor's pattern are the selected inversion's, the same bits as sim3opt_marginals returns.  The others are
 * sums over the common ancestors of the two vertices in the elimination tree of W(k,a)^T W(k,b), W = L^-1
 * (DESIGN.md section 5f), on the same factorisation: exactly zero between two components of the graph; each unordered
 * pair computed once, the reversed pair its exact transpose; bits that do not depend on the order, the duplicates or
 * the split of the request, on the schedule of the factorisation or on options.cov_workspace_mb (which bounds the
 * device memory of one chunk; too small for the root paths of a single pair: SIM3OPT_ERR_STATE). */
int sim3opt_covariances(sim3opt_graph* g, double lambda, int32_t n, const int32_t* id_a,
                        const int32_t* id_b, double* cov);
/* What the last sim3opt_marginals / _covariances / _gate_edges call did: {chunks of pairs outside the pattern,
 * root paths walked, distinct pairs outside the pattern, pairs on it, workspace bytes, selected inversion run}. */
int sim3opt_covariance_stats(const sim3opt_graph* g, int64_t out[6]);
/* ---- the same blocks on graphs too large to factor: columns of the inverse (options.cov_solver = 1, or 2 where the
 * marginal plan is refused; DESIGN.md section 5f "Blocks by columns of the inverse") ----
 * sim3opt_covariances and sim3opt_gate_edges then solve (H + lambda I) y = e_k for the seven unit vectors of a set of
 * vertices that covers the request (every unordered pair has an endpoint in it; sim3opt_covariance_columns_plan) with
 * the PCG and preconditioner the graph was initialised with -- on a multigrid graph four columns per pass over the
 * blocks -- and read block (a, b) as rows a of the columns of b.  Each column is checked by its true residual against
 * options.cov_rel_tol and refined at most twice; one that stays above it, a PCG breakdown or a failed set-up pivot:
 * SIM3OPT_ERR_STATE naming the vertex and the residual, nothing written.  Every entry of a returned block is within
 * cov_rel_tol / lambda_min(H + lambda I) of the true one; cond x eps is the floor of a residual in FP64, so an
 * ill-conditioned H wants a lambda > 0.  Each unordered pair is computed once, the reversed pair is its exact
 * transpose, a diagonal block is symmetrised, duplicates are identical; the bits of an off-diagonal block depend on
 * which endpoint the cover chose, hence on the rest of the request (unlike the exact path), and on nothing else.  The
 * LM state is left as it was.  The exact path's counters (sim3opt_covariance_stats) read 0 after such a call. */
/* Host only, may be called before initialize.  The vertices (ids, in the order chosen) whose columns of
 * (H + lambda I)^-1 cov_solver = 1 would solve for this request; two calls, vertices NULL to size it.  Greedy cover:
 * repeatedly the vertex that covers the most pairs not yet covered, ties to the lowest block row.
 * A fixed or unknown vertex: SIM3OPT_ERR_ARG. */
int sim3opt_covariance_columns_plan(sim3opt_graph* g, int32_t n, const int32_t* id_a, const int32_t* id_b,
                                    int32_t* n_vertices, int32_t* vertices);
/* What the last column call did: counts = {vertices solved, columns, PCG iterations summed over the columns,
 * refinement rounds, batches}; res = {largest ||g - (H + lambda I) y||_2 / ||g||_2 over the columns, cov_rel_tol used}. */
int sim3opt_covariance_columns_stats(const sim3opt_graph* g, int64_t counts[5], double res[2]);
/* Chi-square gate of candidate edges that are NOT added to the graph (is this loop closure consistent with what the
 * optimiser believes?).  Per candidate (id_v0, id_v1, meas as sim3opt_add_edge takes it, info column-major or NULL
 * for I): e[7] = EdgeSim3's residual at the current estimates; S[49] (column-major) = J0 S00 J0^T + J0 S01 J1^T +
 * J1 S10 J0^T + J1 S11 J1^T + info^-1 with the Jacobians of options.jacobians (0: central differences with fd_delta,
 * 1: closed form; columns as sim3opt_edge_jacobians, dof_mask applied) and Sxy the blocks sim3opt_covariances returns
 * (one factorisation per call; zero for a fixed endpoint); d2 = e^T S^-1 e, chi-square with 7 degrees of freedom
 * under the linearised Gaussian model.  v0 == v1, an unknown id, a non-finite measurement or an info that is not
 * symmetric positive definite: SIM3OPT_ERR_ARG, nothing written.  Other errors as sim3opt_covariances.  The graph,
 * its estimates and the LM state are untouched. */
int sim3opt_gate_edges(sim3opt_graph* g, double lambda, int32_t n, const int32_t* id_v0, const int32_t* id_v1,
                       const double* meas /* n x 8 */, const double* info /* NULL = I, or n x 49 */,
                       double* e /* n x 7 */, double* S /* n x 49 col-major */, double* d2 /* n */);
/* Plan of the selected inversion (host only, no GPU needed, may be called before initialize), on the
 * factor plan of sim3opt_direct_plan (perm, colptr, lrow, gptr, lcolp as there).  Block s of Z is
 * ( Z0 - sum_p op(Z[za[p]]) L[zl[p]] ) L(j,j)^-1 over p in zptr[s]..zptr[s+1], in that order, where
 * op transposes when zt[p] = 1 and Z0 = L(j,j)^-T on a diagonal block, 0 elsewhere; Z and L share the
 * block numbering of L.  Levels run top-down, off-diagonal blocks of a level before its diagonal ones.
 * dims = {columns, blocks of L, products, elimination-tree height, groups, levels}.  Two calls: arrays
 * NULL to size them, then filled.  max_pairs <= 0: 3e7. */
int sim3opt_marginal_plan(sim3opt_graph* g, int64_t max_pairs, int64_t dims[6], int32_t* perm,
                          int32_t* colptr, int32_t* lrow, int32_t* gptr, int32_t* lcolp, int32_t* zptr,
                          int32_t* za, int32_t* zt, int32_t* zl);
/* Structure of the multigrid hierarchy `preconditioner = 2` would use for this graph (host only, no
 * GPU needed, may be called before initialize): *n_levels levels; rows[l] / blocks[l] = block rows
 * and stored 7x7 blocks of level l (up to `capacity` levels are written); aggregate_of_row (may be
 * NULL) receives, for each level-0 block row (free vertex in insertion order), its level-1 row.
 * SIM3OPT_ERR_STATE when the graph does not coarsen (block-Jacobi is used then). */
int sim3opt_amg_hierarchy(sim3opt_graph* g, int32_t capacity, int32_t* n_levels, int32_t* rows,
                          int64_t* blocks, int32_t* aggregate_of_row);

/* ---- diagnostic read-outs of the PCG's preconditioners (tests/test_gpu_preconditioners.py compares them with a
 * long-double restatement, tests/amg_ref.py).  Inspection calls like sim3opt_get_system: nothing in the solver uses
 * them, and a solve or optimize() after one of them computes bit for bit what it computes without it. ---- */
/* Diagnostic.  Structure of level `level` of the hierarchy sim3opt_amg_hierarchy describes (host only, no GPU, may be
 * called before initialize): *n_levels, the level's block rows and blocks, its pattern (rowptr n_block_rows + 1,
 * colidx n_blocks; level 0: the system's; coarse levels: diagonal first, then unique ascending columns) and, on
 * every level but the coarsest, the aggregate (row of level + 1) of each row.  Any pointer may be NULL: call once
 * for the sizes, once for the arrays. */
int sim3opt_amg_level_structure(sim3opt_graph* g, int32_t level, int32_t* n_levels, int32_t* n_block_rows,
                                int64_t* n_blocks, int32_t* rowptr, int32_t* colidx, int32_t* aggregate_of_row);
/* Diagnostic.  Numbers of level `level` after the set-up a multigrid PCG solve with damping `lambda` runs on the
 * last linearisation (Galerkin products if the linearisation is new, then the per-trial part).  Any pointer may be
 * NULL.  rowptr / colidx: the pattern as the device holds it; values: n_blocks x 49 column-major blocks (level 0:
 * H undamped; coarse levels: the diagonal blocks damped by lambda W); values32: the FP32 copy the cycle's matrix
 * passes stream, de-interleaved to n_blocks x 49 (options.amg_fp32 = 0: SIM3OPT_ERR_STATE); W = P^T P and diagH =
 * the undamped diagonal blocks (n_block_rows x 49 column-major; coarse levels only); Minv = omega (D + lambda W)^-1
 * (n_block_rows x 49 ROW-major, as stored); P = Ad(S_v) of every level-0 row (column-major; level 0 only).
 * A non-positive pivot in the set-up: SIM3OPT_ERR_STATE (a solve would fall back to block-Jacobi).  One GPU only
 * (world > 1: SIM3OPT_ERR_STATE), multigrid graphs only. */
int sim3opt_amg_level_numbers(sim3opt_graph* g, double lambda, int32_t level, int32_t* rowptr, int32_t* colidx,
                              double* values, float* values32, double* W, double* diagH, double* Minv, double* P);
/* Diagnostic.  The dense inverse of the coarsest level for `lambda` (7 rows x 7 rows of that level, row-major);
 * otherwise as sim3opt_amg_level_numbers. */
int sim3opt_amg_coarsest_inverse(sim3opt_graph* g, double lambda, double* Ainv);
/* Diagnostic.  z[q] = M^-1 r[q], q < nrhs (vectors of 7 x block rows, one after the other), for prec = 0 block-Jacobi,
 * 1 chain segments, 2 aggregation multigrid -- 1 and 2 only on a graph initialised with that preconditioner
 * (sim3opt_preconditioner_in_use) -- on the last linearisation: ONE set-up for `lambda`, then per right-hand side
 * the launches of a PCG iteration with the engine's current cycle options.  A failed set-up pivot is
 * SIM3OPT_ERR_STATE.  One GPU only. */
int sim3opt_preconditioner_apply(sim3opt_graph* g, int32_t prec, double lambda, int32_t nrhs, const double* r,
                                 double* z);
/* ---- diagnostic read-outs of the PCG's own operator (tests/test_gpu_pcg_operator.py compares them with a
 * long-double restatement, tests/pcg_ref.py); inspection calls like the ones above. ---- */
/* Diagnostic.  The table of row spans the span SpMV's wavefronts work on, as the device holds it: *n_spans =
 * 4 x workgroups, wrow (may be NULL: call once for the size) receives *n_spans + 1 ascending block rows; wavefront w
 * owns rows wrow[w] .. wrow[w + 1] - 1 (a partitioned run: this rank's table). */
int sim3opt_spmv_spans(sim3opt_graph* g, int32_t* n_spans, int32_t* wrow);
/* Diagnostic.  The instantiation of the one-system span SpMV in use: *chunk = 4 or 8 blocks per lane group and load,
 * *non_temporal = 1 if the blocks are streamed with non-temporal loads (SIM3OPT_SPMV="chunk,nt", read when the graph
 * is initialised). */
int sim3opt_spmv_variant(sim3opt_graph* g, int32_t* chunk, int32_t* non_temporal);
/* Diagnostic.  q[s] = (H + lambda[s] I) p[s], pq[s] = p[s] . q[s] and, with rvec, rp[s] = rvec[s] . p[s] for s < nrhs
 * (vectors of 7 x block rows, one after the other) on the last linearisation, by the launches of a PCG iteration:
 * nrhs = 1 the one-system SpMV with the engine's current variant (SIM3OPT_SPMV) and span table, the damping read from
 * the device's scalars, its partial sums added by the function a solve adds them with (the same value; a solve of up
 * to 2048 workgroups adds them inside its step kernel, not in a launch of their own); nrhs = 2 .. 4 the SpMV of the
 * batched trial solves (per-system damping, one pass over the blocks) and its sum -- on a graph with the multigrid
 * preconditioner only (else SIM3OPT_ERR_STATE).  rvec and rp are both NULL or both given; for nrhs > 1 the batched
 * solves themselves never pass rvec (their r.z comes from the cycle), so rp then exercises the kernel for this read-out
 * alone.  One GPU only (world > 1: SIM3OPT_ERR_STATE). */
int sim3opt_operator_apply(sim3opt_graph* g, int32_t nrhs, const double* lambda, const double* p, const double* rvec,
                           double* q, double* pq, double* rp);

/* ---- row-partitioned multi-GPU (one process per GPU, RCCL over xGMI) ----
 * Every rank adds the SAME full graph; rank r then owns a contiguous range of block rows (equal
 * length), linearises the edges incident to them, streams its rows in the SpMV and keeps
 * a replica of all vertex estimates.  Collectives per PCG iteration (single-reduction CG): ONE
 * in-place all-gather of the preconditioned residual and ONE 2-double all-reduce; with the multigrid
 * preconditioner a second all-gather and the all-reduce of the restricted level-1 residual
 * (DESIGN.md section 7 lists sizes for N = 2 / 4 / 8); per LM trial: one all-gather of the step, one
 * 2-double all-reduce.  All ranks return identical results.  Call between create and initialize.
 * unique_id is the 128-byte ncclUniqueId produced by sim3opt_comm_unique_id on rank 0 and broadcast
 * by the caller (torch.distributed / MPI). */
int sim3opt_comm_unique_id(uint8_t id_out[128]);
int sim3opt_comm_init(sim3opt_graph* g, int32_t rank, int32_t world, const uint8_t unique_id[128]);
/* Same partitioned path over user-supplied host collectives (MPI, gloo, ...): operands are staged
 * through pinned host memory.  op: 0 = sum, 1 = max.  offsets has world+1 entries in doubles; rank r
 * owns buf[offsets[r] .. offsets[r+1]) on entry and the whole buf must be filled on return.
 * Callbacks return 0 on success. */
typedef int (*sim3opt_allreduce_fn)(void* ctx, double* buf, int32_t n, int32_t op);
typedef int (*sim3opt_allgatherv_fn)(void* ctx, double* buf, const int64_t* offsets, int32_t rank,
                                     int32_t world);
int sim3opt_comm_init_callbacks(sim3opt_graph* g, int32_t rank, int32_t world,
                                sim3opt_allreduce_fn allreduce, sim3opt_allgatherv_fn allgatherv,
                                void* ctx);
/* Optional third callback: the neighbour exchange of the partitioned path (halo rows of a level go to the
 * ranks that read them and to nobody else).  send[send_offsets[p] .. send_offsets[p+1]) goes to rank p,
 * recv[recv_offsets[p] .. recv_offsets[p+1]) must hold what rank p sent to this rank on return (offsets
 * in doubles, world+1 entries each; most spans are empty: a slab has two neighbours).  Without it the
 * library falls back to the all-gather of the whole vector.  Call after sim3opt_comm_init_callbacks. */
typedef int (*sim3opt_alltoallv_fn)(void* ctx, const double* send, const int64_t* send_offsets, double* recv,
                                    const int64_t* recv_offsets, int32_t rank, int32_t world);
int sim3opt_comm_set_alltoallv(sim3opt_graph* g, sim3opt_alltoallv_fn alltoallv);
/* Plan of the per-iteration exchange for `n_block_rows` rows over `world` ranks (host only): fills
 * row_begin (world+1, may be NULL) with the equal-length rank partition and returns 1 when the
 * in-place equal-count ncclAllGather applies (always, for this partition -- trailing ranks may be
 * short or empty), 0 otherwise, negative on bad arguments.  *count = doubles each rank contributes,
 * *padded_len = doubles every exchanged vector is allocated with (world * count >= 7 n_block_rows;
 * the tail is padding no kernel reads). */
int sim3opt_comm_allgather_plan(int32_t n_block_rows, int32_t world, int32_t* row_begin,
                                int64_t* count, int64_t* padded_len);
/* host-side partition plans (no GPU needed), world+1 entries each:
 *   _equal : the RANK partition -- equal-length row spans, so the per-iteration exchange is one
 *            in-place ncclAllGather (pose-graph rows have near-uniform block counts)
 *   plain  : spans balanced by stored 7x7 blocks (used for the SpMV's per-wavefront spans) */
int sim3opt_partition_rows_equal(int32_t n_block_rows, int32_t world, int32_t* row_begin);
int sim3opt_partition_rows(int32_t n_block_rows, const int32_t* rowptr, int32_t world,
                           int32_t* row_begin /*world+1*/);
/* Row order and halo of the partition over `world` ranks (host only, may be called before
 * initialize).  locality = 1: the block rows in the breadth-first locality order the partitioned path
 * gives a graph with world > 1 (contiguous rank spans are slabs of the graph); 0: insertion order (what
 * one rank uses: g2o's hessianIndex).  vertex_of_row (n_block_rows entries, may be NULL): vertex index
 * (insertion order) of every block row; row_begin: world + 1; boundary_rows_of_rank[r]: rows of rank r
 * with a neighbour on another rank -- what it sends per exchange of the partitioned PCG;
 * *cut_edges: edges whose endpoints two ranks own (both linearise them). */
int sim3opt_partition_plan(sim3opt_graph* g, int32_t world, int32_t locality, int32_t* vertex_of_row,
                           int32_t* row_begin, int32_t* boundary_rows_of_rank, int64_t* cut_edges);
/* Neighbour-only exchange plan of rank `rank` on level 0 of the partition over `world` ranks (host only;
 * locality order): rows it sends (its own rows another rank's rows reference, grouped by that rank:
 * send_seg has world + 1 entries) and rows it receives (grouped by owner).  Two calls: rows NULL to get
 * the counts.  By the symmetry of the pattern, rank p's receive group for q equals q's send group for p. */
int sim3opt_halo_plan(sim3opt_graph* g, int32_t world, int32_t rank, int32_t* n_send, int32_t* n_recv,
                      int32_t* send_rows, int32_t* send_seg, int32_t* recv_rows, int32_t* recv_seg);
/* block-row range [begin, end) this graph's rank owns (valid after initialize) */
int sim3opt_local_rows(const sim3opt_graph* g, int32_t* begin, int32_t* end);

/* ---- one process drives N devices (the caller stays single-threaded) ----
 * sim3opt_set_devices gives the handle n ranks (1..8) INSIDE the library: a worker thread per rank, bound to
 * devices[r], with its own engine; the ranks exchange through each other's device memory (peer access over xGMI
 * between distinct devices, enabled here; a pair without it: sim3opt_initialize returns SIM3OPT_ERR_COMM and names
 * the pair).  An ordinal may repeat: N ranks on one GPU, the same kernels.  Call between create and initialize;
 * collective_timeout_s <= 0: 120 s.  SIM3OPT_ERR_ARG: n out of range, NULL, an ordinal below 0 or beyond the device
 * count; SIM3OPT_ERR_STATE: after initialize, or after sim3opt_comm_init* on this handle (and sim3opt_comm_init*
 * after this call).  n == 1 only selects the device: the plain one-rank graph.
 *
 * With n > 1 the handle stays ONE object and every entry is called once, from one thread:
 *   - what a partitioned graph serves runs on all ranks and returns rank 0's answer (all ranks hold a replica of
 *     every estimate and return identical results): initialize, optimize, chi2, get / set vertex(es), the stats,
 *     set_edge_kernels, edge_chi2 / edge_errors, linearize, amg_in_use, preconditioner_in_use, linear_solver_in_use,
 *     kernel_times, comm_times;
 *   - what a partitioned graph refuses stays SIM3OPT_ERR_STATE: marginals, covariances, gate_edges, solve, the
 *     operator, preconditioner and factor read-outs;
 *   - sim3opt_local_rows / sim3opt_device_bytes answer for rank 0, their _of_rank siblings for any rank.
 * A rank that fails, or waits longer than the timeout for its peers (its message names the collective's sequence
 * number), releases the others with SIM3OPT_ERR_COMM; the handle then answers SIM3OPT_ERR_STATE until it is
 * destroyed.  Nothing in here ends the process.  (INTEGRATION.md has the table, DESIGN.md section 7 the protocol.) */
int sim3opt_set_devices(sim3opt_graph* g, int32_t n, const int32_t* devices, double collective_timeout_s);
/* ranks this handle drives: n of sim3opt_set_devices, else 1 */
int sim3opt_rank_count(const sim3opt_graph* g);
int sim3opt_local_rows_of_rank(const sim3opt_graph* g, int32_t rank, int32_t* begin, int32_t* end);
int sim3opt_device_bytes_of_rank(const sim3opt_graph* g, int32_t rank, int64_t bytes[2]);

/* ---- diagnostic read-outs of the in-process transport (tests/test_gpu_comm_operators.py compares them bit for bit
 * with the numpy restatement tests/comm_ref.py) ----
 * Each runs exactly ONE collective on operands the caller supplies: every rank's own communicator, on that rank's own
 * stream, the same allreduce / allgatherv / exchange the engine calls during an optimisation.  They are for testing the
 * transport at payloads an optimisation never sends; nothing in the product calls them.  `world` below is
 * sim3opt_rank_count(g).  Rank r's operand is uploaded into a scratch device block of its own, at element offset
 * `phase` (0 or 1) from a 16-byte aligned start, between guard doubles of a fixed bit pattern (at least 4 either side);
 * the stream is synchronised, the block read back and every guard compared: one that changed is SIM3OPT_ERR_STATE, the
 * message names the rank and the index relative to the operand, and the handle is finished (device memory was written
 * that nobody owned).  The scratch blocks are returned before the call returns; the mailboxes may grow and stay with
 * the handle, as in a run; the engine's vectors, scalars and estimates are not touched.  With options.time_kernels the
 * collective is counted in sim3opt_get_comm_times like any other.
 * Refusals are decided on the host for all ranks at once, before any rank enters the collective, and leave the handle as
 * it was: SIM3OPT_ERR_STATE unless the handle is initialised and sim3opt_set_devices gave it more than one rank (and for a
 * finished handle, as everywhere); SIM3OPT_ERR_ARG for a NULL pointer, a phase other than 0 / 1, an op other than 0 / 1,
 * n < 0 (or beyond 2^30), offsets that decrease or start below 0, and exchange plans that disagree.  n = 0 and plans
 * without a double are valid: the ranks meet at the barrier and nothing else changes.
 * (sim3opt_version is unchanged: diagnostics are not part of the versioned interface.) */
/* Diagnostic.  in and out: world x n doubles, row r is rank r's operand before and after.  op: 0 sum (a left fold in
 * rank order, ((s0 + s1) + s2) + ..., no contraction), 1 max (a NaN wins, as numpy.maximum has it). */
int sim3opt_comm_apply_allreduce(sim3opt_graph* g, int64_t n, int32_t op, int32_t phase, const double* in, double* out);
/* Diagnostic.  offs[0 .. world], offs[0] = 0, never decreasing: rank r owns [offs[r], offs[r + 1]) of a vector of
 * offs[world] doubles.  in and out: world x offs[world] doubles, row r is rank r's whole vector before and after (what
 * it holds outside its own span before the call is replaced by the owners' spans). */
int sim3opt_comm_apply_allgatherv(sim3opt_graph* g, const int64_t* offs, int32_t phase, const double* in, double* out);
/* Diagnostic.  soffs and roffs: world rows of world + 1 offsets, row r is rank r's plan: it sends
 * [soffs[r][p], soffs[r][p + 1]) of its send buffer (soffs[r][world] doubles) to rank p and receives rank p's segment
 * into [roffs[r][p], roffs[r][p + 1]) of its receive buffer (roffs[r][world] doubles); rank p's count for q must be q's
 * count from p.  A row may start above 0: what lies in front of the first segment is not part of the exchange.  send:
 * the ranks' send buffers one after the other (checked to come back unchanged); recv: the ranks' receive buffers one
 * after the other, read AND written: what no segment covers keeps the caller's numbers. */
int sim3opt_comm_apply_exchange(sim3opt_graph* g, const int64_t* soffs, const int64_t* roffs, int32_t send_phase,
                                int32_t recv_phase, const double* send, double* recv);
/* Diagnostic.  out = {capacity of a mailbox in doubles, collectives so far (barrier waits: an exchange that grows the
 * mailboxes counts 3)} of rank 0; both are the same on every rank.  Same SIM3OPT_ERR_STATE rule as above. */
int sim3opt_comm_local_state(sim3opt_graph* g, int64_t out[2]);

/* Returns the device blocks the library keeps for re-use (graphs that are re-initialised after growing
 * by an edge find their predecessor's buffers, csrc/devmem.cpp; at most 1 GB) to the HIP runtime, together
 * with the idle streams, events and pinned host blocks (<= 64 MB) it recycles the same way.
 * Called automatically when the last sim3opt_graph / sim3opt_ba handle of the process is destroyed;
 * call it yourself before allocating large device buffers of your own next to a live handle. */
void sim3opt_release_device_cache(void);
/* Diagnostic.  out = {blocks, bytes} of device memory the library has handed to its handles and calls and not got
 * back: every live sim3opt_graph / sim3opt_ba / sim3opt_ba_batch / sim3opt_pnp_batch / sim3opt_match_batch / sim3opt_place_batch / sim3opt_vocabulary / sim3opt_surf_batch of the process, on all
 * devices; bytes as the block cache rounds them.  Blocks waiting in the cache for re-use are not counted.  The same before and after any call
 * that creates no handle and initialises none is what "this call keeps no device memory" means
 * (tests/test_gpu_device_memory.py). */
void sim3opt_device_memory_in_use(int64_t out[2]);
/* Test mode of the block cache (tests/test_gpu_stale_memory.py); off by default, switched by this call alone, process-wide.
 * Recycled blocks are not cleared and sizes are rounded up by up to 12.5 %: a kernel that reads what nobody wrote, or
 * writes past an array's end into the block's own slack, is silent.  While the mode is on every block handed out -- of
 * every handle and every call, on every device -- is 256 to about 12.5 % bytes longer than asked for; the bytes asked
 * for are filled with 0xFF (a quiet NaN as float and as double) where the elements are floating point and with 0
 * where they are not, the tail behind them with 0xA5; when the block comes back the tail is compared with 0xA5.
 *   covered:     floating-point reads before writes (the result turns NaN or differs from a run with the mode off),
 *                writes into a block's own slack (counted by the report below)
 *   not covered: integer arrays (a stale integer may be an index; a poison must not send a load elsewhere), LDS, pinned
 *                host memory, accesses outside the block
 * Blocks handed out while the mode was off are not checked, so it may be switched while handles live.  Every
 * allocation then synchronises its device: for tests only.  To run a new handle type under it: build it, run it, read
 * everything out and close it once with the mode off and once with it on (sim3opt_release_device_cache before each) and
 * compare the bytes; the report must show no overwritten tail and as many blocks checked as filled. */
void sim3opt_debug_device_memory(int32_t on);
/* out = {blocks filled, blocks checked when they came back, blocks whose tail was overwritten, offset past the requested
 * size of the first overwritten byte of the first such block or -1}, since the mode was last switched on. */
void sim3opt_debug_device_memory_report(int64_t out[4]);
/* Shows that the check can fail, with no access outside a block: takes a block of `bytes` bytes from the cache (floating:
 * its elements count as floating point) on the current device, sets `overrun` bytes from offset `bytes` on (refused with
 * SIM3OPT_ERR_ARG if they would leave the block), copies the block's first out_len bytes to `out` and gives the block
 * back.  Returns the block's size in bytes, or an error code (< 0). */
int64_t sim3opt_debug_device_memory_probe(int64_t bytes, int32_t floating, int64_t overrun, unsigned char* out,
                                          int64_t out_len);

/* ---- reference-format I/O (host C++; the callers either side of the path) ---- */
/* Builds the graph of testDirectSim3Optimization                   kitti_surf.cpp:562-670
 * from <dir>/cc.txt, <dir>/framePoses.txt (or framePoses_kf.txt), <dir>/loopConstraints.txt. */
int sim3opt_load_kitti_direct(sim3opt_graph* g, const char* dir, int32_t use_one_constraint);
/* Consistency graph against numbers the reference wrote itself: vertices = the KITTI ground-truth
 * poses (<dir>/gt_kf.txt, or 00.txt; 3x4 Pc2w rows, kitti_surf.cpp:1164-1190) as S_iw = (Rw2c, tw2c, 1);
 * edges = line 1 of every <dir>/loopConstraints.txt record, i.e. DCM2Euler(Pw2c[f2] Pw2c[f1]^-1) + its
 * translation as the reference's detector printed them from the same ground truth
 * (kittiDetector.h:1051-1060), v0 = frame 1, v1 = frame 2, scale 1.  Every residual of this graph
 * vanishes to the 8 decimals of the file iff the Euler convention, compose, inverse and edge
 * orientation used by sim3opt_load_kitti_direct are the reference's.  Host only. */
int sim3opt_load_kitti_gt_loops(sim3opt_graph* g, const char* dir);
/* Writes "kfid s tx ty tz qx qy qz qw" rows (S_wi of each estimate)  kitti_surf.cpp:678-701;
 * precision: 17 significant digits (the reference prints 6). image_ids may be NULL. */
int sim3opt_write_poses(sim3opt_graph* g, const char* path, const int32_t* image_ids);

/* ---- interchange formats and map re-anchoring ----
 * KeyFrame .bin reader: LoadComboKeyFrame                            drawPTAMPoints.cpp:33-84
 * Two-call pattern: with capacity < *n_obs only the header (id, Rw2c row-major, twinc, n_obs) is
 * returned; point_ids / points_w (n x 3) / obs_uv (n x 2) are filled when capacity >= n_obs. */
int sim3opt_read_keyframe_bin(const char* path, int32_t* kf_id, double Rw2c[9], double twinc[3],
                              int32_t* n_obs, uint32_t* point_ids, double* points_w, double* obs_uv,
                              int32_t capacity);
/* figureKITTIBA's re-anchoring                                        drawPTAMPoints.cpp:416-429
 * points[k] <- S_new(f)^-1 * (R_old(f) points[k] + t_old(f)), f = keyframe of the point's LAST
 * observation in (obs_frame, obs_point) order; unobserved points keep their coordinates.
 * old_Rt: n_frames x 12 (R row-major, then t); new_states: n_frames x 8 (S_iw).  Runs on the GPU. */
int sim3opt_reanchor_points(int32_t n_frames, const double* old_Rt, const double* new_states,
                            int32_t n_points, double* points, int32_t n_obs,
                            const int32_t* obs_frame, const int32_t* obs_point, int32_t device);
/* BAL problem file (ceres-solver format) handed from figureKITTIBA to ba_demo:
 * SaveBALFile                                                          drawPTAMPoints.cpp:218-283
 * Rw2c: n_cams x 9 row-major, tw2c: n_cams x 3, points: n_points x 3, observations as (camera,
 * point, u, v).  Point ids must be exactly 0..n_points-1 (SIM3OPT_ERR_ARG otherwise; the reference
 * exits).  Host only. */
int sim3opt_write_bal(const char* path, int32_t n_cams, const double* Rw2c, const double* tw2c,
                      const double f_k1_k2[3], int32_t n_points, const double* points,
                      int32_t n_obs, const int32_t* obs_cam, const int32_t* obs_point,
                      const double* obs_uv);
/* g2o text export (VERTEX_SIM3:EXPMAP / EDGE_SIM3:EXPMAP / FIX) of a graph with ids 0..n-1 and
 * identity information, for re-running it in stock g2o */
int sim3opt_write_g2o(sim3opt_graph* g, const char* path);

/* ---- bundle adjustment hand-off: the reference's ba_demo on the GPU ----
 * bal_example.cpp:44-243: g2o::VertexSE3Expmap cameras (T_w2c), g2o::VertexSBAPointXYZ points
 * (marginalised), g2o::EdgeProjectXYZ2UV with ONE fixed g2o::CameraParameters(f, pp, 0) (:90-97),
 * information I / pixel_noise^2 (:147), g2o::RobustKernelHuber(2.5) (:149-153), Levenberg-Marquardt
 * over BlockSolver_6_3 + LinearSolverEigen (:76-88), optimize(maxIterations) (:213).  No vertex is
 * fixed (the reference fixes none); the damping carries the gauge, as it does there.
 * Device pipeline: sim3opt_amd/csrc/ba.hip.  No CPU fallback: SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_ba sim3opt_ba;

typedef struct sim3opt_ba_options {
  double huber_delta;       /* RobustKernelHuber delta; 0 = no robust kernel      default 2.5  :151 */
  double pixel_noise;       /* information = I / pixel_noise^2                     default 1.0  :62  */
  double tau;               /* lambda_0 = tau * max diag(H)                        default 1e-5      */
  double user_lambda_init;  /* > 0: used instead                                   default 0         */
  int32_t max_trials;       /* LM trials per iteration                             default 10        */
  int32_t pcg_max_iters;    /* reduced camera system; 0 = automatic                default 0         */
  double pcg_rel_tol;       /* |r|_M / |r0|_M of the reduced system                default 1e-12     */
  int32_t linear_solver;    /* reduced camera system: -1 automatic (exact block Cholesky unless one
                               factorisation needs > 8 M block products), 1 exact or fail, 0 block-Jacobi
                               PCG                                                 default -1   :76-80 */
  int32_t device;           /* HIP device ordinal, -1 = current                    default -1        */
  int32_t verbose;          /* one line per LM iteration on stderr                 default 0    :72  */
} sim3opt_ba_options;

void sim3opt_ba_options_default(sim3opt_ba_options* o);
sim3opt_ba* sim3opt_ba_create(void);
void sim3opt_ba_destroy(sim3opt_ba* b);
const char* sim3opt_ba_last_error(const sim3opt_ba* b);
int sim3opt_ba_set_options(sim3opt_ba* b, const sim3opt_ba_options* o);
/* cameras: n_cams x 7 [qx qy qz qw tx ty tz] of T_w2c (the SE3Quat of :170-172); points n x 3;
 * observations (camera index, point index, u, v) as the BAL rows (:134-158).  Indices out of range
 * -> SIM3OPT_ERR_ARG (the reference asserts).  focal / cx / cy: the fixed CameraParameters. */
int sim3opt_ba_set_problem(sim3opt_ba* b, int32_t n_cams, const double* cam_qt, int32_t n_points,
                           const double* points, int32_t n_obs, const int32_t* obs_cam,
                           const int32_t* obs_point, const double* obs_uv, double focal, double cx,
                           double cy);
/* OptimizableGraph::Vertex::setFixed on cameras (n_cams flags; ba_demo itself fixes none).  A fixed
 * camera keeps its estimate and leaves the linear system. */
int sim3opt_ba_set_fixed_cameras(sim3opt_ba* b, const uint8_t* fixed);
/* the BAL file ba_demo takes as argv[1] (:104-189; per-camera f, k1, k2 are read and ignored as
 * there: the projection uses the fixed focal / cx / cy) */
int sim3opt_ba_read_bal(sim3opt_ba* b, const char* path, double focal, double cx, double cy);
int sim3opt_ba_dims(const sim3opt_ba* b, int32_t* n_cams, int32_t* n_points, int32_t* n_obs);
/* robustified chi2 of the current estimates (SparseOptimizer::activeRobustChi2) */
int sim3opt_ba_chi2(sim3opt_ba* b, double* chi2);
/* LM iterations performed (g2o's return convention: 0 on failure, -1 for an empty problem) */
int sim3opt_ba_optimize(sim3opt_ba* b, int32_t max_iters);
int sim3opt_ba_get_cameras(const sim3opt_ba* b, double* cam_qt /* n_cams x 7 */);
int sim3opt_ba_get_points(const sim3opt_ba* b, double* points /* n_points x 3 */);
int32_t sim3opt_ba_num_iterations(const sim3opt_ba* b);
int sim3opt_ba_get_stats(const sim3opt_ba* b, int32_t iter, sim3opt_iter_stats* out);
/* "% SE3 optimization result: kf id, tcinw, rc2w(qxyzw)" rows                        :223-238 */
int sim3opt_ba_write_poses(const sim3opt_ba* b, const char* path);

/* ---- read-outs of the bundle adjuster's intermediates, for tests ----
 * Contract of all five: nothing in the solver uses them; they run the launch code of sim3opt_ba_optimize on the
 * current estimate (uploading the problem first if need be), copy device buffers to the host and leave the estimate,
 * the statistics and every later sim3opt_ba_optimize / sim3opt_ba_chi2 result bit for bit what they are without the
 * call.  Camera vectors hold 7 doubles per camera [omega, upsilon, pad]; blocks are 7 x 7, column-major (entry (r, c)
 * at r + 7 c), the 7th row / column zero but for a 1 at (6, 6) of the diagonal blocks.  SIM3OPT_ERR_STATE without a problem, SIM3OPT_ERR_ARG for a
 * NULL output that is not marked optional or a non-finite lambda; the message is in sim3opt_ba_last_error. */
/* Diagnostic.  Block-CSR pattern of the reduced camera system: *n_blocks, rptr (n_cams + 1), bcol (n_blocks), the
 * diagonal block first in every row.  rptr = bcol = NULL: the size query. */
int sim3opt_ba_debug_pattern(sim3opt_ba* b, int32_t* n_blocks, int32_t* rptr, int32_t* bcol);
/* Diagnostic.  The linearisation of the current estimate as k_ba_obs writes it: n_obs x 20 = [A = sqrt(w) J_cam
 * (2 x 6 row-major), B = sqrt(w) J_point (2 x 3 row-major), es = sqrt(w) e], w = Huber weight / pixel_noise^2. */
int sim3opt_ba_debug_linearization(sim3opt_ba* b, double* lin);
/* Diagnostic.  The reduced system of an LM trial with damping `lambda` (k_ba_obs, k_ba_points, k_ba_obs2,
 * k_ba_reduced, the max-diagonal part of k_ba_final).  Every output may be NULL, not all of them:
 * S (n_blocks x 49), g and b_c (n_cams x 7), Hpp_inv = (H_pp + lambda I)^-1 (n_points x 9), b_p (n_points x 3),
 * Z = (A^T B) Hpp_inv (n_obs x 18, 6 x 3 row-major), point_maxdiag (n_points) and cam_maxdiag (n_cams x 7): the
 * undamped diagonals' maxima per point / entries per camera, *maxdiag: the maximum over both. */
int sim3opt_ba_debug_reduced(sim3opt_ba* b, double lambda, double* S, double* g, double* b_c, double* Hpp_inv,
                             double* b_p, double* Z, double* point_maxdiag, double* cam_maxdiag, double* maxdiag);
/* Diagnostic.  The step of an LM trial with damping `lambda`: the reduced system as above, S dx_c = g by solver = 1
 * the exact block Cholesky (SIM3OPT_ERR_STATE when the problem was initialised without its plan) or solver = 0
 * k_ba_pcg with at most pcg_max_iters iterations (0: automatic) to pcg_rel_tol -- a cap of k returns the iterate
 * x_k --, then dx_p by k_ba_backsub.  dx_c (n_cams x 7), dx_p (n_points x 3) and *fail (a breakdown of the PCG or a
 * non-positive pivot: the step is then meaningless, the return code still SIM3OPT_OK) are required; pcg_iters and
 * pcg_rel may be NULL.  The estimate is not moved. */
int sim3opt_ba_debug_step(sim3opt_ba* b, double lambda, int32_t solver, int32_t pcg_max_iters, double pcg_rel_tol,
                          double* dx_c, double* dx_p, int32_t* pcg_iters, double* pcg_rel, int32_t* fail);
/* Diagnostic.  What an LM trial makes of a caller's step dx_c (n_cams x 7), dx_p (n_points x 3), any numbers:
 * the estimate k_ba_update produces (cam_qt n_cams x 7, points n_points x 3), its robustified chi2 (k_ba_chi2,
 * k_ba_final) and scale = x . (lambda x + b) over cameras and points (k_ba_scale, k_ba_final; b = b_c, b_p of the
 * current estimate).  with_fail != 0 runs the update with the trial's fail flag set: nothing may move.  The estimate
 * is then restored from the trial's backup buffers.  The four outputs may be NULL, not all of them. */
int sim3opt_ba_debug_update(sim3opt_ba* b, const double* dx_c, const double* dx_p, double lambda, int32_t with_fail,
                            double* cam_qt, double* points, double* chi2, double* scale);

/* ---- Bundle-adjustment covariances: cameras and points by selected inversion (g2o's computeMarginals) ----
 * Definition.  H = J^T W J at the CURRENT estimates, with the Huber weights and 1 / pixel_noise^2 exactly as k_ba_obs
 * forms them; the tangent order is the update's, [omega, upsilon] per camera (T <- exp(.) T), xyz per point.  Fixed
 * cameras are removed.  lambda >= 0 is added to every diagonal entry, cameras and points (the caller's prior;
 * computeMarginals is lambda = 0).  With Sigma = (H + lambda I)^-1:
 *   camera-camera block (a, b), 6 x 6:  Sigma_cc = S^-1, S the reduced camera system of an LM trial with damping lambda.
 *     Answered for a camera with itself and for every pair on the pattern of the factor of S; every two cameras that
 *     share a point are on it.  A pair outside it: SIM3OPT_ERR_ARG, nothing written (as sim3opt_marginals).  A fixed
 *     camera on either side: the block is exactly +0 (a fixed camera stays a row of S, an identity row, so its block
 *     of S^-1 is not its covariance and is masked).
 *   point block p, 3 x 3:  Sigma_pp = H_pp^-1 + sum over a, b in obs(p) of Z_a^T Sigma_cc[cam(a), cam(b)] Z_b, over ALL
 *     ordered pairs of the point's observations in the order of its observation list (ascending observation index; a
 *     outer, b inner), H_pp^-1 = (H_pp + lambda I)^-1 and Z_o = (A^T B)_o H_pp^-1 as sim3opt_ba_debug_reduced returns them.
 *     Blocks with a fixed camera contribute nothing.  The result is symmetrised once, (M + M^T) / 2: symmetric bit for bit.
 *   point-camera block (p, c), 3 x 6:  Sigma_pc = - sum over a in obs(p) of Z_a^T Sigma_cc[cam(a), c].  c fixed: +0.  A
 *     needed camera pair outside the pattern (possible only when c does not observe p): SIM3OPT_ERR_ARG.
 * All blocks are column-major (entry (r, c) at r + rows c): 36, 9 and 18 doubles per block.
 * Singular system: SIM3OPT_ERR_STATE, nothing written, never NaN -- a non-positive pivot of the factorisation of S, a
 * pivot of it below 1e-13 max |H_dd| (the selected inversion's test), a non-finite result, or ANY point of the problem
 * (requested or not: every point enters S) whose H_pp + lambda I fails its pivot test: the 3 x 3 LDL^T in x, y, z order
 * with a pivot <= 1e-13 x the point's largest undamped diagonal entry, or <= 0; the message names the lowest such
 * point.  A map with points seen once, with a free camera nobody observes with, or with no fixed camera therefore
 * wants lambda > 0.  (S is stored in 7 x 7 blocks with a unit pad, and a fixed camera is an identity row; where
 * max |H_dd| exceeds 1e13 those ones would fail the selected inversion's relative pivot test.  Before factoring, the
 * call sets the pads and the fixed cameras' diagonals to max(1, max |H_dd|): they couple to nothing, so the 6 x 6 blocks
 * of S^-1 keep their bits, and they pass the test at every scale.)
 * No side effects: the call factors in a context of its own (built at the first call; a refused plan -- more block
 * products than SIM3OPT_BA_COV_MAX_PAIRS, else SIM3OPT_BA_MAX_PAIRS, else 30 M -- is SIM3OPT_ERR_STATE, remembered until
 * the problem changes) and leaves the LM's factorisation, the estimate, the statistics and every later
 * sim3opt_ba_optimize / sim3opt_ba_chi2 / read-out result bit for bit what they are without it, under either linear
 * solver.  Deterministic: no floating-point atomics, fixed summation orders; the bits of a block depend neither on the
 * order, duplicates or split of the request nor on the schedule knobs SIM3OPT_BA_SUBTREE / SIM3OPT_BA_WG_SUB.
 * One call runs one linearisation, one factorisation and one selected inversion for its three requests (camera pairs
 * cam_a / cam_b -> cov_cc n_cc x 36; points -> cov_pp n_pp x 9; (pc_point, pc_cam) -> cov_pc n_pc x 18); any of them may
 * be empty (count 0, arrays NULL).  Unknown indices, a non-finite or negative lambda: SIM3OPT_ERR_ARG; no problem set:
 * SIM3OPT_ERR_STATE. */
int sim3opt_ba_covariances(sim3opt_ba* b, double lambda, int32_t n_cc, const int32_t* cam_a, const int32_t* cam_b,
                           double* cov_cc, int32_t n_pp, const int32_t* point, double* cov_pp, int32_t n_pc,
                           const int32_t* pc_point, const int32_t* pc_cam, double* cov_pc);
/* of the last sim3opt_ba_covariances that got as far as its plan: columns of the factor, blocks of L / Z, 7x7x7 products
 * of the factorisation, of the selected inversion, ordered observation pairs summed for the distinct requested points
 * (pairs with a fixed camera left out), 1 when the selected inversion ran */
int sim3opt_ba_covariance_stats(const sim3opt_ba* b, int64_t out[6]);
/* Diagnostic.  The pattern of the covariances' factor (built if need be): *nb columns (the cameras), *nL stored blocks,
 * *ngroups workgroups of its schedule; perm (nb: the camera eliminated at position j), colptr (nb + 1) and lrow (nL:
 * the rows, as positions, of column j's blocks, the diagonal first, ascending) may be NULL (the size query).  Camera
 * pair (a, b) is answered iff block (max(pos a, pos b), min(pos a, pos b)) is stored. */
int sim3opt_ba_covariance_plan(sim3opt_ba* b, int32_t* nb, int64_t* nL, int32_t* ngroups, int32_t* perm, int32_t* colptr,
                               int32_t* lrow);

/* ---- batched two-view bundle adjustment: the loop detector's refinement, every candidate in one launch ----
 * BAOptimize (kittiDetector.h:845-954, helpers :712-788), which the detector calls once per accepted loop
 * candidate (:1325) and whose result is line 4 of a loopConstraints.txt record: two VertexSE3Expmap cameras, the
 * first fixed (:861-870), the matched points as VertexSBAPointXYZ (:892-894), two EdgeProjectXYZ2UV observations
 * per point with information I and RobustKernelHuber (:753-770, :895-901), LM over BlockSolver_6_3 (:716-731).
 * Problem k owns the points point_ptr[k] .. point_ptr[k+1]-1; all problems share one CameraParameters.  Device
 * pipeline: sim3opt_amd/csrc/ba_batch.hip, one workgroup per problem, the whole LM loop on the device.  A
 * problem's result does not depend on the other problems of the batch or on its place among them.  No CPU
 * fallback: SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_ba_batch sim3opt_ba_batch;

typedef struct sim3opt_ba_batch_options {
  double huber_delta;       /* RobustKernelHuber delta; 0 = no robust kernel   default 3.0    :1325 OptParams(10, true, 3) */
  double pixel_noise;       /* information = I / pixel_noise^2                  default 1.0    :758-764 (weight = 1)        */
  double tau;               /* lambda_0 = tau * max diag(H) when user_lambda_init <= 0         default 1e-5                */
  double user_lambda_init;  /* > 0: lambda_0                                    default 50.0   :779-782 setUserLambdaInit   */
  double outlier_chi2;      /* an observation above it counts as an outlier     default 5.995  :847, :947-953               */
  int32_t max_iters;        /* LM iterations                                    default 10     :1325, :786                  */
  int32_t max_trials;       /* LM trials per iteration                          default 5      :730 setMaxTrialsAfterFailure */
  int32_t device;           /* HIP device ordinal, -1 = current                 default -1                                  */
} sim3opt_ba_batch_options;

void sim3opt_ba_batch_options_default(sim3opt_ba_batch_options* o);
sim3opt_ba_batch* sim3opt_ba_batch_create(void);
void sim3opt_ba_batch_destroy(sim3opt_ba_batch* b);
const char* sim3opt_ba_batch_last_error(const sim3opt_ba_batch* b);
/* SIM3OPT_ERR_ARG, nothing changed: max_iters < 1, max_trials < 1, pixel_noise <= 0, tau <= 0, huber_delta < 0, a
 * non-finite value. */
int sim3opt_ba_batch_set_options(sim3opt_ba_batch* b, const sim3opt_ba_batch_options* o);
/* The arguments of BAOptimize (:845-846) for n_problems candidates at once: point_ptr (n_problems + 1, ragged,
 * point_ptr[0] = 0), cam0 (n x 7 [qx qy qz qw tx ty tz] of T_w2c, fixed; the reference's is the identity, :861-869),
 * cam1 (n x 7, the start: Rf2s and tfins, :873-887), points (total x 3 in camera 0's world: pointsXYZ), uv0 / uv1
 * (total x 2: points1 / points2), focal / cx / cy of K (:850-854).  Quaternions are normalised as
 * sim3opt_ba_set_problem normalises them.  SIM3OPT_ERR_ARG with nothing changed: n_problems < 1, a problem with no
 * point, a non-monotone point_ptr, a non-finite number, a zero quaternion, focal <= 0, a NULL array. */
int sim3opt_ba_batch_set_problems(sim3opt_ba_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                  const double* cam0, const double* cam1, const double* points, const double* uv0,
                                  const double* uv1, double focal, double cx, double cy);
int sim3opt_ba_batch_dims(const sim3opt_ba_batch* b, int32_t* n_problems, int32_t* total_points);
/* runSparseBAOptimizer (:772-788) of every problem, ONE kernel launch for the batch.  Returns the number of
 * problems optimised, or a negative SIM3OPT_ERR_* (SIM3OPT_ERR_STATE: no problems set).  The estimates move:
 * another call continues from them, sim3opt_ba_batch_set_problems starts again. */
int sim3opt_ba_batch_optimize(sim3opt_ba_batch* b);
/* cam0 (n x 7, exactly as given) and / or cam1 (n x 7: Rf2s, tfins of :915-921); either may be NULL */
int sim3opt_ba_batch_get_cameras(const sim3opt_ba_batch* b, double* cam0, double* cam1);
int sim3opt_ba_batch_get_points(const sim3opt_ba_batch* b, double* points /* total x 3 */);
/* LM iterations problem `problem` ran in the last optimize, and their records (chi2_before, chi2_after, lambda,
 * rho, trials; the other fields 0) */
int32_t sim3opt_ba_batch_num_iterations(const sim3opt_ba_batch* b, int32_t problem);
int sim3opt_ba_batch_get_stats(const sim3opt_ba_batch* b, int32_t problem, int32_t iter, sim3opt_iter_stats* out);
/* lambda_0 of every problem in the last optimize (n): user_lambda_init, or computeLambdaInit's tau * max diag(H)
 * over camera 1 and the points.  SIM3OPT_ERR_STATE before the first optimize. */
int sim3opt_ba_batch_get_lambda_init(const sim3opt_ba_batch* b, double* lambda_init);
/* Of the last optimize, per problem: g2o's activeChi2 (not robustified) before and after, which the reference
 * prints (:785-787, :907), active_before / active_after (n each); e->chi2() of every observation at the final
 * estimate, edge_chi2 (total x 2: camera 0's, camera 1's observation of each point, the order of `edges`, :891-902);
 * the observations above outlier_chi2, n_outlier_edges (n; :947-953).  Each may be NULL, not all.
 * SIM3OPT_ERR_STATE before the first optimize. */
int sim3opt_ba_batch_get_chi2(const sim3opt_ba_batch* b, double* active_before, double* active_after,
                              double* edge_chi2, int32_t* n_outlier_edges);
/* Diagnostic read-out of ONE LM trial of every problem, in one launch, at the current estimate (the start before
 * the first optimize, else its result): the linearisation (pass L), the elimination of the points at the caller's
 * damping lambda[k] (pass S; n values, any finite number, negative allowed), the 6x6 Cholesky, and the back-
 * substitution with the trial's chi2 (pass U) -- the device functions sim3opt_ba_batch_optimize runs, not copies of
 * them.  With dx_c (n x 6, [omega, upsilon]; may be NULL) pass U uses that camera step instead of the Cholesky's, which
 * is still reported.  Nothing in the solver uses this call and it changes nothing: the estimates, the results of the
 * last optimize and the handle's device blocks stay; its own device memory is gone when it returns.
 *   point_rows   (SIM3OPT_BA_BATCH_TRIAL_POINT_ROWS x total, row r of point g at [r * total + g]) the kernel's scratch:
 *                rows 0-5 H_pp (undamped; xx xy xz yy yz zz), 6-8 b_p, 9-20 A_1 (2 x 6 row-major), 21-26 B_1 (2 x 3),
 *                27-28 es_1, 29-34 H_pp^-1 (damped; as H_pp), 35-52 Z (6 x 3 row-major), 53-55 the trial point
 *   problem_rows (n x SIM3OPT_BA_BATCH_TRIAL_PROBLEM_DOUBLES) 0-20 sum A_1^T A_1 (upper triangle, row by row), 21-26
 *                b_c, 27 the robust chi2, 28 activeChi2, 29 computeLambdaInit's max diag(H) (whatever
 *                user_lambda_init is), 30-50 - sum Z Y^T, 51-56 - sum Z b_p, 57-77 the damped S, 78-83 g, 84-89 dx_c
 *                of the Cholesky, 90 fail (1: a non-positive pivot), 91-97 the trial camera 1, 98 the trial's robust
 *                chi2, 99 x.(lambda x + b) over the points and the camera
 * A failed trial does what the LM loop does: pass U is skipped, the trial camera is the current one, its chi2 DBL_MAX,
 * the scale and the trial points 0.  Either output may be NULL, not both.  SIM3OPT_ERR_STATE: no problems set.
 * SIM3OPT_ERR_ARG with a message: lambda NULL, both outputs NULL, a non-finite lambda or dx_c. */
#define SIM3OPT_BA_BATCH_TRIAL_POINT_ROWS 56
#define SIM3OPT_BA_BATCH_TRIAL_PROBLEM_DOUBLES 100
int sim3opt_ba_batch_debug_trial(sim3opt_ba_batch* b, const double* lambda, const double* dx_c, double* point_rows,
                                 double* problem_rows);

/* ---- batched PnP RANSAC: the loop detector's start pose, every candidate in one launch ----
 * cv::solvePnPRansac(surfPoints[0], points2, K, dist, rvec, tvec, false, 100, 3, 10, noArray(), CV_ITERATIVE)
 * (kittiDetector.h:1300-1301), which the detector calls once per accepted loop candidate before BAOptimize (:1325)
 * and whose result is line 3 of a loopConstraints.txt record: camera 1 (T_w2c of camera 0's frame) from camera 0's
 * 3-D points and camera 1's pixels.  Its poses are the cam1 the batched two-view refinement above starts from.
 * PARITY UNPINNED: the reference stores the outputs of its PnP runs, not their inputs, and OpenCV's sampling is not
 * reproducible.  What is OpenCV's here: the order of the steps and the inlier criterion, squared reprojection error
 * <= reproj_error^2.  What is not: hypotheses are closed-form P3P solutions of three points, chosen by a fourth
 * (OpenCV: EPnP); all `iterations` hypotheses are evaluated (OpenCV stops early on its confidence estimate); the
 * sampler is counter-based -- draw j of hypothesis h is splitmix64 of seed + (4 h + j + 1) * 0x9E3779B97F4A7C15
 * modulo n - j, stepped over the earlier picks -- so a seed gives the same samples everywhere; the final refit is a
 * Levenberg-Marquardt on camera 1 over the best hypothesis's inliers (OpenCV: CV_ITERATIVE).  Device pipeline:
 * sim3opt_amd/csrc/pnp_batch.hip, one workgroup per problem, one launch.  A problem's result does not depend on the
 * other problems of the batch or on its place among them.  No CPU fallback: SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_pnp_batch sim3opt_pnp_batch;

typedef struct sim3opt_pnp_batch_options {
  double reproj_error;      /* inlier: squared error <= reproj_error^2 [px]      default 3.0    :1301 reprojectionError     */
  double tau;               /* refit: lambda_0 = tau * max diag(H)              default 1e-5                                */
  uint64_t seed;            /* of the sampler                                   default 0                                   */
  int32_t iterations;       /* hypotheses per problem, 1..4096                  default 100    :1301 iterationsCount        */
  int32_t min_inliers;      /* fewer final inliers: status 3                    default 10     :1301 minInliersCount        */
  int32_t min_points;       /* fewer points: status 1, nothing run; >= 4        default 9      :1282 point_count > 8        */
  int32_t refine_iters;     /* LM iterations of the refit, 0 = no refit         default 10                                  */
  int32_t max_trials;       /* LM trials per iteration                          default 5                                   */
  int32_t device;           /* HIP device ordinal, -1 = current                 default -1                                  */
} sim3opt_pnp_batch_options;

#define SIM3OPT_PNP_OK 0            /* a pose from at least min_inliers inliers                                  */
#define SIM3OPT_PNP_FEW_POINTS 1    /* fewer than min_points points: nothing run, the pose is the identity       */
#define SIM3OPT_PNP_NO_HYPOTHESIS 2 /* no sample gave a pose: the pose is the identity                           */
#define SIM3OPT_PNP_FEW_INLIERS 3   /* fewer than min_inliers final inliers: the pose is returned all the same    */

void sim3opt_pnp_batch_options_default(sim3opt_pnp_batch_options* o);
sim3opt_pnp_batch* sim3opt_pnp_batch_create(void);
void sim3opt_pnp_batch_destroy(sim3opt_pnp_batch* b);
const char* sim3opt_pnp_batch_last_error(const sim3opt_pnp_batch* b);
/* SIM3OPT_ERR_ARG, nothing changed: iterations outside 1..4096, reproj_error <= 0, tau <= 0, min_points < 4,
 * min_inliers < 0, refine_iters < 0, max_trials < 1, a non-finite value. */
int sim3opt_pnp_batch_set_options(sim3opt_pnp_batch* b, const sim3opt_pnp_batch_options* o);
/* The arguments of the call at :1300 for n_problems candidates at once: point_ptr (n_problems + 1, ragged,
 * point_ptr[0] = 0), points (total x 3 in camera 0's frame: surfPoints[0]), uv1 (total x 2: points2), focal / cx / cy
 * of K (the reference's distortion is zero).  SIM3OPT_ERR_ARG with nothing changed: n_problems < 1, a problem with no
 * point, a non-monotone point_ptr, a non-finite number, focal <= 0, a NULL array.  A problem with fewer than
 * min_points points is accepted and ends with status 1. */
int sim3opt_pnp_batch_set_problems(sim3opt_pnp_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                   const double* points, const double* uv1, double focal, double cx, double cy);
int sim3opt_pnp_batch_dims(const sim3opt_pnp_batch* b, int32_t* n_problems, int32_t* total_points);
/* Every problem, ONE kernel launch for the batch.  Returns the number of problems with status 0, or a negative
 * SIM3OPT_ERR_* (SIM3OPT_ERR_STATE: no problems set); one problem's failure is its status, never the batch's. */
int sim3opt_pnp_batch_solve(sim3opt_pnp_batch* b);
/* The getters return SIM3OPT_ERR_STATE before the first solve.  cam1: n x 7 [qx qy qz qw tx ty tz] of T_w2c, the
 * layout the batched two-view refinement takes as its cam1 (rvec, tvec of :1300 as a quaternion). */
int sim3opt_pnp_batch_get_poses(const sim3opt_pnp_batch* b, double* cam1);
/* mask (total, 1 = inlier of the returned pose) and / or n_inliers (n); either may be NULL */
int sim3opt_pnp_batch_get_inliers(const sim3opt_pnp_batch* b, uint8_t* mask, int32_t* n_inliers);
/* Per problem (n each, each may be NULL): status (SIM3OPT_PNP_*), the index of the best hypothesis (-1: none), its
 * inlier count and the sum of its inliers' squared errors, the RMS error [px] of the final inliers, the LM
 * iterations the refit ran. */
int sim3opt_pnp_batch_get_summary(const sim3opt_pnp_batch* b, int32_t* status, int32_t* best_hypothesis,
                                  int32_t* n_inliers_hypothesis, double* cost_hypothesis, double* rms_px,
                                  int32_t* refine_iterations);
/* Diagnostics.  Each leaves the results of the last solve as they were.
 * What the last solve computed for `problem`, H = options.iterations hypotheses: sample (H x 4 point indices),
 * n_solutions (P3P solutions with positive depths), valid, pose (H x 7; the identity where not valid), count and cost
 * of the scoring (0 where not valid).  Each may be NULL.  SIM3OPT_ERR_STATE before the first solve. */
int sim3opt_pnp_batch_debug_hypotheses(sim3opt_pnp_batch* b, int32_t problem, int32_t* sample, int32_t* n_solutions,
                                       int32_t* valid, double* pose, int32_t* count, double* cost);
/* P (1..4096) supplied poses per problem (poses: n x P x 7, any numbers) through the scoring code of k_pnp_ransac:
 * count and cost (n x P each, one may be NULL). */
int sim3opt_pnp_batch_debug_score(sim3opt_pnp_batch* b, int32_t P, const double* poses, int32_t* count, double* cost);
/* The refit of k_pnp_ransac from a supplied pose per problem (poses: n x 7, finite) on a supplied inlier set (mask:
 * total): pose_out (n x 7), the LM iterations run (n), chi2 (n x 2: the masked points' sum of squared errors before and
 * after) and trials (n x refine_iters, 0 for iterations not run).  The outputs may be NULL. */
int sim3opt_pnp_batch_debug_refine(sim3opt_pnp_batch* b, const double* poses, const uint8_t* mask, double* pose_out,
                                   int32_t* iterations, double* chi2, int32_t* trials);
/* Host, doubles.  "compute scale change" of :1305-1311 for n_problems candidates: ratio[k] = the element at index
 * floor(0.5 n) of problem k's sorted depth1 over the same element of its sorted depth0 (sloop, the second number of a
 * loopConstraints.txt record's line 3).  SIM3OPT_ERR_ARG: as for point_ptr above, a NULL array, a non-finite depth. */
int sim3opt_median_depth_ratio(int32_t n_problems, const int32_t* point_ptr, const double* depth0,
                               const double* depth1, double* ratio);

/* ---- batched essential-matrix RANSAC: the loop detector's two-view pose without depths, every candidate in one launch ----
 * ExtractCameras(points1, points2, Rf2s, tfins, K) (kittiDetector.h:279-293, called at :1161-1185):
 * cv::findEssentialMat(points1, points2, focal, pp, cv::RANSAC, 0.999, 1.0, mask), then cv::recoverPose(E, points1,
 * points2, R, t, focal, pp, mask).  Its result is line 2 of a loopConstraints.txt record: the match count, the Euler
 * angles of Rc12c2 and the unit translation.  It is the one pose of the chain that does not use the map's depths.
 * PARITY UNPINNED: the reference stores the outputs of its runs, not the matched pixels they were given, and
 * OpenCV's sampling is not reproducible.  What is OpenCV's here: the order of the steps, the inlier criterion after
 * its normalisation by focal, the cheirality vote with its distance threshold and the narrowing of the mask.  What is
 * not: a hypothesis is the five-point solution chosen by a sixth point (OpenCV scores every solution); all
 * `iterations` hypotheses are evaluated (OpenCV stops early on its confidence 0.999); the sampler is counter-based;
 * the pose candidates come from a closed form and a least-squares triangulation (OpenCV: SVD, DLT).
 * Definition.
 * Coordinates: x = ((u - cx) / f, (v - cy) / f, 1) in double for both views; x1^T E x0 = 0, view 0 is uv0 (points1,
 * the first frame); the pose is Rc12c2, tc1inc2: X1 = R X0 + t, the convention of the PnP stage's cam1.
 * Sampler: draw j (0..5) of hypothesis h is splitmix64(seed + (6 h + j + 1) * 0x9E3779B97F4A7C15) modulo n - j,
 * stepped over the earlier picks in ascending order.  Points 0..4 make the hypothesis, point 5 chooses its solution.
 * Hypothesis: Nister's five-point method (four-dimensional null space of the 5 x 9 epipolar system; det E = 0 and
 * 2 E E^T E - tr(E E^T) E = 0 as a 10 x 20 matrix, eliminated with row pivoting; the degree-10 polynomial's real
 * roots by a Sturm chain with a fixed bisection depth and a fixed number of Newton steps; every solution polished by a
 * fixed number of Gauss-Newton steps on the ten cubics; up to ten E, each scaled to Frobenius norm 1).  Of the real
 * solutions the one with the smallest Sampson error on the sixth point.  Invalid (E = 0 stored, skipped): a repeated
 * point among the six (the same four coordinates), any pivot below its threshold (1e-12 in the 5 x 9 system and in
 * the 10 x 20 matrix, 1e-14 for a leading coefficient of the Sturm chain), no real root, a non-finite number.
 * Inlier: a0..2 = E x0, b0..1 = (E^T x1)_0..1, d = x1 . a, e2 = d^2 / (a0^2 + a1^2 + b0^2 + b1^2), every product and
 * sum rounded on its own, left to right (no fused multiply-add); inlier iff e2 <= (threshold / focal)^2.
 * Best: the largest inlier count, then the smallest cost (the sum of the inliers' e2), then the smallest index.
 * Pose: t is the unit vector spanning E's left null space whose component of largest magnitude (the first such) is
 * positive; Ra and Rb are the rotations with E = +s [t]x Ra and E = -s [t]x Rb, s > 0.  Candidates: 0 (Ra, t),
 * 1 (Rb, t), 2 (Ra, -t), 3 (Rb, -t).  The depths (z0, z1) of a correspondence under (R, t) are the least-squares
 * solution of z0 R x0 - z1 x1 = -t; an inlier of the best hypothesis votes for a candidate iff 0 < z0 < distance_threshold
 * and 0 < z1 < distance_threshold.  The candidate with the most votes wins, the lower index on a tie; the final mask is
 * the inliers that voted for it.
 * Device pipeline: sim3opt_amd/csrc/essential_batch.hip, one workgroup per problem, one launch.  A problem's result
 * does not depend on the other problems of the batch or on its place among them.  No CPU fallback:
 * SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_essential_batch sim3opt_essential_batch;

typedef struct sim3opt_essential_batch_options {
  double threshold;           /* inlier: Sampson e2 <= (threshold / focal)^2 [px]  default 1.0   :290 findEssentialMat's threshold */
  double distance_threshold;  /* a vote needs both depths below it, |t| = 1       default 50    :292 recoverPose [upstream-recall] */
  uint64_t seed;              /* of the sampler                                   default 0                                        */
  int32_t iterations;         /* hypotheses per problem, 1..4096                  default 1000  :290 maxIters [upstream-recall]    */
  int32_t min_points;         /* fewer points: status 1, nothing run; >= 6        default 9     :1163 point_count > 8              */
  int32_t device;             /* HIP device ordinal, -1 = current                 default -1                                       */
} sim3opt_essential_batch_options;

#define SIM3OPT_ESSENTIAL_OK 0            /* E, a pose and its inliers                                                    */
#define SIM3OPT_ESSENTIAL_FEW_POINTS 1    /* fewer than min_points points: nothing run, identity rotation, zero t, E = 0   */
#define SIM3OPT_ESSENTIAL_NO_HYPOTHESIS 2 /* no sample gave an E: likewise                                                */
#define SIM3OPT_ESSENTIAL_NO_POSE 3       /* no inlier in front of both cameras under any candidate: candidate 0, E kept   */

void sim3opt_essential_batch_options_default(sim3opt_essential_batch_options* o);
sim3opt_essential_batch* sim3opt_essential_batch_create(void);
void sim3opt_essential_batch_destroy(sim3opt_essential_batch* b);
const char* sim3opt_essential_batch_last_error(const sim3opt_essential_batch* b);
/* SIM3OPT_ERR_ARG, nothing changed: iterations outside 1..4096, threshold <= 0, distance_threshold <= 0,
 * min_points < 6, a non-finite value. */
int sim3opt_essential_batch_set_options(sim3opt_essential_batch* b, const sim3opt_essential_batch_options* o);
/* The arguments of the call at :1174 for n_problems candidates at once: point_ptr (n_problems + 1, ragged,
 * point_ptr[0] = 0), uv0 and uv1 (total x 2: points1, points2) -- exactly the match_ptr, uv0, uv1 that
 * sim3opt_match_batch_get_* return -- and focal / cx / cy of K.  SIM3OPT_ERR_ARG with nothing changed: n_problems < 1,
 * a problem with no point, a non-monotone point_ptr, a non-finite number, focal <= 0, a NULL array.  A problem with
 * fewer than min_points points is accepted and ends with status 1. */
int sim3opt_essential_batch_set_problems(sim3opt_essential_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                         const double* uv0, const double* uv1, double focal, double cx, double cy);
/* Each may be NULL.  tiles[2]: the points staged in LDS at most and the hypotheses of a chunk: the sizes at which
 * the kernel takes another path. */
int sim3opt_essential_batch_dims(const sim3opt_essential_batch* b, int32_t* n_problems, int32_t* total_points,
                                 int32_t tiles[2]);
/* Every problem, ONE kernel launch for the batch.  Returns the number of problems with status 0, or a negative
 * SIM3OPT_ERR_* (SIM3OPT_ERR_STATE: no problems set); one problem's failure is its status, never the batch's. */
int sim3opt_essential_batch_solve(sim3opt_essential_batch* b);
/* The getters return SIM3OPT_ERR_STATE before the first solve.  poses: n x 7 [qx qy qz qw tx ty tz] of Rc12c2 and
 * tc1inc2, |t| = 1 (status 1 and 2: the identity and zero). */
int sim3opt_essential_batch_get_poses(const sim3opt_essential_batch* b, double* poses);
/* essentials: n x 9 row-major, Frobenius norm 1 (status 1 and 2: zero) */
int sim3opt_essential_batch_get_essentials(const sim3opt_essential_batch* b, double* essentials);
/* mask (total, 1 = inlier of the best hypothesis that voted for the winning candidate) and / or n_inliers (n) */
int sim3opt_essential_batch_get_inliers(const sim3opt_essential_batch* b, uint8_t* mask, int32_t* n_inliers);
/* Per problem (n each, votes n x 4; each may be NULL): status (SIM3OPT_ESSENTIAL_*), the index of the best hypothesis
 * (-1: none), its inlier count and the sum of its inliers' e2, the winning candidate, its votes, all four vote counts. */
int sim3opt_essential_batch_get_summary(const sim3opt_essential_batch* b, int32_t* status, int32_t* best_hypothesis,
                                        int32_t* n_inliers_hypothesis, double* cost_hypothesis, int32_t* winner,
                                        int32_t* votes_winner, int32_t* votes);
/* Diagnostics.  Each leaves the results of the last solve as they were.
 * What the last solve computed for `problem`, H = options.iterations hypotheses: sample (H x 6 point indices),
 * n_solutions (real solutions with a finite E), valid, essential (H x 9; zero where not valid), count and cost of the
 * scoring (0 where not valid).  Each may be NULL.  SIM3OPT_ERR_STATE before the first solve. */
int sim3opt_essential_batch_debug_hypotheses(sim3opt_essential_batch* b, int32_t problem, int32_t* sample,
                                             int32_t* n_solutions, int32_t* valid, double* essential, int32_t* count,
                                             double* cost);
/* P (1..4096) supplied matrices per problem (essentials: n x P x 9, finite) through the scoring code of
 * k_essential_ransac: count and cost (n x P each, one may be NULL). */
int sim3opt_essential_batch_debug_score(sim3opt_essential_batch* b, int32_t P, const double* essentials,
                                        int32_t* count, double* cost);
/* The pose step of k_essential_ransac on a supplied matrix per problem (essentials: n x 9, finite) and a supplied
 * inlier set (mask: total): the four candidates (n x 4 x 7, in the order above), their votes (n x 4), the winner (n)
 * and the mask narrowed to its voters (total).  The outputs may be NULL. */
int sim3opt_essential_batch_debug_pose(sim3opt_essential_batch* b, const double* essentials, const uint8_t* mask,
                                       double* candidates, int32_t* votes, int32_t* winner, uint8_t* mask_out);

/* ---- batched homography MLESAC and decomposition: the loop detector's planar two-view pose, every candidate in one launch ----
 * HomographyInit::Compute(vMatches, 5.0, se3) (kittiDetector.h:1387-1443, the USE_KLEIN record line; HomographyInit.cc,
 * MEstimator.h): 300 MLESAC trials of a four-point homography, the inliers of the best one, five Tukey-reweighted
 * refinement rounds on them, the Faugeras-Lustman decomposition into eight (R, t, n, d), two visibility tests and a
 * Sampson tie-break.  It is the estimator that works where the five-point one degenerates: facades, the road surface,
 * revisits with little parallax.
 * PARITY UNPINNED: the reference cannot be built here (TooN and libCVD are absent) and its rand() sampling is not
 * reproducible.  What is the reference's: every step and formula below from the error on, in its order, with its
 * constants.  What is not: the sampler is counter-based; the linear algebra (TooN's SVD of the 8 x 9 system, its WLS, its
 * 3 x 3 SVD) is a closed form, a Cholesky factorisation and a Jacobi eigen-solver; equal scores are ordered by the
 * decomposition's number (std::sort leaves that open); the camera is the pinhole (the reference: ATANCamera); the
 * least-squares branch the call site reaches at exactly nine points is not here (status 1 below min_points = 10).
 * Definition.
 * Coordinates: v2CamPlane = ((u - cx) / f, (v - cy) / f) in double for both views, m2PixelProjectionJac = f I; view 0 is
 * uv0 (First); second ~ H first; the pose is se3SecondFromFirst: X1 = R X0 + t.
 * Sampler: draw j (0..3) of hypothesis h is splitmix64(seed + (4 h + j + 1) * 0x9E3779B97F4A7C15) modulo n - j, stepped
 * over the earlier picks in ascending order.
 * Hypothesis (:65-115): the homography of the four correspondences, H = B adj(A) with A (B) the map from the standard
 * projective basis to the four points of view 0 (1) -- the null vector of the reference's 8 x 9 system up to sign --
 * scaled to Frobenius norm 1.  Invalid (the identity stored, skipped): twice the area of a triangle of three of the four
 * points at most 1e-9 in either view (collinear or repeated points), a non-finite entry.
 * Error (:14-33): p = H (x0, y0, 1), e = f ((x1, y1) - (p0, p1) / p2), e2 = |e|^2 in px^2, every product and sum
 * rounded on its own, left to right (no fused multiply-add).  MLESAC: the cost of a hypothesis is the sum over all
 * points of min(e2, max_pixel_error^2) (a non-finite e2 costs the cap).  Best: the smallest cost, then the smallest index.
 * Inliers (:44-47): e2 < max_pixel_error^2 under the best H; the set is fixed from here on; fewer than 4: status 3.
 * Refinement (:120-177), refine_rounds times: the inliers' e and 2 x 9 Jacobians at H; sigma^2 = (4.6851 * 1.4826 *
 * (1 + 5 / (2 m - 6)) * sqrt(median))^2 with the median the element of rank floor(m / 2) (from 0) of the m squared
 * errors in ascending order, exactly; weights (1 - e2 / sigma^2)^2, 0 where e2 > sigma^2; (I + J^T W J) update =
 * J^T W e summed in a fixed order and solved by Cholesky; H += update.
 * Decomposition (:232-339): H = U diag(d1 >= d2 >= d3) V^T (V and d^2 from eight cyclic Jacobi sweeps on H^T H,
 * U = H V diag(1 / d); every column of V signed so that its component of largest magnitude, the first such, is
 * positive -- the reference leaves that to TooN's SVD, and with it which of the eight is which), s = det U det V.  Only d1 != d2 != d3 exactly (the reference's case 1); anything else, or a
 * non-finite number: status 4.  Decomposition k = 0..3 has d = s d2 and Eq. 13-14, k = 4..7 d = -s d2 and Eq. 15-16,
 * with the signs (e1, e3) = (+, +), (-, +), (+, -), (-, -) within each four; R = s U Rp V^T, t = U tp, n = V np.
 * Choice (:363-435): first count, per decomposition, of inliers with (H row 2 . (x0, y0, 1)) / d > 0; the four with
 * the largest counts stay (equal counts: the smaller k first); second count: ((x0, y0, 1) . n) / d > 0; two stay.
 * dRatio = score[1] / score[0] of the negated counts; dRatio < 0.9 takes the first; otherwise (0 / 0 included) the sums
 * over ALL points of Sampson's error of second^T [t]x R first, each capped at 4 max_pixel_error^2, decide with <=.
 * H and -H give the same pose: decomposition k of H is decomposition (k & 4) | (3 - (k & 3)) of -H.
 * Device pipeline: sim3opt_amd/csrc/homography_batch.hip, one workgroup per problem, one launch.  A problem's result
 * does not depend on the other problems of the batch or on its place among them.  No CPU fallback:
 * SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_homography_batch sim3opt_homography_batch;

typedef struct sim3opt_homography_batch_options {
  double max_pixel_error;  /* inlier: e2 < max_pixel_error^2 [px]; MLESAC's cap       default 5.0   :1414 dMaxPixelError        */
  uint64_t seed;           /* of the sampler                                           default 0                                 */
  int32_t iterations;      /* hypotheses per problem, 1..4096                          default 300   HomographyInit.cc:195       */
  int32_t refine_rounds;   /* Tukey-reweighted rounds on the inliers, 0..8             default 5     HomographyInit.cc:48        */
  int32_t min_points;      /* fewer points: status 1, nothing run; >= 4                default 10    HomographyInit.cc:182       */
  int32_t device;          /* HIP device ordinal, -1 = current                         default -1                                */
} sim3opt_homography_batch_options;

#define SIM3OPT_HOMOGRAPHY_OK 0            /* H, a pose and its inliers                                                     */
#define SIM3OPT_HOMOGRAPHY_FEW_POINTS 1    /* fewer than min_points points: nothing run, identity rotation, zero t, H = 0    */
#define SIM3OPT_HOMOGRAPHY_NO_HYPOTHESIS 2 /* no sample gave an H: likewise                                                 */
#define SIM3OPT_HOMOGRAPHY_NO_INLIERS 3    /* fewer than 4 inliers of the best H: identity pose, both H the MLESAC one       */
#define SIM3OPT_HOMOGRAPHY_DEGENERATE 4    /* not the decomposition's case 1, or a non-finite number: identity pose, H kept  */

void sim3opt_homography_batch_options_default(sim3opt_homography_batch_options* o);
sim3opt_homography_batch* sim3opt_homography_batch_create(void);
void sim3opt_homography_batch_destroy(sim3opt_homography_batch* b);
const char* sim3opt_homography_batch_last_error(const sim3opt_homography_batch* b);
/* SIM3OPT_ERR_ARG, nothing changed: iterations outside 1..4096, max_pixel_error <= 0 or not finite, refine_rounds
 * outside 0..8, min_points < 4. */
int sim3opt_homography_batch_set_options(sim3opt_homography_batch* b, const sim3opt_homography_batch_options* o);
/* vMatches of the call at :1414 (built at :1393-1409) for n_problems candidates at once: point_ptr (n_problems + 1,
 * ragged, point_ptr[0] = 0), uv0 and uv1 (total x 2) -- exactly the match_ptr, uv0, uv1 that
 * sim3opt_match_batch_get_* return -- and focal / cx / cy.  SIM3OPT_ERR_ARG with nothing changed: n_problems < 1, a
 * problem with no point, a non-monotone point_ptr, a non-finite number, focal <= 0, a NULL array.  A problem with fewer
 * than min_points points is accepted and ends with status 1. */
int sim3opt_homography_batch_set_problems(sim3opt_homography_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                          const double* uv0, const double* uv1, double focal, double cx, double cy);
/* Each may be NULL.  tiles[2]: the points staged in LDS at most and the hypotheses of a chunk: the sizes at which
 * the kernel takes another path. */
int sim3opt_homography_batch_dims(const sim3opt_homography_batch* b, int32_t* n_problems, int32_t* total_points,
                                  int32_t tiles[2]);
/* Compute (:35-63) of every problem, ONE kernel launch for the batch.  Returns the number of problems with status 0, or
 * a negative SIM3OPT_ERR_* (SIM3OPT_ERR_STATE: no problems set); one problem's failure is its status, never the batch's. */
int sim3opt_homography_batch_solve(sim3opt_homography_batch* b);
/* The getters return SIM3OPT_ERR_STATE before the first solve.  poses: n x 7 [qx qy qz qw tx ty tz] of
 * se3SecondFromFirst (:61), t as computed, not normalised (:1431 normalises it; status 1..4: the identity and zero). */
int sim3opt_homography_batch_get_poses(const sim3opt_homography_batch* b, double* poses);
/* n x 9 row-major each, one may be NULL: the best MLESAC hypothesis (:179-230, Frobenius norm 1) and mm3BestHomography
 * after the refinement rounds (:48-49) */
int sim3opt_homography_batch_get_homographies(const sim3opt_homography_batch* b, double* mlesac, double* refined);
/* mask (total, 1 = in mvHomographyInliers, :44-47) and / or n_inliers (n) */
int sim3opt_homography_batch_get_inliers(const sim3opt_homography_batch* b, uint8_t* mask, int32_t* n_inliers);
/* Per problem (each may be NULL): status (SIM3OPT_HOMOGRAPHY_*), the index of the best hypothesis (-1: none) and its
 * cost (dBestError, :224-228), the inlier count, sigma^2 of every round (n x 8, zero beyond refine_rounds; :161), the
 * first counts (n x 8; :366-378), the four decompositions kept (n x 4) and their second counts (n x 4; :383-395), the
 * chosen decomposition (0..7), whether the ambiguity branch ran (:404-433) and its two Sampson sums (n x 2, zero if
 * not). */
int sim3opt_homography_batch_get_summary(const sim3opt_homography_batch* b, int32_t* status, int32_t* best_hypothesis,
                                         double* cost_hypothesis, int32_t* n_inliers, double* sigma2,
                                         int32_t* counts_first, int32_t* kept, int32_t* counts_second,
                                         int32_t* choice, int32_t* ambiguous, double* sampson);
/* Diagnostics.  Each leaves the results of the last solve as they were.
 * What the last solve computed for `problem`, H = options.iterations hypotheses (:195-229): sample (H x 4 point
 * indices), n_solutions (1 where valid), valid, homography (H x 9; the identity where not valid), count (n where
 * valid) and cost of the scoring (0 where not valid).  Each may be NULL.  SIM3OPT_ERR_STATE before the first solve. */
int sim3opt_homography_batch_debug_hypotheses(sim3opt_homography_batch* b, int32_t problem, int32_t* sample,
                                              int32_t* n_solutions, int32_t* valid, double* homography,
                                              int32_t* count, double* cost);
/* P (1..4096) supplied matrices per problem (homographies: n x P x 9, finite) through the scoring code of
 * k_homography_ransac (MLESACScore, :23-33): count (= the problem's points) and cost (n x P each, one may be NULL). */
int sim3opt_homography_batch_debug_score(sim3opt_homography_batch* b, int32_t P, const double* homographies,
                                         int32_t* count, double* cost);
/* RefineHomographyWithInliers (:120-177), refine_rounds times, from a supplied matrix per problem (homographies:
 * n x 9, finite) on a supplied inlier set (mask: total): sigma^2 (n x refine_rounds) and H (n x refine_rounds x 9)
 * after every round; zero for a problem whose set has fewer than four points.  One output may be NULL. */
int sim3opt_homography_batch_debug_refine(sim3opt_homography_batch* b, const double* homographies,
                                          const uint8_t* mask, double* sigma2, double* refined);
/* DecomposeHomography and ChooseBestDecomposition (:232-435) of a supplied matrix per problem (homographies: n x 9,
 * finite) on a supplied inlier set (mask: total): the eight decompositions (n x 8 x 16: R row-major, t, n, d; zero with
 * status 4), status (0 or 4), and what sim3opt_homography_batch_get_summary returns of the choice, then the poses
 * (n x 7).  The outputs may be NULL. */
int sim3opt_homography_batch_debug_decompose(sim3opt_homography_batch* b, const double* homographies,
                                             const uint8_t* mask, double* decompositions, int32_t* status,
                                             int32_t* counts_first, int32_t* kept, int32_t* counts_second,
                                             int32_t* choice, int32_t* ambiguous, double* sampson, double* poses);

/* ---- batched Sim(3) RANSAC and refinement: a loop edge with its information, every candidate in one launch ----
 * What sim3opt_add_edge / sim3opt_gate_edges consume and nothing upstream produced: a Sim(3) measurement C with
 * X1 ~ s R X0 + t between the two frames of a candidate, each at its own map's scale, and Omega, the information of C.
 * PARITY UNPINNED: the reference has no such step.  Its scale is a ratio of median depths (kittiDetector.h:1305-1311;
 * sim3opt_median_depth_ratio), rotation and translation come from a rigid two-view BA, every loop edge carries
 * Identity(7) (kitti_surf.cpp:167, 202) and Constraint::fisher_information (kittiDetector.h:404-422) is never filled.
 * The method is Horn's closed form as ORB-SLAM's Sim3Solver / OptimizeSim3 use it.  Deviations from ORB-SLAM: the
 * sampler is counter-based; the rotation is the eigenvector of Horn's 4 x 4 matrix by ten cyclic Jacobi sweeps (there:
 * cv::eigen); errors are taken on the camera plane and scaled by f; the refinement is a Levenberg-Marquardt under this
 * library's damping rule on a fixed inlier set (there: five g2o iterations, outliers dropped, five more); exp has the
 * exact small-angle limit of its B coefficient (fix_small_angle_b = 1 of the pose-graph options); there is no early
 * termination of the hypotheses: all `iterations` are made and scored.
 * Definition.
 * Points: (x, y) = ((u - cx) / f, (v - cy) / f), X0 = depth0 (x0, y0, 1), X1 = depth1 (x1, y1, 1), in double, every
 * product and sum rounded on its own (no fused multiply-add).
 * Sampler: draw j (0..2) of hypothesis h is splitmix64(seed + (3 h + j + 1) * 0x9E3779B97F4A7C15) modulo n - j, stepped
 * over the earlier picks in ascending order.
 * Hypothesis: centred a_i = X0_i - mean, b_i = X1_i - mean; S = sum a_i b_i^T; the unit eigenvector (qw >= 0) of the
 * largest eigenvalue of Horn's N(S) is R; s = sum b_i . R a_i / sum |a_i|^2 (Horn's asymmetric form);
 * t = mean1 - s R mean0.  Invalid (the identity stored, not scored): |a x b|^2 <= min_triangle_sin2 |a|^2 |b|^2 for the
 * edges a, b at the sample's first point in either frame (collinear or repeated points); s not finite and positive; a
 * sample point with non-positive depth under C or C^-1.
 * Scoring: Y = s R X0 + t, Z = C^-1 X1; e1 = f^2 |Y.xy / Y.z - (x1, y1)|^2, e0 = f^2 |Z.xy / Z.z - (x0, y0)|^2; a match
 * is an inlier iff Y.z > 0, Z.z > 0, e1 <= max_pixel_error^2 and e0 <= max_pixel_error^2, and then costs e0 + e1.  Best:
 * the largest count, then the smallest cost, then the smallest index.
 * Refinement on the best hypothesis's inliers, fixed: C <- exp(delta) C with delta = [omega, upsilon, sigma] (g2o's
 * Sim(3) exp), four residuals a match, Huber of width huber_delta per 2-vector (0: none), analytic Jacobians, at most
 * refine_iters iterations of at most max_trials trials, lambda_0 = tau max diag; it also ends when a step promises less
 * than 1e-9 of chi2.  The sums are reduced in a fixed order: a thread's matches (t, t + 256, ...) ascending, a
 * butterfly over the wavefront, the four wavefronts in order.  Points are fixed (ORB-SLAM's choice): Omega is
 * optimistic -- the back-projected points carry the pixel noise (measured: about 3.5 times in d2 with exact depths)
 * and depth error is not seen; pixel_noise scales it.
 * Result: the mask re-derived under the refined C with the scoring rule, its count, RMS = sqrt(sum (e0 + e1) / (2 count)),
 * Omega = sum w J^T J / pixel_noise^2 over it (w: the Huber weights, J: the derivative by the same left perturbation):
 * with EdgeSim3's residual log(C S0 S1^-1) an estimate exp(eps) C* has the residual eps at the true vertices, so Omega
 * is the `info` of sim3opt_add_edge / sim3opt_gate_edges as it stands, with no adjoint.
 * Device pipeline: sim3opt_amd/csrc/sim3_batch.hip, one workgroup per problem, one launch.  A problem's result does not
 * depend on the other problems of the batch or on its place among them.  No CPU fallback: SIM3OPT_ERR_NO_DEVICE
 * without a GPU. */
typedef struct sim3opt_sim3_batch sim3opt_sim3_batch;

typedef struct sim3opt_sim3_batch_options {
  double max_pixel_error;   /* inlier: both errors <= max_pixel_error^2 [px]        default sqrt(9.210): chi^2_2 0.99, 1 px */
  double huber_delta;       /* Huber width per reprojection [px]; 0: no kernel      default sqrt(9.210)                    */
  double pixel_noise;       /* Omega is divided by its square [px]                   default 1                              */
  double min_triangle_sin2; /* a sample's triangle is degenerate at or below, [0, 1) default 1e-6                           */
  double tau;               /* lambda_0 = tau * max diag(J^T W J)                    default 1e-5                           */
  uint64_t seed;            /* of the sampler                                        default 0                              */
  int32_t iterations;       /* hypotheses per problem, 1..4096                       default 300                            */
  int32_t min_points;       /* fewer matches: status 1, nothing run; >= 3            default 9                              */
  int32_t min_inliers;      /* fewer final inliers: status 3                         default 10                             */
  int32_t refine_iters;     /* LM iterations at most; 0: none                        default 10                             */
  int32_t max_trials;       /* LM trials an iteration at most, >= 1                  default 5                              */
  int32_t device;           /* HIP device ordinal, -1 = current                      default -1                             */
} sim3opt_sim3_batch_options;

#define SIM3OPT_SIM3_OK 0               /* C, Omega and the inliers                                                     */
#define SIM3OPT_SIM3_FEW_POINTS 1       /* fewer than min_points matches: nothing run, C the identity, Omega zero        */
#define SIM3OPT_SIM3_NO_HYPOTHESIS 2    /* no sample gave a C: likewise                                                 */
#define SIM3OPT_SIM3_FEW_INLIERS 3      /* fewer than min_inliers final inliers; C and Omega as computed                */
#define SIM3OPT_SIM3_NOT_POSITIVE 4     /* Omega's Cholesky fails on the device; C and Omega as computed                */

void sim3opt_sim3_batch_options_default(sim3opt_sim3_batch_options* o);
sim3opt_sim3_batch* sim3opt_sim3_batch_create(void);
void sim3opt_sim3_batch_destroy(sim3opt_sim3_batch* b);
const char* sim3opt_sim3_batch_last_error(const sim3opt_sim3_batch* b);
/* SIM3OPT_ERR_ARG, nothing changed: iterations outside 1..4096; max_pixel_error, pixel_noise or tau <= 0 or not finite;
 * huber_delta < 0 or not finite; min_triangle_sin2 outside [0, 1); min_inliers < 0; min_points < 3; refine_iters < 0;
 * max_trials < 1. */
int sim3opt_sim3_batch_set_options(sim3opt_sim3_batch* b, const sim3opt_sim3_batch_options* o);
/* n_problems candidates at once: point_ptr (n_problems + 1, ragged, point_ptr[0] = 0), uv0 and uv1 (total x 2), depth0
 * and depth1 (total) -- exactly the match_ptr, uv0, uv1, depth0, depth1 that sim3opt_match_batch_get_* return -- and
 * focal / cx / cy.  SIM3OPT_ERR_ARG with nothing changed: n_problems < 1, a problem with no match, a non-monotone
 * point_ptr, a non-finite number, a depth <= 0, focal <= 0, a NULL array.  A problem with fewer than min_points matches
 * is accepted and ends with status 1. */
int sim3opt_sim3_batch_set_problems(sim3opt_sim3_batch* b, int32_t n_problems, const int32_t* point_ptr,
                                    const double* uv0, const double* uv1, const double* depth0, const double* depth1,
                                    double focal, double cx, double cy);
/* Each may be NULL.  tiles[2]: the matches staged in LDS at most and the hypotheses of a chunk: the sizes at which the
 * kernel takes another path. */
int sim3opt_sim3_batch_dims(const sim3opt_sim3_batch* b, int32_t* n_problems, int32_t* total_points, int32_t tiles[2]);
/* Every problem, ONE kernel launch for the batch.  Returns the number of problems with status 0, or a negative
 * SIM3OPT_ERR_* (SIM3OPT_ERR_STATE: no problems set); one problem's failure is its status, never the batch's. */
int sim3opt_sim3_batch_solve(sim3opt_sim3_batch* b);
/* The getters return SIM3OPT_ERR_STATE before the first solve.  sim3: n x 8 [qx qy qz qw tx ty tz s], the `meas` of
 * sim3opt_add_edge(v0 = frame 0, v1 = frame 1); information: n x 49, column-major, its `info`.  One may be NULL. */
int sim3opt_sim3_batch_get_sim3(const sim3opt_sim3_batch* b, double* sim3, double* information);
/* mask (total, 1 = final inlier) and / or n_inliers (n) */
int sim3opt_sim3_batch_get_inliers(const sim3opt_sim3_batch* b, uint8_t* mask, int32_t* n_inliers);
/* Per problem (each may be NULL): status (SIM3OPT_SIM3_*), the index of the best hypothesis (-1: none), its inlier
 * count and cost, the RMS pixel error of the final inliers, the LM iterations run, chi2 before and after them (n x 2). */
int sim3opt_sim3_batch_get_summary(const sim3opt_sim3_batch* b, int32_t* status, int32_t* best_hypothesis,
                                   int32_t* n_inliers_hypothesis, double* cost_hypothesis, double* rms_px,
                                   int32_t* refine_iterations, double* chi2);
/* Diagnostics.  Each leaves the results of the last solve as they were.
 * What the last solve computed for `problem`, H = options.iterations hypotheses: sample (H x 3 match indices),
 * n_solutions (1 where valid), valid, sim3 (H x 8; the identity where not valid), count and cost of the scoring (0 where
 * not valid).  Each may be NULL.  SIM3OPT_ERR_STATE before the first solve. */
int sim3opt_sim3_batch_debug_hypotheses(sim3opt_sim3_batch* b, int32_t problem, int32_t* sample, int32_t* n_solutions,
                                        int32_t* valid, double* sim3, int32_t* count, double* cost);
/* P (1..4096) supplied C per problem (sims: n x P x 8, finite, unit quaternions) through the scoring code of
 * k_sim3_ransac: count and cost (n x P each, one may be NULL). */
int sim3opt_sim3_batch_debug_score(sim3opt_sim3_batch* b, int32_t P, const double* sims, int32_t* count, double* cost);
/* The refinement from a supplied C per problem (sims: n x 8, finite, unit quaternion, s > 0) on a supplied inlier set
 * (mask: total): the refined C (n x 8), the iterations run (n), chi2 before and after (n x 2), the trials of every
 * iteration (n x refine_iters, zero beyond those run).  The outputs may be NULL. */
int sim3opt_sim3_batch_debug_refine(sim3opt_sim3_batch* b, const double* sims, const uint8_t* mask, double* sim_out,
                                    int32_t* iterations, double* chi2, int32_t* trials);
/* Omega (n x 49, column-major) and the Huber weights of every match (total x 2: the reprojection in image 1, in image
 * 0; zero outside the mask) at a supplied C on a supplied mask, with no LM; positive_definite (n): whether Omega's
 * Cholesky succeeds.  At least one output. */
int sim3opt_sim3_batch_debug_information(sim3opt_sim3_batch* b, const double* sims, const uint8_t* mask,
                                         double* information, double* weights, int32_t* positive_definite);

/* ---- batched descriptor matching and map-depth lookup: what the three blocks above consume, every candidate at once ----
 * The front of computeConstraints: matcher.match / knnMatch(.., 2) with the ratio test, the 1/10 image-border filter,
 * the skew filter and the uniqueness pass (kittiDetector.h:1085-1160), then the depth of every kept match in both
 * keyframes as the mean over the K = 6 map-point observations nearest in the image (cv::ml::KNearest, :1229-1279) and
 * surfPoints[0] = depth K^-1 (u, v, 1)^T.  match_ptr / points0 / uv1 are the point_ptr / points / uv1 of
 * sim3opt_pnp_batch_set_problems, uv0 / uv1 / points0 what sim3opt_ba_batch_set_problems takes, depth0 / depth1 what
 * sim3opt_median_depth_ratio takes.
 * PARITY UNPINNED: the reference stores neither descriptors nor matches, and its FlannBasedMatcher is an approximate
 * search over randomised trees.  Here the search is exact and deterministic.  The filters, their constants, the
 * uniqueness rule, K = 6 and the mean are the reference's.
 * Definition.  d2(i, j) = sum_k (a_ik - b_jk)^2 in FP32 (the difference form: near-duplicate descriptors do not
 * cancel), distance = sqrtf(d2).  The nearest train descriptor has the smallest d2, the lower index on equal d2; the
 * second nearest likewise among the rest.  ratio > 0 keeps a query iff n_train >= 2 and (d_1 == 0 && d_2 > 0) or
 * d_2 / d_1 > ratio (a float division of the two distances).  Border: both keypoints' x in [border_ratio w,
 * (1 - border_ratio) w] and y likewise with h; skew: |y1 - y0| < skew_y h and |x1 - x0| < skew_x w; all in double on
 * the float pixels.  Uniqueness: among kept queries with one train index the smallest d2 survives, the lower query
 * index on equal d2.  Survivors are listed by ascending query index.  Depth of a match on side c (side 0: the query
 * keypoint, frame0's observations): the min(K, n_obs) observations with the smallest FP32 squared pixel distance
 * fl(fl(dx dx) + fl(dy dy)), the lower index on equal distance; their obs_depth summed in double in that order, divided
 * by their number and rounded to float.  points0 = depth0 ((u - cx) / f, (v - cy) / f, 1) in double.
 * Device pipeline: sim3opt_amd/csrc/match_batch.hip; the launches of a solve do not depend on the number of pairs, and
 * a pair's result does not depend on the other pairs or its place among them.  No CPU fallback:
 * SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_match_batch sim3opt_match_batch;

typedef struct sim3opt_match_batch_options {
  double ratio;         /* ratio test of USE_KNN_MATCH, 0 = off (the reference's build)   default 0      :1097 thresh        */
  double border_ratio;  /* keypoints this share of the image from its edge or closer go   default 0.1    :1101 boundaryRatio */
  double skew_x;        /* |x1 - x0| < skew_x * image_width                               default 1/3    :1106 skewThreshX   */
  double skew_y;        /* |y1 - y0| < skew_y * image_height                              default 1/4    :1106 skewThreshY   */
  int32_t knn_k;        /* observations a depth is the mean of, 1..16                     default 6      :1238 K             */
  int32_t device;       /* HIP device ordinal, -1 = current                               default -1                         */
} sim3opt_match_batch_options;

#define SIM3OPT_MATCH_OK 0            /* matched (possibly with no match left)                                   */
#define SIM3OPT_MATCH_NO_KEYPOINTS 1  /* one of the two frames has no keypoint: no matches                        */
#define SIM3OPT_MATCH_NO_MAP 2        /* one of the two frames has no map-point observation: no matches           */

void sim3opt_match_batch_options_default(sim3opt_match_batch_options* o);
sim3opt_match_batch* sim3opt_match_batch_create(void);
void sim3opt_match_batch_destroy(sim3opt_match_batch* b);
const char* sim3opt_match_batch_last_error(const sim3opt_match_batch* b);
/* SIM3OPT_ERR_ARG, nothing changed: a negative or non-finite threshold, knn_k outside 1..16. */
int sim3opt_match_batch_set_options(sim3opt_match_batch* b, const sim3opt_match_batch_options* o);
/* n_frames ragged frames: frame f owns the keypoints kp_ptr[f]:kp_ptr[f+1] of kp (x 2, pixels) and desc (x 64) and the
 * observations obs_ptr[f]:obs_ptr[f+1] of obs_uv (x 2) and obs_depth (z of the map point in that camera's frame); a
 * frame may have none of either.  SIM3OPT_ERR_ARG with nothing changed: n_frames < 1, a NULL array, a pointer array
 * that does not start at 0 or decreases, a non-finite number, focal <= 0, a non-positive image size.  A successful call
 * drops the pairs and the results of the last solve. */
int sim3opt_match_batch_set_frames(sim3opt_match_batch* b, int32_t n_frames, const int32_t* kp_ptr,
                                   const int32_t* obs_ptr, const float* kp, const float* desc, const float* obs_uv,
                                   const float* obs_depth, double focal, double cx, double cy, int32_t image_width,
                                   int32_t image_height);
/* pairs: n_pairs x 2 (frame0 = the query side, frame1); a frame may be in any number of pairs, and in both places of
 * one.  SIM3OPT_ERR_STATE before set_frames; SIM3OPT_ERR_ARG with nothing changed: n_pairs < 1, NULL, a frame index
 * out of range.  A successful call drops the results of the last solve; the frames stay on the device. */
int sim3opt_match_batch_set_pairs(sim3opt_match_batch* b, int32_t n_pairs, const int32_t* pairs);
/* Each may be NULL.  tiles[4]: the lanes of a wavefront, the queries of a workgroup of k_match_nn, the train descriptors
 * and the observations staged in LDS at a time: the sizes at which the kernels take another path. */
int sim3opt_match_batch_dims(const sim3opt_match_batch* b, int32_t* n_frames, int32_t* n_pairs,
                             int32_t* total_keypoints, int32_t* total_observations, int32_t tiles[4]);
/* Every pair; the same launches whatever their number.  Returns the number of pairs with status 0, or a negative
 * SIM3OPT_ERR_* (SIM3OPT_ERR_STATE: no frames or no pairs set); one pair's failure is its status, never the batch's. */
int sim3opt_match_batch_solve(sim3opt_match_batch* b);
/* The getters return SIM3OPT_ERR_STATE before the first solve.  match_ptr: n_pairs + 1. */
int sim3opt_match_batch_get_match_ptr(const sim3opt_match_batch* b, int32_t* match_ptr);
/* Per match (total = match_ptr[n_pairs]), each may be NULL: query_idx and train_idx within their frames, distance,
 * uv0 and uv1 (x 2), depth0 and depth1, points0 (x 3). */
int sim3opt_match_batch_get_matches(const sim3opt_match_batch* b, int32_t* query_idx, int32_t* train_idx,
                                    float* distance, double* uv0, double* uv1, double* depth0, double* depth1,
                                    double* points0);
/* Per pair (n_pairs each, each may be NULL): status (SIM3OPT_MATCH_*) and the queries left after each stage: with a
 * nearest neighbour, after the ratio test, after border and skew, after uniqueness (= the pair's matches). */
int sim3opt_match_batch_get_summary(const sim3opt_match_batch* b, int32_t* status, int32_t* n_nearest,
                                    int32_t* n_after_ratio, int32_t* n_after_filters, int32_t* n_after_unique);
/* Diagnostics.  Each leaves the results of the last solve as they were.
 * What k_match_nn wrote for every query of `pair` in the last solve (n_query each, each may be NULL); second_idx = -1
 * and second_d2 = +inf with one train keypoint.  SIM3OPT_ERR_STATE before the first solve and for a pair whose status
 * is not 0 (nothing was computed for it). */
int sim3opt_match_batch_debug_nn(sim3opt_match_batch* b, int32_t pair, int32_t* best_idx, float* best_d2,
                                 int32_t* second_idx, float* second_d2);
/* n supplied pixels (uv: n x 2, finite) through the K-nearest code of k_match_depth on the observations of `frame`:
 * depth (n) and the chosen observations in (distance, index) order (neighbours: n x knn_k, -1 padded).  Needs frames
 * (SIM3OPT_ERR_STATE) with at least one observation in `frame` (SIM3OPT_ERR_ARG), no solve. */
int sim3opt_match_batch_debug_depth(sim3opt_match_batch* b, int32_t n, int32_t frame, const float* uv, double* depth,
                                    int32_t* neighbours);

/* ---- batched bag-of-words place recognition: the candidate pairs the blocks above start from, every keyframe at once ----
 * detector.detectLoop(keys, descriptors, result) (kittiDetector.h:1663): DLoopDetector over a DBoW2 SURF-64 vocabulary,
 * configured at :1549-1564.  It takes the kp_ptr / desc of sim3opt_match_batch_set_frames and returns the pairs of
 * sim3opt_match_batch_set_pairs.
 * PARITY UNPINNED: the reference tree holds neither DLoopDetector's nor DBoW2's source, no vocabulary, no descriptors
 * and no detection results.  Reference-held are FSurf64::distance (FSurf64.cpp:47-58), which d2 below follows exactly,
 * and the parameter values at the call site (use_nss, alpha, k, di_levels).  Everything else restates the published
 * algorithm (Galvez-Lopez and Tardos, T-RO 2012) and DLoopDetector's defaults from memory: [upstream recall]
 * dislocal 20, max_db_results 50, min_nss_factor 0.005, min_matches_per_group 1, max_intragroup_gap 3,
 * max_distance_between_groups 3, max_distance_between_queries 2, the order of the tests and of the status values, the
 * L1 normalisation and L1Scoring.  Each of them is an option, so a wrong recollection costs a default.
 * Definition.
 * Vocabulary: a tree as arrays.  Node 0 is the root (parent[0] = -1), 0 <= parent[i] < i otherwise; centre (n_nodes x
 * 64 floats); weight (n_nodes doubles, read at leaves only); word_id (-1 at inner nodes, a permutation of 0..n_words-1
 * at the leaves).  The children of a node are the nodes naming it as parent, in ascending index, at most 64.  The tree
 * may be unbalanced.  This is what DBoW2's save() writes (nodes: nodeId, parentId, weight, descriptor; words: wordId,
 * nodeId); parsing .yml.gz is the caller's.
 * Word of a descriptor: from the root, at every inner node go to the child of smallest d2, the lower child on equal d2,
 * until a leaf.  d2(a, b) = sum_k (double) fl32(fl32(a_k - b_k) * fl32(a_k - b_k)): difference and square in FP32,
 * each rounded once and not fused, the 64 terms added in double in ascending k.  The roundings are IEEE's: a square
 * below 2^-126 is a subnormal FP32 and is not flushed to zero, so two descriptors 2^-70 apart have d2 > 0.
 * Bag-of-words vector of a frame: for every word of weight > 0 that a descriptor of the frame reaches, value = count *
 * weight (one multiplication; DBoW2 adds the weight count times), or value = weight with options.accumulate = 0; the
 * values divided by their sum, taken in double in ascending word id: the sum is 0 plus the values one after the other,
 * not fused with the multiplication, and every value is divided by it once.  A frame without descriptors or without a
 * word of positive weight has the empty vector.
 * Score: s(a, b) = -1/2 sum_{w in a and b} (|a_w - b_w| - (|a_w| + |b_w|)) in double, the terms added one after the
 * other in ascending word id: a function of the two vectors alone and symmetric in them bit for bit; 0 without a
 * common word.  The term is associated as written, fabs(a_w - b_w) - (fabs(a_w) + fabs(b_w)): three roundings; the
 * terms are added to 0; the sum is multiplied once by -0.5; a sum of 0 gives +0.
 * Per query frame i (entry ids are frame indices):
 *  1. i <= dislocal: SIM3OPT_PLACE_CLOSE_MATCHES_ONLY.
 *  2. Results: the frames j <= i - dislocal with s(v_i, v_j) > 0, by score descending and lower j on equal score, the
 *     first max_db_results of them.  None: SIM3OPT_PLACE_NO_DB_RESULTS.
 *  3. ns = s(v_i, v_{i-1}) with use_nss, else 1.  With use_nss, ns < min_nss_factor: SIM3OPT_PLACE_LOW_NSS_FACTOR.
 *  4. Kept: the results with score >= alpha * ns.  None: SIM3OPT_PLACE_LOW_SCORES.  From here on match is reported.
 *  5. Islands: the kept results in ascending j; runs in which each j is less than max_intragroup_gap above the one
 *     before.  An island has first, last, score (its results' scores added one after the other in ascending j) and
 *     best_entry (its result of highest score, the lower j on ties); islands of fewer than min_matches_per_group
 *     results are dropped.
 *     None left: SIM3OPT_PLACE_NO_GROUPS with match = the best result.  The chosen island has the highest score, the
 *     lower first on ties; match = its best_entry.
 *  6. Temporal window, a recurrence over the queries that reached 5 with an island, state (a1, a2, last_query, n),
 *     n = 0 at the start: n = 1 if n == 0 or i - last_query > max_distance_between_queries; else n += 1 if [a1, a2]
 *     and [first, last] intersect or max(a1 - last, first - a2) <= max_distance_between_groups, else n = 1; then
 *     (a1, a2, last_query) = (first, last, i).  n > k: SIM3OPT_PLACE_CANDIDATE, else
 *     SIM3OPT_PLACE_NO_TEMPORAL_CONSISTENCY.
 * Not here: DLoopDetector's geometric check (GEOM_FLANN: a fundamental matrix by RANSAC, at least 12 inliers) is what
 * sim3opt_match_batch and sim3opt_essential_batch do with the pairs (the caller reads n_inliers), so there is no
 * NO_GEOMETRICAL_CONSISTENCY status; the direct index (di_levels) serves GEOM_DI only and is not built.
 * Device pipeline: sim3opt_amd/csrc/place_batch.hip; steps 1-5 run per query on the device, step 6 (an integer
 * recurrence of n_frames steps) on the host.  The launches of a solve do not depend on the number of frames; a pair's
 * score and a frame's outcome up to step 5 do not depend on the other frames or on their place in the batch.
 * No CPU fallback: SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_place_batch sim3opt_place_batch;

#define SIM3OPT_PLACE_MAX_FRAMES 16384 /* the scores of all pairs j <= i stay on the device: 8 n (n + 1) / 2 bytes, 1.0 GiB here */

typedef struct sim3opt_place_batch_options {
  double alpha;                         /* results below alpha * ns go                    default 0.3    :1549-1564         */
  double min_nss_factor;                /* queries with ns below it are not trusted       default 0.005  [upstream recall]  */
  int32_t use_nss;                      /* normalise by the score against frame i - 1     default 1      :1549-1564         */
  int32_t k;                            /* a candidate needs n > k consistent queries     default 3      :1549-1564         */
  int32_t dislocal;                     /* frames this close before the query are skipped default 20     [upstream recall]  */
  int32_t max_db_results;               /* results kept per query, 1..1024                default 50     [upstream recall]  */
  int32_t max_intragroup_gap;           /* j closer than this to the one before: same island  default 3  [upstream recall]  */
  int32_t min_matches_per_group;        /* results an island needs                        default 1      [upstream recall]  */
  int32_t max_distance_between_queries; /* a longer break restarts the temporal window    default 2      [upstream recall]  */
  int32_t max_distance_between_groups;  /* islands this far apart still fit the window    default 3      [upstream recall]  */
  int32_t accumulate;                   /* 1: value = count * weight (TF-IDF, TF); 0: value = weight (IDF, binary)  default 1 */
  int32_t device;                       /* HIP device ordinal, -1 = current               default -1                        */
} sim3opt_place_batch_options;

#define SIM3OPT_PLACE_CANDIDATE 0               /* a loop candidate: (query, match) is a pair                 */
#define SIM3OPT_PLACE_CLOSE_MATCHES_ONLY 1      /* i <= dislocal                                              */
#define SIM3OPT_PLACE_NO_DB_RESULTS 2           /* no earlier frame scores above 0                            */
#define SIM3OPT_PLACE_LOW_NSS_FACTOR 3          /* the score against the frame before is below min_nss_factor */
#define SIM3OPT_PLACE_LOW_SCORES 4              /* no result reaches alpha * ns                               */
#define SIM3OPT_PLACE_NO_GROUPS 5               /* no island of min_matches_per_group results                 */
#define SIM3OPT_PLACE_NO_TEMPORAL_CONSISTENCY 6 /* the window holds k queries or fewer                        */

void sim3opt_place_batch_options_default(sim3opt_place_batch_options* o);
sim3opt_place_batch* sim3opt_place_batch_create(void);
void sim3opt_place_batch_destroy(sim3opt_place_batch* b);
const char* sim3opt_place_batch_last_error(const sim3opt_place_batch* b);
/* SIM3OPT_ERR_ARG, nothing changed: alpha or min_nss_factor negative or not finite, use_nss or accumulate not 0 or 1,
 * k < 0, dislocal < 1, max_db_results outside 1..1024, max_intragroup_gap < 1, min_matches_per_group < 1, a negative
 * distance.  The frames, their words and vectors stay; the results of the last solve stay too (they are that solve's). */
int sim3opt_place_batch_set_options(sim3opt_place_batch* b, const sim3opt_place_batch_options* o);
/* The tree of the definition.  SIM3OPT_ERR_ARG with nothing changed: a NULL array, n_nodes < 2, a parent that is not
 * smaller than its child, a non-finite centre, a negative or non-finite weight at a leaf, a leaf without a word id, an
 * inner node with one, a word id repeated or not below the number of leaves, a node with more than 64 children.  A
 * successful call keeps the frames and drops the results of the last solve. */
int sim3opt_place_batch_set_vocabulary(sim3opt_place_batch* b, int32_t n_nodes, const int32_t* parent,
                                       const float* centre, const double* weight, const int32_t* word_id);
/* The matching stage's arrays as they are: frame f owns the descriptors kp_ptr[f]:kp_ptr[f+1] of desc (x 64); a frame
 * may have none.  SIM3OPT_ERR_ARG with nothing changed: n_frames < 1 or above SIM3OPT_PLACE_MAX_FRAMES, a NULL array,
 * a pointer array that does not start at 0 or decreases, a non-finite descriptor.  A successful call keeps the
 * vocabulary (on the device too) and drops the results of the last solve. */
int sim3opt_place_batch_set_frames(sim3opt_place_batch* b, int32_t n_frames, const int32_t* kp_ptr, const float* desc);
/* Each may be NULL.  depth: edges from the root to the deepest leaf.  tiles[6]: the lanes of a wavefront (the vector
 * entries k_place_score looks up at a time), the lanes of a workgroup (the descriptors of one of k_place_words, the
 * scan width of k_place_bow and k_place_select), the words k_place_bow stages at a time, the longest query vector
 * k_place_score keeps in LDS, the database frames of one of its workgroups, the nodes k_place_words stages in LDS:
 * the sizes at which the kernels take another path. */
int sim3opt_place_batch_dims(const sim3opt_place_batch* b, int32_t* n_nodes, int32_t* n_words, int32_t* depth,
                             int32_t* n_frames, int32_t* total_descriptors, int32_t tiles[6]);
/* Every frame; the same launches whatever their number.  Returns the number of candidates, or a negative SIM3OPT_ERR_*
 * (SIM3OPT_ERR_STATE: no vocabulary or no frames set); a frame's outcome is its status, never the batch's. */
int sim3opt_place_batch_solve(sim3opt_place_batch* b);
/* The getters return SIM3OPT_ERR_STATE before the first solve.  Per frame, each may be NULL: status (SIM3OPT_PLACE_*);
 * match (-1 before step 4) and its score (0 likewise); ns_factor (0 for the statuses of steps 1 and 2); n_consistent
 * (the n of step 6, 0 for a query that did not reach it); island (n x 2: first, last of the chosen island, -1 without). */
int sim3opt_place_batch_get_results(const sim3opt_place_batch* b, int32_t* status, int32_t* match, double* score,
                                    double* ns_factor, int32_t* n_consistent, int32_t* island);
/* The rows (query, match) of the candidates in ascending query: the pairs of sim3opt_match_batch_set_pairs, frame0 =
 * the query side.  n_pairs receives their number whatever the capacity (rows); SIM3OPT_ERR_ARG when they do not fit
 * (pairs may be NULL with capacity 0: the number alone). */
int sim3opt_place_batch_get_pairs(const sim3opt_place_batch* b, int32_t capacity, int32_t* n_pairs, int32_t* pairs);
/* The ragged vectors: bow_ptr (n_frames + 1), word and value (bow_ptr[n_frames] each, by ascending word id within a
 * frame).  Each may be NULL: call with bow_ptr alone for the sizes. */
int sim3opt_place_batch_get_bow(const sim3opt_place_batch* b, int32_t* bow_ptr, int32_t* word, double* value);
/* Diagnostics.  Each leaves the results of the last solve as they were.
 * n supplied descriptors (n x 64, finite) through the descent code of k_place_words: word (n) and the winning d2 of
 * every level (path_d2: n x depth, -1 past the leaf).  At least one output.  Needs a vocabulary (SIM3OPT_ERR_STATE). */
int sim3opt_place_batch_debug_words(sim3opt_place_batch* b, int32_t n, const float* desc, int32_t* word,
                                    double* path_d2);
/* The full score row s(v_query, v_j) for every j of the last solve (row: n_frames), without the j <= i - dislocal cut.
 * SIM3OPT_ERR_STATE before the first solve. */
int sim3opt_place_batch_debug_scores(sim3opt_place_batch* b, int32_t query, double* row);
/* Steps 2-5 of one query of the last solve again: the kept results in ascending j (n_kept; kept_j and kept_score with
 * room for max_db_results) and the islands left after min_matches_per_group in ascending first (n_islands; island:
 * x 4 = first, last, best_entry, number of results; island_score), room for the max_db_results of that solve each
 * (1024 always suffices).  Each may be NULL. */
int sim3opt_place_batch_debug_islands(sim3opt_place_batch* b, int32_t query, int32_t* n_kept, int32_t* kept_j,
                                      double* kept_score, int32_t* n_islands, int32_t* island, double* island_score);

/* ---- batched vocabulary training: the tree place recognition descends, from the sequence's own descriptors ----
 * DBoW2's TemplatedVocabulary::create over FSurf64 (the Surf64Vocabulary typedef at kitti_surf.cpp:1231): hierarchical
 * k-means, k-means++ seeded.  It takes the kp_ptr / desc of sim3opt_place_batch_set_frames (the frames are the training
 * images) and returns the four arrays sim3opt_place_batch_set_vocabulary takes, with no conversion.
 * PARITY UNPINNED: the reference tree holds neither DBoW2's source nor a vocabulary file.  Reference-held are
 * FSurf64::distance and FSurf64::meanValue (FSurf64.cpp:23-58), the two functions create is parameterised by.
 * Everything else about create is recalled from upstream, marked [upstream recall] below, and an option where it is a
 * number, so a wrong recollection costs a default.
 * Definition.
 * Distance: the d2 of place recognition, word for word: d2(a, b) = sum_k (double) fl32(fl32(a_k - b_k) * fl32(a_k -
 * b_k)), difference and square in FP32, each rounded once and not fused, the 64 terms added in double in ascending k.
 * Split of a node with members m_0 < m_1 < ... (ascending descriptor index), n of them, at a level < levels:
 *  - n <= k: every member is a child of its own, the centre being the member, in member order.  [upstream recall]
 *  - otherwise k-means++ seeding [upstream recall]: centre 0 is member splitmix64(key(0)) % n.  For c = 1..k-1: w_i is
 *    the smallest d2 of member i to the centres so far and W = sum w_i; W = 0 ends the seeding with c centres;
 *    otherwise r = u W with u = (splitmix64(key(c)) >> 11) 2^-53, and the new centre is the first member, in member
 *    order, whose inclusive prefix sum of w exceeds r (the last member if none does).  key(c) = seed + (64 node + c + 1)
 *    * 0x9E3779B97F4A7C15 with node the node's output index: it holds the seed, the node and c only.  The prefix sums
 *    are double, formed in an order that is a function of the inputs alone (a scan within 256 members, the runs of 256
 *    one after the other).  To the bit: the members are cut into runs of 256 in member order.  A run's scan starts
 *    from its w followed by zeros up to 256 entries (a partial run is padded, not shortened); then for s = 1, 2, 4, ...,
 *    128 every entry i >= s becomes itself plus entry i - s, all from the values before the step.  A run's total is
 *    the scan's entry 255 -- in a partial run another association of the same terms than its last member's entry, so
 *    the two may differ in the last bit.  carry = 0 before the first run and carry + total after each; a member's
 *    prefix is its scan entry plus the carry before its run; W is the carry after the last run, and r = u W is one
 *    multiplication.  W may therefore round above the last member's prefix; r < W then leaves no prefix above r, and
 *    the choice falls to the last member.
 *  - Lloyd: a pass assigns every member to the centre of smallest d2, the lower cluster on equal d2, and then sets the
 *    centre of every non-empty cluster to its mean; an empty cluster keeps its centre.  Passes repeat until one
 *    changes no assignment (its means are not taken again: they are the pass before's) or max_iters passes have run;
 *    a node stopped by max_iters counts in n_unconverged.
 *  - Mean: the members' coordinates added in double, divided once by the count, rounded once to FP32.  A STATED
 *    DEVIATION from FSurf64::meanValue, which adds FP32 quotients one after the other in member order: that order is
 *    serial over up to a million members; the double sum differs from it by its FP32 rounding only.  The order of the
 *    double sum: runs of 1024 members in member order, each added one member after the other, then the runs one after
 *    the other.  The runs are the node's (1024 of its members, whatever their clusters); a cluster's sum within a run
 *    is 0 plus its members there in member order, and its sum is 0 plus the runs' sums in run order.  (The addends are
 *    FP32, so on unit-norm descriptors this sum is exact and its order invisible in the centres.)  No floating-point
 *    atomics.
 *  - Children: the non-empty clusters, in cluster order.
 *  - Leaves: a node whose seeding ended with one centre (all members equal), a node of one member, every node at level
 *    `levels`.
 * Numbering: breadth first.  The root is 0, then levels 1, 2, ..., within a level by parent, then cluster; so
 * 0 <= parent[i] < i.  word_id counts the leaves in ascending node index and is -1 at inner nodes.  The root's centre
 * is all zeros.
 * Weights: N = the frames with at least one descriptor; N_i = the frames with a descriptor whose word by the descent
 * rule of place recognition on the finished tree is leaf i (DBoW2's transform [upstream recall]); weight = log(N / N_i)
 * in double on the host, 0 for a leaf no descent reaches; with idf = 0 every leaf has weight 1.  The TF part is
 * sim3opt_place_batch_options.accumulate.
 * Device pipeline: sim3opt_amd/csrc/vocab_train.hip, level-synchronous; the launches of a seeding round and of a Lloyd
 * pass do not depend on the number of nodes or descriptors.  No CPU fallback: SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_vocabulary sim3opt_vocabulary;

typedef struct sim3opt_vocabulary_options {
  uint64_t seed;     /* of the seeding's draws                                         default 0                      */
  int32_t k;         /* branching, 2..64                                               default 10  [upstream recall]  */
  int32_t levels;    /* L, 1..8 (8: with k = 10 more nodes than an int32 index x 64)   default 5   [upstream recall]  */
  int32_t max_iters; /* Lloyd passes per node, >= 1 (ours: DBoW2 has no cap)           default 100                    */
  int32_t idf;       /* 1: weight = log(N / N_i); 0: weight = 1                        default 1   [upstream recall]  */
  int32_t device;    /* HIP device ordinal, -1 = current                               default -1                     */
} sim3opt_vocabulary_options;

void sim3opt_vocabulary_options_default(sim3opt_vocabulary_options* o);
sim3opt_vocabulary* sim3opt_vocabulary_create(void);
void sim3opt_vocabulary_destroy(sim3opt_vocabulary* b);
const char* sim3opt_vocabulary_last_error(const sim3opt_vocabulary* b);
/* SIM3OPT_ERR_ARG, nothing changed: k outside 2..64, levels outside 1..8, max_iters < 1, idf not 0 or 1.  The frames
 * and the last training's results stay (they are that training's). */
int sim3opt_vocabulary_set_options(sim3opt_vocabulary* b, const sim3opt_vocabulary_options* o);
/* The arrays of sim3opt_place_batch_set_frames as they are; a frame may own no descriptor.  SIM3OPT_ERR_ARG with
 * nothing changed: that call's refusals, and fewer than two distinct descriptors in total (the tree needs two nodes).
 * A successful call drops the results of the last training. */
int sim3opt_vocabulary_set_frames(sim3opt_vocabulary* b, int32_t n_frames, const int32_t* kp_ptr, const float* desc);
/* Returns the number of nodes, or a negative SIM3OPT_ERR_* (SIM3OPT_ERR_STATE: no frames set; SIM3OPT_ERR_ARG: the
 * tree would hold more than INT32_MAX / 64 nodes). */
int sim3opt_vocabulary_train(sim3opt_vocabulary* b);
/* Each may be NULL; the first four are 0 before the first training.  depth: edges from the root to the deepest leaf.
 * passes[8]: the Lloyd passes run at each level (the most of any of its nodes, the pass that changed nothing
 * included; 0 where no node ran k-means).  tiles[2]: the members of a node one workgroup takes (a lane each) and the
 * members whose coordinates one wavefront adds one after the other: the sizes at which the kernels take another path. */
int sim3opt_vocabulary_dims(const sim3opt_vocabulary* b, int32_t* n_nodes, int32_t* n_words, int32_t* depth,
                            int32_t* n_unconverged, int32_t* n_frames, int32_t* total_descriptors, int32_t passes[8],
                            int32_t tiles[2]);
/* The getters return SIM3OPT_ERR_STATE before the first training.  Per node, each may be NULL: what
 * sim3opt_place_batch_set_vocabulary takes (centre x 64). */
int sim3opt_vocabulary_get_vocabulary(const sim3opt_vocabulary* b, int32_t* parent, float* centre, double* weight,
                                      int32_t* word_id);
/* Per training descriptor, each may be NULL: the leaf node it ended in by clustering, and the leaf node the descent
 * rule reaches on the finished tree (what the weights were counted from).  The two agree on a converged tree without
 * equal centres under one parent. */
int sim3opt_vocabulary_get_assignment(const sim3opt_vocabulary* b, int32_t* node_of_descriptor, int32_t* descent_node);
/* Read-outs of the last training for tests; they change nothing of its results.
 * The seeding of output node `node`: the chosen members as descriptor indices (n_chosen; member with room for k), and
 * W and r of every round run (n_rounds; room for k - 1 each; a round that ended the seeding has W = r = 0).  A node
 * that was not seeded (a leaf by its size or level, n <= k) has n_chosen = n_rounds = 0.  Each may be NULL. */
int sim3opt_vocabulary_debug_seeding(sim3opt_vocabulary* b, int32_t node, int32_t* n_chosen, int32_t* member,
                                     int32_t* n_rounds, double* W, double* r);
/* The state after `pass` passes (0..passes[level]) of `level`, run again from the stored start of the level: cluster
 * (per training descriptor: its cluster in its node; its rank in a node of n <= k; -1 where the descriptor's node at
 * that level is a leaf or the descriptor ended above) and centre (n_level_nodes x k x 64: the centres of every node of
 * the level, zero where there is none).  first_node: the output index of the level's first node.  Call with cluster and
 * centre NULL for the sizes.  Needs the device blocks of the last training (SIM3OPT_ERR_STATE after set_frames or a
 * change of the device). */
int sim3opt_vocabulary_debug_lloyd(sim3opt_vocabulary* b, int32_t level, int32_t pass, int32_t* first_node,
                                   int32_t* n_level_nodes, int32_t* cluster, float* centre);
/* Host only.  The file is this library's: "SIM3VOC\0", then int32 version (1), n_nodes, 64, then parent, centre, weight
 * and word_id as they are, little endian.  SIM3OPT_ERR_IO: the file cannot be written / read, or is truncated, of
 * another magic, version or length.  load hands out four blocks for sim3opt_vocabulary_free. */
int sim3opt_vocabulary_save(const char* path, int32_t n_nodes, const int32_t* parent, const float* centre,
                            const double* weight, const int32_t* word_id);
int sim3opt_vocabulary_load(const char* path, int32_t* n_nodes, int32_t** parent, float** centre, double** weight,
                            int32_t** word_id);
void sim3opt_vocabulary_free(void* block);

/* ---- batched SURF-64 extraction: keypoints and descriptors from the images, the head of the chain ----
 * SurfExtractor::operator() (kitti_surf.cpp:501-523): cv::xfeatures2d::SURF::create(400), detect + compute, a 64-float
 * descriptor per keypoint, once per keyframe.  Grey images in; kp_ptr, kp and desc out, in exactly the layout
 * sim3opt_match_batch_set_frames, sim3opt_place_batch_set_frames and sim3opt_vocabulary_set_frames take.
 * PARITY UNPINNED: OpenCV is not part of the reference tree, which holds no image, keypoint or descriptor either.
 * Reference-held is the call site: minHessian = 400, every other parameter at SURF's default, descriptorSize() == 64,
 * FSurf64 consuming 64 floats.  Everything about the algorithm is recalled from upstream's surf.cpp, marked [upstream
 * recall] below, and an option where it is a number, so a wrong recollection costs a default.
 * Definition.  The definition is the specification: the device is held to it bit for bit, and it to planted truth.
 * Arithmetic: the integral image is int32 and exact (set_images refuses 255 w h >= 2^31).  Every floating-point step
 *   below is FP32, rounded once per operation and never fused, in the order written (a + b + c is (a + b) + c);
 *   "rint" rounds a half to even; no libm function whose last bit may differ between host and device is used: the
 *   Gaussian tables are made once on the host in double and rounded once to FP32, the angle is the polynomial below,
 *   sin and cos are the polynomials below, sqrt is correctly rounded.
 * Integral image: S is (h + 1) x (w + 1) with a zero first row and column; S[y + 1][x + 1] = sum of the pixels [0..y] x
 *   [0..x].  A box {x1, y1, x2, y2} anchored at (y, x) sums to S[y+y1][x+x1] + S[y+y2][x+x2] - S[y+y2][x+x1] - S[y+y1][x+x2].
 * Layers: octave o of n_octaves has layers l = 0 .. n_octave_layers + 1; filter size (9 + 6 l) << o, step = 1 << o; the
 *   response plane has (h / step) x (w / step) entries (upstream's (rows - 1) / step is taken on the integral image's
 *   rows, which are h + 1: that reading is kept).  [upstream recall]
 * Response: the size-9 patterns {x1, y1, x2, y2, weight} are Dxx {0,2,3,7,+1} {3,2,6,7,-2} {6,2,9,7,+1}, Dyy their
 *   transpose, Dxy {1,1,4,4,+1} {5,1,8,4,-1} {1,5,4,8,-1} {5,5,8,8,+1}.  Resized to `size`: every corner coordinate c
 *   becomes rint(fl(size / 9) * c), the weight fl(weight / fl(fl(x2 - x1) * fl(y2 - y1))).  A response is 0 + (float)
 *   box_0 * w_0 + (float) box_1 * w_1 + ... in pattern order.  det = fl(dx * dy) - fl(fl(0.81 * dxy) * dxy), trace = dx +
 *   dy, stored at (i + margin, j + margin) with margin = (size / 2) / step for sample (i, j) anchored at (i step, j
 *   step), i < 1 + (h - size) / step, j < 1 + (w - size) / step; every other entry of the plane is 0 (ours: upstream
 *   leaves them unwritten), and a layer whose size exceeds h or w has no samples.
 * Extrema: middle layers l = 1 .. n_octave_layers; positions margin' <= i < h / step - margin' (j likewise) with
 *   margin' = (size_{l+1} / 2) / step + 1.  A candidate has det > (float) hessian_threshold and det strictly greater
 *   than all 26 neighbours in the three layers.  Centre = step (i - (size / 2) / step) + (size - 1) 0.5 in both axes
 *   (x from j), size = size_l, response = det, laplacian = the sign of trace (-1, 0, 1), octave = o.
 * Interpolation: with N(dl, di, dj) the 27 values, b = -((N(0,0,1) - N(0,0,-1)) / 2, (N(0,1,0) - N(0,-1,0)) / 2,
 *   (N(1,0,0) - N(-1,0,0)) / 2); A is symmetric with diagonal (N(0,0,-1) - 2 N(0,0,0)) + N(0,0,1) (and the same in i and
 *   in l) and off-diagonals (((N(+,+) - N(+,-)) - N(-,+)) + N(-,-)) / 4 over the pair of axes, the layer axis first in
 *   the signs' order for the two layer terms (xs: N(1,0,1) - N(1,0,-1) - N(-1,0,1) + N(-1,0,-1)).  A x = b by Gaussian
 *   elimination with partial pivoting (the first row of largest |entry| in the column), back-substitution x2, x1, x0;
 *   a zero pivot means no solution.  Kept iff a solution exists, x != 0 and every |x_k| <= 1; then pt += (x0, x1)
 *   step and size = rint(size + x2 (size_l - size_{l-1})).  [upstream recall]
 * Order and cap: within an image the kept candidates are ordered by response descending, ties by scan index
 *   ascending (octave, layer, row, column).  A STATED NARROWING of upstream's KeypointGreater, whose further keys can
 *   only differ on equal responses.  max_keypoints > 0 keeps the first that many (ours).  No atomic decides the order.
 * Orientation (upright = 1 skips it: angle = 270 [upstream recall]): s = size 1.2 / 9, g = 2 rint(2 s).  The 113 grid
 *   points (i, j), i^2 + j^2 <= 36, i outer and j inner, weigh G13[i + 6] G13[j + 6] (13 taps of sigma 2.5, scaled to
 *   sum 1).  Sample k sits at x = rint((pt.x + i s) - (g - 1) / 2), y = rint((pt.y + j s) - (g - 1) / 2) and counts
 *   when 0 <= x < w + 1 - g and 0 <= y < h + 1 - g; its vx, vy are the Haar responses {0,0,2,4,-1} {2,0,4,4,+1} and
 *   {0,0,4,2,+1} {0,2,4,4,-1}, resized from 4 to g, times the weight.  A keypoint with no such sample (so also one
 *   whose g exceeds the integral image) is dropped.  The angle function atan2deg(y, x), degrees in [0, 360]: with
 *   ax = |x|, ay = |y|, c = min / (max + (float) DBL_EPSILON) and P(c) = (((p7 c^2 + p5) c^2 + p3) c^2 + p1) c, where p1,
 *   p3, p5, p7 = 0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128 each times (float)
 *   (180 / pi): a = P(c) if ax >= ay else 90 - P(c); x < 0: a = 180 - a; y < 0: a = 360 - a.  [upstream recall; the
 *   coefficients are the definition either way, they make the function plain arithmetic.]  For each window centre c =
 *   0, 5, ..., 355 the sums of vx and of vy run over the samples with d = |rint(angle) - c|, d < 30 or d > 330, in
 *   sample order; the first window of largest sumx^2 + sumy^2 (strictly greater than 0 to start with) gives angle =
 *   atan2deg(-sumy, sumx): upstream's sign convention, fastAtan2(-besty, bestx).  [upstream recall]
 * Descriptor: win = (int)(21 s); a keypoint with win < 1 is dropped (ours).  (sin, cos) of the angle: q = (int)(angle /
 *   90) and r = (angle - 90 q) pi / 180 in double, sin r and cos r by their Taylor polynomials to r^19 and r^18 in nested
 *   form in double, turned by the quadrant, rounded once to FP32 (ours: upstream calls libm).  With sin_dir = -sin,
 *   cos_dir = cos and off = -(win - 1) / 2, window sample (row i, column j) is at px = (pt.x + (j + off) cos_dir) + (i
 *   + off) sin_dir, py = (pt.y - (j + off) sin_dir) + (i + off) cos_dir (ours: in closed form, where upstream adds
 *   increments one after the other).  Where 0 <= floor(px) < w - 1 and 0 <= floor(py) < h - 1 its value is rint of
 *   ((p00 (1-a)) (1-b) + (p01 a) (1-b)) + (p10 (1-a)) b + (p11 a) b with a, b the fractions; elsewhere the pixel at (rint
 *   px, rint py) clamped into the image.  The 21 x 21 patch: cell (u, v) covers [u win/21, (u+1) win/21) in each axis
 *   (scale = fl(win / 21), bounds fl(u scale)); a sample i weighs fl(min(upper, i + 1) - max(lower, i)) where positive;
 *   the cell is the sum of (wy wx) sample, row-major, over fl(scale scale), rint, clamped to 0..255 [upstream recall:
 *   area resize into an 8-bit patch].  On the 20 x 20 interior vx = (((p01 - p00) + p11) - p10) dw and vy = (((p10 -
 *   p00) + p11) - p01) dw with dw = G20[row] G20[column] (20 taps of sigma 3.3).  Sub-region r = 4 i + j of 5 x 5 gives
 *   sum vx, sum vy, sum |vx|, sum |vy|, its samples row-major: 64 floats in sub-region order, each times 1 / (sqrt(sum of
 *   the 64 squares in ascending index) + FLT_EPSILON).  Only the 64-float form exists: `extended` is not an option.
 * An image's result is a function of the image and the options alone: not of the other images, its place among them
 * or images_per_pass.  One image size per batch.
 * Device pipeline: sim3opt_amd/csrc/surf_batch.hip; the launches of a pass do not depend on the number of images in
 * it; the response planes never leave LDS.  No CPU fallback: SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_surf_batch sim3opt_surf_batch;

typedef struct sim3opt_surf_batch_options {
  double hessian_threshold; /* minHessian, >= 0 and finite                              default 400 (the call site)  */
  int32_t n_octaves;        /* 1..6                                                     default 4  [upstream recall] */
  int32_t n_octave_layers;  /* 1..6                                                     default 3  [upstream recall] */
  int32_t upright;          /* 1: no orientation step, angle = 270                      default 0                    */
  int32_t max_keypoints;    /* > 0: the strongest that many per image; 0: no cap        default 0                    */
  int32_t images_per_pass;  /* >= 1: bounds the device memory of a pass                 default 64                   */
  int32_t device;           /* HIP device ordinal, -1 = current                         default -1                   */
} sim3opt_surf_batch_options;

#define SIM3OPT_SURF_OK 0            /* the image has keypoints */
#define SIM3OPT_SURF_NO_KEYPOINTS 1  /* none: no layer fits, nothing above the threshold, or every one dropped */

void sim3opt_surf_batch_options_default(sim3opt_surf_batch_options* o);
sim3opt_surf_batch* sim3opt_surf_batch_create(void);
void sim3opt_surf_batch_destroy(sim3opt_surf_batch* b);
const char* sim3opt_surf_batch_last_error(const sim3opt_surf_batch* b);
/* SIM3OPT_ERR_ARG, nothing changed: hessian_threshold negative or not finite, n_octaves or n_octave_layers outside
 * 1..6, upright not 0 or 1, max_keypoints < 0, images_per_pass < 1. */
int sim3opt_surf_batch_set_options(sim3opt_surf_batch* b, const sim3opt_surf_batch_options* o);
/* n_images grey images of one size, row-major, row_stride bytes from row to row and height rows from image to image;
 * copied.  SIM3OPT_ERR_ARG with nothing changed: n_images < 1, pixels NULL, width or height < 1, row_stride < width,
 * 255 width height >= 2^31.  A successful call drops the results of the last solve. */
int sim3opt_surf_batch_set_images(sim3opt_surf_batch* b, int32_t n_images, int32_t width, int32_t height, int32_t row_stride,
                                  const uint8_t* pixels);
/* Each may be NULL.  total_keypoints is 0 before the first solve.  tiles[3]: the side of the detection tile, the keys
 * the ranking stages at a time, the lanes per keypoint: the sizes at which a kernel takes another path. */
int sim3opt_surf_batch_dims(const sim3opt_surf_batch* b, int32_t* n_images, int32_t* width, int32_t* height,
                            int32_t* total_keypoints, int32_t tiles[3]);
/* Returns the number of images with status SIM3OPT_SURF_OK, or a negative SIM3OPT_ERR_* (SIM3OPT_ERR_STATE: no images
 * set; SIM3OPT_ERR_ARG: a pass of images_per_pass images could hold more candidates than an int32 offset counts, at
 * most one per 2 x 2 block of every middle layer -- at the defaults 256 images of 4096 x 2056 could, 128 cannot; lower
 * images_per_pass); an
 * image's outcome is its status, never the batch's. */
int sim3opt_surf_batch_solve(sim3opt_surf_batch* b);
/* The getters return SIM3OPT_ERR_STATE before the first solve.  kp_ptr: n_images + 1. */
int sim3opt_surf_batch_get_kp_ptr(const sim3opt_surf_batch* b, int32_t* kp_ptr);
/* Per keypoint, each may be NULL: kp (x, y), desc (x 64), size, angle (degrees), response, octave, laplacian. */
int sim3opt_surf_batch_get_keypoints(const sim3opt_surf_batch* b, float* kp, float* desc, float* size, float* angle,
                                     float* response, int32_t* octave, int32_t* laplacian);
/* Per image, each may be NULL: status (SIM3OPT_SURF_*), the candidates before the interpolation and after it, and the
 * keypoints dropped at the orientation step.  n_interpolated counts before max_keypoints is applied, so with a cap the
 * image's keypoints are min(n_interpolated, max_keypoints) - n_dropped.  The drop rule is upstream's and is kept as the
 * definition, but no image reaches it: a layer yields candidates only where the next layer's filter fits with a margin,
 * which puts the keypoint at least size / 2 inside the image while g is about 0.53 size, so its central orientation
 * sample always counts, and win >= 8.  n_dropped is therefore 0 for every image; the path is exercised on the host
 * alone (tests/cxx/surf_host_driver.cpp calls the description with a size no layer has). */
int sim3opt_surf_batch_get_summary(const sim3opt_surf_batch* b, int32_t* status, int32_t* n_candidates,
                                   int32_t* n_interpolated, int32_t* n_dropped);
/* Read-outs for tests.  Each takes its image through a pass of its own with the options of the last solve, leaves that
 * solve's results untouched and hands back every block it takes.  SIM3OPT_ERR_STATE before the first solve.
 * S: (height + 1) x (width + 1). */
int sim3opt_surf_batch_debug_integral(sim3opt_surf_batch* b, int32_t image, int32_t* S);
/* The detection kernel's LDS values of layer `layer` (0 .. n_octave_layers + 1) of `octave`, written out by the DUMP
 * instantiation, whose other stores are the counting one's; trace is computed beside them.  rows x cols = (height >>
 * octave) x (width >> octave) each; call with det and trace NULL for the sizes. */
int sim3opt_surf_batch_debug_responses(sim3opt_surf_batch* b, int32_t image, int32_t octave, int32_t layer, int32_t* rows,
                                       int32_t* cols, float* det, float* trace);
/* The candidates of an image in scan order: layer (octave * 8 + layer), pos0 (x 3: x, y, size before the
 * interpolation), response, kept, pos1 (x 3: after it; pos0 where not kept).  Room for the image's n_candidates of
 * sim3opt_surf_batch_get_summary each; each may be NULL. */
int sim3opt_surf_batch_debug_candidates(sim3opt_surf_batch* b, int32_t image, int32_t* n_candidates, int32_t* layer,
                                        float* pos0, float* response, uint8_t* kept, float* pos1);
/* Of keypoint `keypoint` (an index into the last solve's outputs): per orientation sample (113 each) whether it
 * counts, vx, vy and its angle; the 72 window magnitudes.  Each may be NULL. */
int sim3opt_surf_batch_debug_orientation(sim3opt_surf_batch* b, int32_t keypoint, int32_t* valid, float* vx, float* vy,
                                         float* angle, float* window);
/* ... and its 21 x 21 patch, row-major. */
int sim3opt_surf_batch_debug_patch(sim3opt_surf_batch* b, int32_t keypoint, float* patch);
/* A TEST AID, and the one exception to "no CPU fallback": the definition above restated serially on the host for one
 * image, in the same FP32 operations and orders (sim3opt_amd/csrc/surf_host.hpp).  It needs no device and is never
 * used by sim3opt_surf_batch_solve.  Returns the image's number of keypoints (the arrays receive the first `capacity`
 * of them, each may be NULL) or SIM3OPT_ERR_ARG for what set_options or set_images would refuse.  counts[3]: the
 * candidates before and after the interpolation, the keypoints dropped.  S as debug_integral; det, trace of (resp_octave,
 * resp_layer) as debug_responses; the first cand_capacity candidates as debug_candidates.  Each may be NULL. */
int sim3opt_surf_reference_image(const sim3opt_surf_batch_options* o, int32_t width, int32_t height, int32_t row_stride,
                                 const uint8_t* pixels, int32_t capacity, float* kp, float* desc, float* size, float* angle,
                                 float* response, int32_t* octave, int32_t* laplacian, int32_t counts[3], int32_t* S,
                                 int32_t resp_octave, int32_t resp_layer, float* det, float* trace, int32_t cand_capacity,
                                 int32_t* cand_layer, float* cand_pos0, float* cand_response, uint8_t* cand_kept,
                                 float* cand_pos1);

/* ---- device-resident frame store (sim3opt_amd/csrc/frames.hip, frames_host.hpp) ----
 * One owner for "the frames of a sequence" on one device: kp_ptr (int32, n_frames + 1), kp (float, 2 N) and desc
 * (float, 64 N), contiguous, in the layout sim3opt_match_batch_set_frames, sim3opt_place_batch_set_frames and
 * sim3opt_vocabulary_set_frames take.  The extractor fills it on the device (sim3opt_surf_batch_solve_into) and the
 * three consumers read it in place (sim3opt_*_set_frames_from): the descriptors cross the host boundary never, and the
 * device holds them once.
 *   Snapshots.  What a store holds is an immutable, reference-counted snapshot.  A fill (sim3opt_frames_set,
 * sim3opt_surf_batch_solve_into, sim3opt_frames_debug_compact) makes a new one; a consumer that took the earlier one
 * keeps it alive and unchanged; the blocks go back to the device cache when the last holder -- the store or a consumer
 * -- lets go.  A fill has synchronised its stream before it returns, so consumers on streams of their own only ever
 * read finished memory and no event crosses streams.  A failed fill leaves the store as it was.
 *   The ordered compaction (k_frames_count, k_frames_scan_images, k_frames_move; new with the store): per image the
 * predicate state == 2 over the slots [cand_ptr[i], cand_ptr[i + 1]) is scanned in tiles of compact_tile slots, the
 * carry running from tile to tile; the kept rows are written in slot order behind those of the images before; the kept
 * count of every image is emitted.  No atomic takes part.  A 256-byte descriptor row is moved by 16 lanes with one
 * 16-byte load and store each, four rows a wavefront.
 * No CPU fallback: SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_frames sim3opt_frames;

typedef struct sim3opt_frames_options {
  int32_t device; /* -1: the calling thread's current device at the fill [-1] */
} sim3opt_frames_options;

void sim3opt_frames_options_default(sim3opt_frames_options* o);
sim3opt_frames* sim3opt_frames_create(void);
void sim3opt_frames_destroy(sim3opt_frames* s); /* consumers that took its snapshot keep theirs */
const char* sim3opt_frames_last_error(const sim3opt_frames* s);
/* SIM3OPT_ERR_ARG, nothing changed: a device below -1.  Another device than before empties the store (consumers keep
 * what they took). */
int sim3opt_frames_set_options(sim3opt_frames* s, const sim3opt_frames_options* o);
/* One upload from host arrays: replaces the three private uploads of the consumers' set_frames.  SIM3OPT_ERR_ARG with
 * nothing changed, in the words of those entries: n_frames < 1, a NULL array, a pointer array that does not start at 0
 * or decreases, too many keypoints for the int32 offsets, a non-finite keypoint or descriptor. */
int sim3opt_frames_set(sim3opt_frames* s, int32_t n_frames, const int32_t* kp_ptr, const float* kp, const float* desc);
/* Each may be NULL.  Before a fill: zeros, device -1.  desc_bytes: 256 N, the descriptor block as asked of the
 * allocator.  tiles: {compact_tile, row_lanes}. */
int sim3opt_frames_get_dims(const sim3opt_frames* s, int32_t* n_frames, int32_t* total_keypoints, int32_t* device,
                            int64_t* desc_bytes, int32_t tiles[2]);
/* The read-back (what sim3opt_surf_batch_get_keypoints' desc was): any pointer may be NULL.  SIM3OPT_ERR_STATE before
 * a fill. */
int sim3opt_frames_get(sim3opt_frames* s, int32_t* kp_ptr, float* kp, float* desc);
/* The compaction as an operator: the kernels of sim3opt_surf_batch_solve_into on caller-supplied slot arrays
 * (cand_ptr: n_images + 1; state: a value of 0 .. 3 per slot; slot_kp: 2 floats, slot_desc: 64 floats per slot); the
 * store is filled with the rows of state 2 in slot order.  SIM3OPT_ERR_ARG with nothing changed: n_images < 1, a NULL
 * array, a cand_ptr that does not start at 0 or decreases, a state outside 0 .. 3, a non-finite value. */
int sim3opt_frames_debug_compact(sim3opt_frames* s, int32_t n_images, const int32_t* cand_ptr, const int32_t* state,
                                 const float* slot_kp, const float* slot_desc);

/* sim3opt_surf_batch_solve, but kp and desc stay on the device: it replaces solve + get_keypoints(kp, desc) + the
 * consumers' uploads.  Same kernels and passes; the descriptors are not read back, and the host loop that dropped the
 * slots without a descriptor is the ordered compaction above for kp and desc.  Passes append: the store's arrays are
 * joined once, contiguous.  Afterwards get_kp_ptr, get_summary and get_keypoints with desc = NULL answer as after
 * solve; get_keypoints with desc != NULL answers SIM3OPT_ERR_STATE (read the store: sim3opt_frames_get).  Returns as
 * solve does.  SIM3OPT_ERR_ARG with the handle, the store and the device memory in use unchanged: a NULL store, a store
 * whose options.device names another device than the extractor's, a total beyond the int32 offsets. */
int sim3opt_surf_batch_solve_into(sim3opt_surf_batch* b, sim3opt_frames* store);
/* The consumers take the store's current snapshot in place of sim3opt_*_set_frames' arrays: no upload, no private
 * copy; everything downstream behaves as after set_frames with the same arrays.  SIM3OPT_ERR_ARG: a NULL store, a
 * handle whose options.device resolves to another device than the snapshot's, and what set_frames refuses of the frame
 * count, the descriptors (the trainer: all equal) or the remaining arguments; SIM3OPT_ERR_STATE: an unfilled store.
 * A refusal changes nothing.  set_frames afterwards drops the snapshot, and the other way round; set_options with
 * another device while a snapshot is held is SIM3OPT_ERR_ARG. */
int sim3opt_vocabulary_set_frames_from(sim3opt_vocabulary* b, const sim3opt_frames* store);
int sim3opt_place_batch_set_frames_from(sim3opt_place_batch* b, const sim3opt_frames* store);
/* n_frames (the length of obs_ptr less one: it must be the store's frame count), obs_ptr, obs_uv, obs_depth and the
 * intrinsics: as sim3opt_match_batch_set_frames */
int sim3opt_match_batch_set_frames_from(sim3opt_match_batch* b, const sim3opt_frames* store, int32_t n_frames,
                                        const int32_t* obs_ptr, const float* obs_uv, const float* obs_depth, double focal,
                                        double cx, double cy, int32_t image_width, int32_t image_height);

/* ---- batched loop tracks (sim3opt_amd/csrc/track_batch.hip, track_host.hpp, track_math.hpp) ----
 * The stage between the loop matches and the bundle adjustment: the kept matches of all loop pairs -> multi-view
 * tracks -> one 3-D point per track in the corrected world -> obs_cam / obs_point / obs_uv rows that
 * sim3opt_ba_set_problem takes once they are concatenated behind the map's.  computeConstraints records every kept match
 * as a two-observation track (kittiDetector.h:1493-1501, loopTracks.txt) and SaveAsSfMInit connects those
 * (kitti_surf.cpp:349-391, "there may be some points observed in several images, connect them").
 * PARITY: pinned on the reference's loopTracks.txt for the connection; the point, the gates and the BA rows unpinned --
 * the reference has no such step.
 *   Inputs.  Frames: kp_ptr (int32, n_frames + 1) and kp (float, 2 N), as every stage takes them; a frame may own
 * nothing.  Matches: pairs (int32, n_pairs x 2: frame0, frame1), match_ptr (n_pairs + 1), query_idx (a keypoint of
 * frame0) and train_idx (of frame1) per match and the optional depth0 / depth1 (double per match) exactly as
 * sim3opt_match_batch_get_match_ptr / _get_matches return them; mask: the uint8 inlier mask a RANSAC stage returns for
 * the same matches, or NULL.  A pair may have no match.  A depth that is not finite or not > 0 is absent, not an error.
 * Cameras: n_frames x 8 [qx qy qz qw tx ty tz s], S_iw as sim3opt_get_vertices returns it (q a unit quaternion, R its
 * rotation matrix: a world point X is seen at s R X + t), and the intrinsics.
 *   Tracks.  An observation is (frame, keypoint); its global index is g = kp_ptr[frame] + keypoint.  Kept matches are
 * those whose mask is absent or non-zero.  A track is a connected component of the graph whose vertices are the
 * observations on a side of a kept match and whose edges are the kept matches.  Tracks are numbered by ascending
 * smallest kept match index of the component (the key order of the reference's _TrackMap); the observations of a track
 * are listed by ascending g.
 *   Status per track, the first that applies in this order: */
enum {
  SIM3OPT_TRACK_OK = 0,
  SIM3OPT_TRACK_CONFLICT = 1,     /* two of the track's observations are in one frame (the reference assert(0)s,
                                     kitti_surf.cpp:393-407) */
  SIM3OPT_TRACK_NO_DEPTH = 2,     /* no observation of the track has a depth */
  SIM3OPT_TRACK_BEHIND = 3,       /* the point has z <= 0 in one of the track's cameras */
  SIM3OPT_TRACK_REPROJECTION = 4  /* the pixel gate below */
};
/*   Point of a track.  The depth of an observation is that of the lowest-indexed kept match having it on a side with a
 * depth present (side 0 before side 1 where one match has it on both).  For every observation with a depth d:
 * X_c = d ((u - cx) / f, (v - cy) / f, 1) and X_w = R^T (X_c - t) / s with its frame's state -- sim3opt_reanchor_points'
 * formula on a back-projected keypoint.  The point is the arithmetic mean of those X_w, summed in double in ascending g
 * and divided once; n_depths counts them; without any the point is 0.  No fused multiply-add takes part.
 *   Gate.  With options.max_reproj_px > 0 a track is REPROJECTION when the squared distance of any of its
 * observations, with or without a depth, from the point's projection (f x / z + cx, f y / z + cy) of s R X + t exceeds
 * max_reproj_px squared.  With 0 (the default: nothing in the reference fixes a threshold for mean-of-neighbours depths)
 * only z > 0 is required.
 *   DEVIATIONS from SaveAsSfMInit: a match between two observations that already sit in different tracks joins the
 * tracks (the reference prints a warning and drops the match); the order inside a track is by g, not by insertion; a
 * conflicting track is reported with a status instead of aborting; the point and the gates have no counterpart -- the
 * reference writes index lists only.
 *   Kernels (track_batch.hip says which): components by min-label hooking with 32-bit integer atomicMin and pointer
 * jumping, relaunched until a round hooks nothing -- the host reads one integer a round, and the fixed point (every
 * observation labelled with its component's smallest g) is unique, so nothing depends on arrival order; numbering and
 * layout by ordered scans in tiles with a carry; every segment ordered by rank; a lane per track for the point.  Integer
 * atomics only.  The launches depend on the rounds, never on the number of pairs or tracks.
 * No CPU fallback: SIM3OPT_ERR_NO_DEVICE without a GPU. */
typedef struct sim3opt_track_batch sim3opt_track_batch;

typedef struct sim3opt_track_batch_options {
  double max_reproj_px; /* the pixel gate; 0: none                                              [0]  */
  int32_t max_rounds;   /* hook-and-jump rounds a solve may take, the one that hooks nothing included [64] */
  int32_t device;       /* -1: the calling thread's current device                              [-1] */
} sim3opt_track_batch_options;

void sim3opt_track_batch_options_default(sim3opt_track_batch_options* o);
sim3opt_track_batch* sim3opt_track_batch_create(void);
void sim3opt_track_batch_destroy(sim3opt_track_batch* b);
const char* sim3opt_track_batch_last_error(const sim3opt_track_batch* b);
/* SIM3OPT_ERR_ARG, nothing changed: max_reproj_px negative or not finite, max_rounds < 1, a device below -1, another
 * device while a store's snapshot is held. */
int sim3opt_track_batch_set_options(sim3opt_track_batch* b, const sim3opt_track_batch_options* o);
/* The setters check on the host and keep a copy; the device is touched by solve.  A refusal changes nothing.  set_frames
 * (either form) drops the matches and the cameras; set_matches and set_cameras keep what else is set.
 * SIM3OPT_ERR_ARG: n_frames < 1, a NULL array, a kp_ptr that does not start at 0 or decreases, a non-finite pixel. */
int sim3opt_track_batch_set_frames(sim3opt_track_batch* b, int32_t n_frames, const int32_t* kp_ptr, const float* kp);
/* kp_ptr / kp of the store's current snapshot read in place: the snapshot is held the way the other consumers hold it,
 * and the handle allocates only its own work blocks.  Refusals as sim3opt_*_set_frames_from. */
int sim3opt_track_batch_set_frames_from(sim3opt_track_batch* b, const sim3opt_frames* store);
/* mask, depth0, depth1 may be NULL.  SIM3OPT_ERR_STATE before the frames; SIM3OPT_ERR_ARG: n_pairs < 1, a NULL array, a
 * match_ptr that does not start at 0 or decreases, a pair naming no frame, an index outside its frame, 2^30 matches or
 * more. */
int sim3opt_track_batch_set_matches(sim3opt_track_batch* b, int32_t n_pairs, const int32_t* pairs, const int32_t* match_ptr,
                                    const int32_t* query_idx, const int32_t* train_idx, const uint8_t* mask,
                                    const double* depth0, const double* depth1);
/* SIM3OPT_ERR_STATE before the frames; SIM3OPT_ERR_ARG: a NULL array, another frame count than the frames', a
 * non-finite state or intrinsic, s <= 0, focal <= 0. */
int sim3opt_track_batch_set_cameras(sim3opt_track_batch* b, int32_t n_frames, const double* states, double focal, double cx,
                                    double cy);
/* The number of status-0 tracks (0 with every match masked: no error), or a negative code: SIM3OPT_ERR_STATE before
 * frames, matches and cameras are set; SIM3OPT_ERR_ARG with "the components did not settle in max_rounds = ..." when
 * the rounds run out (never an endless loop; the handle solves again with a larger max_rounds). */
int sim3opt_track_batch_solve(sim3opt_track_batch* b);
/* Each may be NULL; zeros for what is not there yet.  rounds: the hook-and-jump rounds of the last solve, the one that
 * hooked nothing included.  tiles: {workgroup size, scan tile, the longest segment a lane orders, the longest a
 * wavefront orders (longer ones: a workgroup)}. */
int sim3opt_track_batch_dims(const sim3opt_track_batch* b, int32_t* n_frames, int32_t* n_pairs, int32_t* total_matches,
                             int32_t* n_tracks, int32_t* n_observations, int32_t* n_kept_tracks,
                             int32_t* n_kept_observations, int32_t* rounds, int32_t tiles[4]);
/* The getters: SIM3OPT_ERR_STATE before the first solve; any pointer may be NULL.
 * Every track: track_ptr (n_tracks + 1), obs_frame / obs_keypoint (n_observations), status and first_match, the
 * smallest kept match of the track (n_tracks). */
int sim3opt_track_batch_get_tracks(sim3opt_track_batch* b, int32_t* track_ptr, int32_t* obs_frame, int32_t* obs_keypoint,
                                   int32_t* status, int32_t* first_match);
/* the track of every match (total_matches), -1 where masked */
int sim3opt_track_batch_get_match_track(sim3opt_track_batch* b, int32_t* match_track);
/* points: n_tracks x 3; n_depths: n_tracks */
int sim3opt_track_batch_get_points(sim3opt_track_batch* b, double* points, int32_t* n_depths);
/* The status-0 tracks only, in order: points (n_kept_tracks x 3), and per observation of theirs obs_cam = the frame,
 * obs_point = point_base + the track's rank among the kept, obs_uv = the keypoint's pixels (double, 2 each): the rows
 * sim3opt_ba_set_problem takes behind a map of point_base points.  SIM3OPT_ERR_ARG: point_base < 0 or beyond int32. */
int sim3opt_track_batch_get_ba(sim3opt_track_batch* b, int32_t point_base, double* points, int32_t* obs_cam,
                               int32_t* obs_point, double* obs_uv);
/* A test aid: the serial restatement of the definition above (track_host.hpp: union-find, then the arithmetic the
 * kernels share) on the host, with no handle and no device.  Outputs may be NULL; the caller sizes track_ptr for
 * total_matches + 1, the per-track arrays for total_matches and the per-observation arrays for 2 total_matches entries.
 * SIM3OPT_ERR_ARG for what the setters refuse. */
int sim3opt_track_reference(int32_t n_frames, const int32_t* kp_ptr, const float* kp, int32_t n_pairs, const int32_t* pairs,
                            const int32_t* match_ptr, const int32_t* query_idx, const int32_t* train_idx,
                            const uint8_t* mask, const double* depth0, const double* depth1, const double* states,
                            double focal, double cx, double cy, double max_reproj_px, int32_t* n_tracks,
                            int32_t* n_observations, int32_t* track_ptr, int32_t* obs_frame, int32_t* obs_keypoint,
                            int32_t* status, int32_t* first_match, int32_t* match_track, double* points,
                            int32_t* n_depths);

/* ---- stepwise optimisation, stage 1 (host C++) ----
 * "scale_dlt" of testStepwiseSim3Optimization                        kitti_surf.cpp:887-933
 * Null vector of the edge equations s_C x[v0] - x[v1] = 0 (the reference: last column of V of
 * Eigen::JacobiSVD), divided by its first entry, written into the scale of every vertex estimate.
 * Needs dense vertex ids 0..n-1 and n <= 4096.  sigma_ratio (optional) receives an estimate of
 * sigma_min / sigma_max (the reference warns below 5e-4).  Stage 2 / 3 are optimize() runs with
 * dof_mask = 0x78 (rotations frozen) / 127, each warm-started from the previous stage. */
int sim3opt_stepwise_scale_init(sim3opt_graph* g, double* sigma_ratio);

/* ---- evaluation harness (host C++) ----
 * estimateSimilarityTransform = Eigen::umeyama(query, train, true)   kitti_surf.cpp:1091-1161
 * followed by the RMSE / max deviation of the aligned positions      kitti_surf.cpp:1446-1463.
 * S is the 4x4 row-major similarity [cR t; 0 1] mapping query to train coordinates. */
int sim3opt_align_trajectory(int32_t n, const double* query_xyz /*n x 3*/,
                             const double* train_xyz /*n x 3*/, int32_t with_scale, double S[16],
                             double* rmse, double* max_dev);

#ifdef __cplusplus
}
#endif
#endif /* SIM3OPT_H */
