// engine.hpp -- device-resident Levenberg-Marquardt engine (interface).
//
// Replaces g2o's OptimizationAlgorithmLevenberg + BlockSolverX + LinearSolverEigen
// (instantiated at kitti_surf.cpp:552-558) and the per-edge / per-vertex virtual calls
// behind SparseOptimizer::optimize (kitti_surf.cpp:675).  Implementation: engine.hip.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "graph.hpp"

namespace sim3opt {

class Engine;  // opaque, defined in engine.hip

struct Comm;
// comm (may be null) is moved into the engine
Engine* engine_create(const HostGraph& g, const Structure& s, const sim3opt_options& opt,
                      Comm* comm, std::string& err, int& status);
void engine_local_rows(const Engine* e, int32_t* begin, int32_t* end);
void engine_destroy(Engine* e);
// hands the communicator back before the engine is destroyed (re-initialisation)
void engine_take_comm(Engine* e, Comm* out);

int engine_set_options(Engine* e, const sim3opt_options& opt);
int engine_optimize(Engine* e, int32_t max_iters, std::vector<sim3opt_iter_stats>& stats,
                    std::string& err);
// trust-region records of the last optimize() (dogleg; empty after LM and Gauss-Newton)
void engine_trust_region_stats(const Engine* e, std::vector<sim3opt_tr_stats>& out);
int engine_chi2(Engine* e, double* chi2, std::string& err);
int engine_get_states(Engine* e, sim3::Sim3* out, std::string& err);
int engine_set_states(Engine* e, const sim3::Sim3* in, std::string& err);
int engine_edge_errors(Engine* e, double* out, std::string& err);
// g2o Edge::chi2() (e^T Omega e), rho and rho' of each edge's kernel, all edges in insertion order (null: skipped)
int engine_edge_chi2(Engine* e, double* chi2, double* rho, double* weight, std::string& err);
// uploads g.kdelta / g.kkind (allocated on first use); the next chi2 / linearisation uses them
int engine_set_kernels(Engine* e, const HostGraph& g, std::string& err);
int engine_edge_jacobians(Engine* e, double* e_out, double* J_out, std::string& err);
int engine_linearize(Engine* e, std::string& err);
int engine_get_system(Engine* e, int32_t* rowptr, int32_t* colidx, double* values, double* b,
                      std::string& err);
int engine_solve(Engine* e, double lambda, double* x, int32_t* iters, double* rel_res,
                 std::string& err);
// blocks (row_a[q], row_b[q]) of (H + lambda I)^-1, H linearised at the current estimates (engine_direct.hip)
int engine_marginals(Engine* e, double lambda, int32_t n, const int32_t* row_a, const int32_t* row_b, double* cov,
                     std::string& err);
// ... for any pair of free vertices (blocks outside the factor's pattern: cov_kernels.hpp), and what the last such
// call did: {chunks, root paths walked, distinct pairs outside the pattern, pairs on it, workspace bytes, selected
// inversion run}
int engine_covariances(Engine* e, double lambda, int32_t n, const int32_t* row_a, const int32_t* row_b, double* cov,
                       std::string& err);
void engine_covariance_stats(const Engine* e, int64_t out[6]);
// what the last call that took the blocks by columns of the inverse did (options.cov_solver; engine_columns.hip):
// counts = {vertices solved, columns, PCG iterations over the columns, refinement rounds, batches}, res = {largest
// true relative residual, cov_rel_tol used}; failed_vertex (may be null): the vertex index of a column that failed, or -1
void engine_covariance_columns_stats(const Engine* e, int64_t counts[5], double res[2], int32_t* failed_vertex);
// chi-square gate of candidate edges (vertex indices, their block rows or -1 when fixed, Omega^-1 n x 49)
int engine_gate_edges(Engine* e, double lambda, int32_t n, const int32_t* v0, const int32_t* v1, const int32_t* row0,
                      const int32_t* row1, const sim3::Sim3* meas, const double* infoinv, double* e_out, double* S_out,
                      double* d2_out, std::string& err);
// diagnostic read-outs of the preconditioners (one GPU; the solver's state is left as it was)
int engine_amg_level_numbers(Engine* e, double lambda, int32_t level, int32_t* rowptr, int32_t* colidx, double* vals,
                             float* vals32, double* W, double* diagH, double* Minv, double* P, std::string& err);
int engine_amg_coarsest_inverse(Engine* e, double lambda, double* Ainv, std::string& err);
int engine_precond_apply(Engine* e, int32_t prec, double lambda, int32_t nrhs, const double* r, double* z,
                         std::string& err);
// diagnostic read-outs of the LM set-up and update kernels (one GPU; the solver's state is left as it was)
void engine_debug_linearization_dims(const Engine* e, int32_t* n_active, int32_t* n_incidences);
int engine_debug_linearization(Engine* e, double* J, double* w, int32_t* active, double* scratch, int32_t* incptr,
                               int32_t* inc0, int32_t* inc1, int32_t* slot01, int32_t* slot10, double* trace,
                               double* maxdiag, std::string& err);
int engine_debug_update(Engine* e, const double* x, double lambda, bool with_fail, int32_t grid, double* states_out,
                        double* backup_out, double* chi2, double* scale, std::string& err);
// diagnostic read-outs of the dogleg's launches (engine_algorithms.hip) and of the column kernels (engine_columns.hip)
int engine_debug_dogleg(Engine* e, const double* h_gn, double ca, double cg, bool with_fail, int32_t grid, int64_t j0,
                        int64_t j1, double* scalars, double* states_out, double* backup_out, std::string& err);
int engine_debug_column_vectors(Engine* e, int32_t op, int32_t grid, int64_t n, int32_t K, const int64_t* at,
                                int32_t sys, const double* a, const double* b, int32_t first, int32_t count,
                                int32_t col, const int32_t* rows, int32_t n_blocks, double* out, std::string& err);
// the dogleg's step rule (dogleg_rule.hpp; host only, no engine): scalars in the order of DL_*; model = {alpha, norm_sd,
// norm_gn}, trial = {ca, cg, norm_dl, linearGain}, *step = SIM3OPT_STEP_*
void engine_dogleg_rule(const double scalars[6], double delta, double model[3], double trial[4], int32_t* step);
// diagnostic read-out of the exact block Cholesky, its solve and the selected inversion (engine_direct.hip)
int engine_debug_factor_dims(Engine* e, int32_t context, int32_t* nb, int64_t* nL, int64_t* nnzb, std::string& err);
int engine_debug_factor(Engine* e, int32_t context, double lambda, const double* vals, const double* b, bool with_solve,
                        bool with_selinv, double* Aperm, double* bp, double* L, double* Dinv, double* y, double* xp,
                        double* x, int32_t* fail, double* Z, int32_t* singular, int32_t* bord, int32_t* brow,
                        std::string& err);
// diagnostic read-outs of the PCG's operator (engine_pcg.hip)
int engine_spmv_spans(Engine* e, int32_t* n_spans, int32_t* wrow, std::string& err);
int engine_operator_apply(Engine* e, int32_t nrhs, const double* lambda, const double* p, const double* rvec, double* q,
                          double* pq, double* rp, std::string& err);
int engine_span_grid(const Engine* e);  // workgroups of the span SpMV in use
void engine_spmv_variant(const Engine* e, int32_t* chunk, int32_t* non_temporal);  // the instantiation spmv_raw launches
int engine_bench_spmv(Engine* e, int32_t reps, double* ms_mean, std::string& err);
int engine_bench_stream(Engine* e, int32_t mode, int32_t reps, double* ms_mean, std::string& err);
int engine_preconditioner(const Engine* e);
int engine_linear_solver(const Engine* e);
void engine_amg_in_use(const Engine* e, int32_t* n_levels, int32_t* n_partitioned, int32_t visits[4]);
void engine_device_bytes(const Engine* e, int64_t bytes[2]);
int engine_kernel_times(Engine* e, sim3opt_kernel_times* out, bool reset);
int engine_comm_times(Engine* e, sim3opt_comm_times* out);
// diagnostic read-outs of the in-process transport: ONE collective of this rank's communicator on this rank's stream, on
// this rank's operand in a guarded scratch block (phase 0 / 1: on an even / odd double of a 16-byte aligned block); a
// guard that changed is SIM3OPT_ERR_STATE naming the rank and the index.  Every rank of the group calls the same one.
int engine_comm_apply_allreduce(Engine* e, int32_t n, int32_t op, int32_t phase, const double* in, double* out,
                                std::string& err);
int engine_comm_apply_allgatherv(Engine* e, const int64_t* offs, int32_t phase, const double* in, double* out,
                                 std::string& err);
int engine_comm_apply_exchange(Engine* e, const int64_t* soffs, const int64_t* roffs, int32_t send_phase,
                               int32_t recv_phase, const double* send, double* recv, std::string& err);
// {mailbox capacity in doubles, collectives so far} of rank 0 (the same on every rank); false: not that transport
bool engine_comm_local_state(const Engine* e, int64_t out[2]);
// the PCG loops' schedule since the last reset: {iterations enqueued, of them after `done`, polls that synchronised
// with an empty queue behind them, polls waited for with the next chunk queued}
void engine_pcg_schedule_stats(Engine* e, int64_t out[4], bool reset);

}  // namespace sim3opt
