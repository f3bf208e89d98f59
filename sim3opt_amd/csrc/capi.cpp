// capi.cpp -- the C-ABI of libsim3opt (include/sim3opt.h): argument checking, the host graph
// container and dispatch into the HIP engine.  No exceptions leave this file.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "../../include/sim3opt_bench.h"
#include "amg.hpp"
#include "col_plan.hpp"
#include "comm.hpp"
#include "comm_apply_host.hpp"
#include "devmem.hpp"
#include "direct.hpp"
#include "engine.hpp"
#include "graph.hpp"
#include "handle_device.hpp"
#include "rank_group.hpp"
#include "robust.hpp"
#include "sim3_jac.hpp"

using namespace sim3opt;

struct sim3opt_graph {
  HostGraph host;
  Structure structure;
  sim3opt_options opt;
  Engine* engine = nullptr;
  bool initialized = false;
  bool dirty = false;  // vertices/edges added since the last initialize (g2o: re-initialize)
  std::vector<sim3opt_iter_stats> stats;
  std::vector<sim3opt_tr_stats> tr_stats;  // dogleg runs only
  int32_t last_algorithm = SIM3OPT_ALGORITHM_LM;  // of the last optimize()
  std::string err;
  Comm comm;        // handed to the engine at initialize
  bool comm_set = false;
  bool comm_called = false;  // sim3opt_comm_init* was called: the ranks come from outside (no sim3opt_set_devices)
  // sim3opt_set_devices: with n > 1 the ranks live in here, one engine each, and `engine` is rank 0's (not owned)
  bool devices_set = false;
  int32_t device_one = -1;  // n == 1: the ordinal it chose
  std::unique_ptr<RankGroup> group;
  ~sim3opt_graph() {
    if (group) engine = nullptr;  // (the group releases the engines, each under its own device)
    group.reset();
    if (engine) engine_destroy(engine);
  }
};

namespace {

int fail(sim3opt_graph* g, int code, const char* msg) {
  if (g) g->err = msg;
  return code;
}

bool state_ok(const double s[8]) {
  for (int i = 0; i < 8; ++i)
    if (!std::isfinite(s[i])) return false;
  return s[7] > 0.0;
}

sim3::Sim3 to_sim3(const double s[8]) {
  sim3::Sim3 r;
  r.q[0] = s[0]; r.q[1] = s[1]; r.q[2] = s[2]; r.q[3] = s[3];
  r.t[0] = s[4]; r.t[1] = s[5]; r.t[2] = s[6]; r.s = s[7];
  return r;
}

void from_sim3(const sim3::Sim3& r, double s[8]) {
  s[0] = r.q[0]; s[1] = r.q[1]; s[2] = r.q[2]; s[3] = r.q[3];
  s[4] = r.t[0]; s[5] = r.t[1]; s[6] = r.t[2]; s[7] = r.s;
}

bool is_identity77(const double* m) {
  for (int c = 0; c < 7; ++c)
    for (int r = 0; r < 7; ++r)
      if (m[7 * c + r] != (r == c ? 1.0 : 0.0)) return false;
  return true;
}

// An engine call f(engine, rank, err) of a public entry: on the handle's one engine, or, on a handle with several
// ranks, on every rank's worker (all == false: on rank 0's only -- read-outs of what every rank holds a replica of,
// which run no collective).  Returns the lowest failing rank's code with its message in the handle, else rank 0's.
template <class F>
int on_ranks(sim3opt_graph* g, F f, bool all = true) {
  if (!g->group) return f(g->engine, 0, g->err);
  return g->group->run([&](RankCtx& c) { return f(c.engine, (int)c.rank, c.err); }, g->err, all);
}

// after a rank failed or timed out inside a collective the ranks are out of step for good
bool finished(const sim3opt_graph* g) { return g && g->group && g->group->broken(); }
const char* const FINISHED = "a rank failed or timed out: the handle is finished (sim3opt_destroy is what is left)";
#define REFUSE_FINISHED(g) \
  if (finished(g)) return fail(g, SIM3OPT_ERR_STATE, FINISHED)
// entries that serve one rank only (as on a graph partitioned over processes)
#define REFUSE_RANKS(g, who) \
  if ((g)->group) return fail(g, SIM3OPT_ERR_STATE, who ": one rank only (the graph is partitioned over ranks)")

// pulls the current estimates back into the host container (so get/set work either side of
// initialize, like g2o's vertex objects)
int sync_host_states(sim3opt_graph* g) {
  if (!g->initialized) return SIM3OPT_OK;
  return on_ranks(g, [&](Engine* e, int, std::string& err) { return engine_get_states(e, g->host.states.data(), err); },
                  false);
}

int push_host_states(sim3opt_graph* g) {
  return on_ranks(g, [&](Engine* e, int, std::string& err) { return engine_set_states(e, g->host.states.data(), err); });
}

// (no HIP call in f: the workers are idle between two commands)
template <class F>
void for_engines(sim3opt_graph* g, F f) {
  if (!g->group) {
    if (g->engine) f(g->engine);
    return;
  }
  for (int32_t r = 0; r < g->group->size(); ++r)
    if (g->group->ctx(r).engine) f(g->group->ctx(r).engine);
}

// a kind / delta pair as sim3opt_add_edge and sim3opt_set_edge_kernels accept it
bool kernel_ok(int32_t kind, double delta) {
  if (kind < 0 || kind >= ROBUST_KINDS) return false;
  return kind == SIM3OPT_KERNEL_NONE || (std::isfinite(delta) && delta > 0.0);
}

// first edge with a kernel: every earlier edge gets SIM3OPT_KERNEL_NONE
void materialise_kernels(HostGraph& h) {
  if (h.has_kernel) return;
  h.has_kernel = true;
  h.kdelta.assign(h.ev0.size(), 0.0);
  h.kkind.assign(h.ev0.size(), (uint8_t)SIM3OPT_KERNEL_NONE);
}

int add_edge_impl(sim3opt_graph* g, int32_t id0, int32_t id1, const double* meas,
                  const double* info, int32_t kernel, double kdelta) {
  auto a = g->host.id2idx.find(id0), b = g->host.id2idx.find(id1);
  if (a == g->host.id2idx.end() || b == g->host.id2idx.end())
    return fail(g, SIM3OPT_ERR_ARG, "add_edge: unknown vertex id");
  if (a->second == b->second) return fail(g, SIM3OPT_ERR_ARG, "add_edge: identical endpoints");
  if (!state_ok(meas)) return fail(g, SIM3OPT_ERR_ARG, "add_edge: non-finite measurement or scale <= 0");
  if (kernel < 0 || kernel >= ROBUST_KINDS) return fail(g, SIM3OPT_ERR_ARG, "add_edge: unknown robust kernel");
  if (!kernel_ok(kernel, kdelta))
    return fail(g, SIM3OPT_ERR_ARG, "add_edge: robust kernel delta must be finite and > 0");
  HostGraph& h = g->host;
  const size_t m = h.ev0.size();
  const bool nonident = info && !is_identity77(info);
  if (nonident && !h.has_info) {  // first non-identity information: materialise I7 for earlier edges
    h.has_info = true;
    h.info.assign(49 * m, 0.0);
    for (size_t k = 0; k < m; ++k)
      for (int d = 0; d < 7; ++d) h.info[49 * k + 8 * d] = 1.0;
  }
  if (h.has_info) {
    const size_t off = h.info.size();
    h.info.resize(off + 49, 0.0);
    if (info) std::memcpy(&h.info[off], info, sizeof(double) * 49);
    else for (int d = 0; d < 7; ++d) h.info[off + 8 * d] = 1.0;
  }
  const bool has_k = kernel != SIM3OPT_KERNEL_NONE;
  if (has_k) materialise_kernels(h);
  if (h.has_kernel) {
    h.kdelta.push_back(has_k ? kdelta : 0.0);
    h.kkind.push_back((uint8_t)kernel);
  }
  h.ev0.push_back(a->second);
  h.ev1.push_back(b->second);
  h.meas.push_back(to_sim3(meas));
  return SIM3OPT_OK;
}

}  // namespace

extern "C" {

// 1.1: multigrid preconditioner, hierarchy / BAL entry points; 1.2: closed-form Jacobians (options.jacobians);
// 1.3: robust kernels beyond Huber, per edge and changeable after initialize
// (Gauss-Newton and dogleg -- options.algorithm and the dl_* fields appended to sim3opt_options,
// sim3opt_get_trust_region_stats -- keep 130: tests/test_robust_kernels.py pins the number; the new export is
// how a caller detects them; likewise options.cov_solver / cov_rel_tol and sim3opt_covariance_columns_plan / _stats)
int sim3opt_version(void) { return 130; }

void sim3opt_options_default(sim3opt_options* o) {
  if (!o) return;
  o->tau = 1e-5;
  o->user_lambda_init = 0.0;
  o->good_step_lower = 1.0 / 3.0;
  o->good_step_upper = 2.0 / 3.0;
  o->max_trials = 10;
  o->fd_delta = 1e-9;
  o->exp_eps = 1e-5;
  o->small_rot_half = 0;
  o->fix_small_angle_b = 0;
  o->dof_mask = 127;
  o->pcg_max_iters = 0;
  o->pcg_rel_tol = 1e-10;
  o->pcg_check_every = 16;
  o->pcg_graph = 1;
  o->preconditioner = -1;
  o->chain_segment = 256;
  o->device = -1;
  o->verbose = 0;
  o->time_kernels = 0;
  o->linear_solver = -1;
  for (int32_t& v : o->amg_cycle) v = 0;
  for (int32_t& v : o->amg_passes) v = 0;
  o->amg_additive = 0;
  o->amg_fp32 = 1;
  o->amg_pivot = 14;
  o->amg_coarsest = 256;
  o->adaptive_prec = 1;
  o->row_order = -1;
  o->halo_exchange = 1;
  o->span_grid = 0;
  o->force_collectives = 0;
  o->amg_shard_rows = 4096;
  o->amg_virtual_ranks = 0;
  o->pcg_batch = 0;
  o->amg_omega = 0.9;
  o->amg_over[0] = 1.8;
  o->amg_over[1] = 1.6;
  o->direct_max_pairs = 0;
  o->debug_full_arrays = 0;
  o->jacobians = 0;
  o->algorithm = SIM3OPT_ALGORITHM_LM;
  o->dl_max_trials = 100;
  o->dl_delta_init = 1e4;
  o->dl_lambda_init = 1e-7;
  o->dl_lambda_factor = 10.0;
  o->cov_workspace_mb = 256.0;
  o->cov_solver = 0;
  o->cov_rel_tol = 1e-8;
}

// Debug overrides: a SIM3OPT_* environment variable replaces the option field of the same name when the
// graph is initialised (tests and tuning scripts drive the library that way); the override lands in the
// handle's options, so sim3opt_get_options reports what was used.
static void apply_env_overrides(sim3opt_options& o) {
  auto digits = [](const char* ev, int32_t* dst, int n, int lo, int hi) {
    int last = 0;
    const int len = (int)std::strlen(ev);
    for (int l = 0; l < n; ++l) {
      if (l < len && ev[l] - '0' >= lo && ev[l] - '0' <= hi) last = ev[l] - '0';
      dst[l] = last;
    }
  };
  if (const char* ev = std::getenv("SIM3OPT_AMG_CYCLE")) digits(ev, o.amg_cycle, 4, 1, 3);    // "122": levels 1, 2, 3...
  if (const char* ev = std::getenv("SIM3OPT_AMG_PASSES")) digits(ev, o.amg_passes, 3, 1, 6);  // "344"
  if (const char* ev = std::getenv("SIM3OPT_AMG_ADDITIVE")) o.amg_additive = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SIM3OPT_AMG_FP32")) o.amg_fp32 = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SIM3OPT_AMG_PIVOT")) o.amg_pivot = std::atoi(ev);
  if (const char* ev = std::getenv("SIM3OPT_AMG_COARSEST")) o.amg_coarsest = std::atoi(ev);
  if (const char* ev = std::getenv("SIM3OPT_ADAPTIVE_PREC")) o.adaptive_prec = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SIM3OPT_ROW_ORDER")) o.row_order = std::string(ev) == "bfs" ? 1 : 0;
  if (std::getenv("SIM3OPT_NO_HALO")) o.halo_exchange = 0;
  if (const char* ev = std::getenv("SIM3OPT_SPAN_GRID")) o.span_grid = std::atoi(ev);
  if (const char* ev = std::getenv("SIM3OPT_FORCE_COMM")) o.force_collectives = ev[0] == '1';
  if (const char* ev = std::getenv("SIM3OPT_AMG_SHARD_ROWS")) o.amg_shard_rows = std::atoi(ev);
  if (const char* ev = std::getenv("SIM3OPT_AMG_VIRTUAL_RANKS")) o.amg_virtual_ranks = std::atoi(ev);
  if (const char* ev = std::getenv("SIM3OPT_PCG_BATCH")) o.pcg_batch = std::atoi(ev);
  if (const char* ev = std::getenv("SIM3OPT_AMG_OMEGA")) o.amg_omega = std::atof(ev);
  if (const char* ev = std::getenv("SIM3OPT_AMG_OVER")) {  // "a0[,a1]": the last value repeats
    o.amg_over[0] = o.amg_over[1] = std::atof(ev);
    if (const char* c = std::strchr(ev, ',')) o.amg_over[1] = std::atof(c + 1);
  }
  if (const char* ev = std::getenv("SIM3OPT_DIRECT_MAX_PAIRS")) o.direct_max_pairs = std::atoll(ev);
  if (const char* ev = std::getenv("SIM3OPT_DEBUG_FULL_ARRAYS")) o.debug_full_arrays = std::atoi(ev) != 0;
  // (a fraction of a MiB is accepted here only: tests chunk a small request that way)
  if (const char* ev = std::getenv("SIM3OPT_COV_WORKSPACE_MB"))
    if (std::atof(ev) > 0.0) o.cov_workspace_mb = std::atof(ev);
  if (const char* ev = std::getenv("SIM3OPT_COV_SOLVER"))
    if (std::atoi(ev) >= 0 && std::atoi(ev) <= 2) o.cov_solver = std::atoi(ev);
  if (const char* ev = std::getenv("SIM3OPT_COV_REL_TOL"))
    if (std::atof(ev) > 0.0 && std::atof(ev) <= 1e-2) o.cov_rel_tol = std::atof(ev);
}

sim3opt_graph* sim3opt_create(void) { return sim3opt::handle_create<sim3opt_graph>(sim3opt_options_default); }

void sim3opt_destroy(sim3opt_graph* g) { sim3opt::handle_destroy(g); }

void sim3opt_release_device_cache(void) { sim3opt::dev_cache_release(); }

void sim3opt_device_memory_in_use(int64_t out[2]) {
  if (out) sim3opt::dev_in_use(out);
}

void sim3opt_debug_device_memory(int32_t on) { sim3opt::dev_debug(on != 0); }

void sim3opt_debug_device_memory_report(int64_t out[4]) {
  if (out) sim3opt::dev_debug_report(out);
}

int64_t sim3opt_debug_device_memory_probe(int64_t bytes, int32_t floating, int64_t overrun, unsigned char* out,
                                          int64_t out_len) {
  if (bytes < 0 || overrun < 0 || out_len < 0 || (out_len > 0 && !out) || bytes > ((int64_t)1 << 30))
    return SIM3OPT_ERR_ARG;
  size_t size = 0;
  const hipError_t e = sim3opt::dev_debug_probe((size_t)bytes, floating != 0, (size_t)overrun, out, (size_t)out_len, &size);
  if (e == hipErrorInvalidValue) return SIM3OPT_ERR_ARG;  // (the overrun would leave the block)
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return SIM3OPT_ERR_HIP;
  }
  return (int64_t)size;
}

int sim3opt_set_options(sim3opt_graph* g, const sim3opt_options* o) {
  if (!g || !o) return fail(g, SIM3OPT_ERR_ARG, "set_options: null argument");
  REFUSE_FINISHED(g);
  if (!(o->fd_delta > 0) || !(o->exp_eps > 0) || o->max_trials < 1 || !(o->pcg_rel_tol >= 0) ||
      !(o->tau > 0) || o->pcg_check_every < 0 || o->amg_virtual_ranks < 0 || o->pcg_batch < 0 ||
      o->direct_max_pairs < 0 || !(o->amg_omega > 0) || !(o->amg_over[0] > 0) || !(o->amg_over[1] > 0))
    return fail(g, SIM3OPT_ERR_ARG, "set_options: value out of range");
  if (o->jacobians != 0 && o->jacobians != 1)
    return fail(g, SIM3OPT_ERR_ARG, "set_options: jacobians must be 0 (numeric) or 1 (analytic)");
  if (o->algorithm < SIM3OPT_ALGORITHM_LM || o->algorithm > SIM3OPT_ALGORITHM_DOGLEG)
    return fail(g, SIM3OPT_ERR_ARG, "set_options: algorithm must be 0 (LM), 1 (Gauss-Newton) or 2 (dogleg)");
  {
    auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (!pos(o->dl_delta_init) || !pos(o->dl_lambda_init) || !pos(o->dl_lambda_factor) || o->dl_max_trials < 1)
      return fail(g, SIM3OPT_ERR_ARG,
                  "set_options: dl_delta_init, dl_lambda_init and dl_lambda_factor must be finite and positive, "
                  "dl_max_trials at least 1");
  }
  // (a fraction put there by the environment override comes back through get / change another field / set)
  if ((!(o->cov_workspace_mb >= 1.0) && o->cov_workspace_mb != g->opt.cov_workspace_mb) ||
      !std::isfinite(o->cov_workspace_mb))
    return fail(g, SIM3OPT_ERR_ARG, "set_options: cov_workspace_mb must be finite and at least 1");
  if (o->cov_solver < 0 || o->cov_solver > 2)
    return fail(g, SIM3OPT_ERR_ARG, "set_options: cov_solver must be 0 (exact), 1 (columns by PCG) or 2 (exact where the plan is accepted)");
  if (!std::isfinite(o->cov_rel_tol) || !(o->cov_rel_tol > 0.0) || !(o->cov_rel_tol <= 1e-2))
    return fail(g, SIM3OPT_ERR_ARG, "set_options: cov_rel_tol must be finite and in (0, 1e-2]");
  if (o->jacobians == 1 && o->fix_small_angle_b != 1)
    return fail(g, SIM3OPT_ERR_ARG,
                "set_options: jacobians = 1 needs fix_small_angle_b = 1 (the closed form differentiates the exact "
                "map; log's as-written small-angle B departs from it by O(1) below theta ~ 4.5e-3)");
  // span_grid: the handle keeps the caller's REQUEST (clamped anew at every sim3opt_initialize) while
  // sim3opt_get_options reports the value in use; a value that is the reported one leaves the request as it is, so
  // that get / change another field / set does not turn the clamp into the request
  const int32_t span_request = g->opt.span_grid;
  const bool span_as_reported = g->engine && span_request > 0 && o->span_grid == engine_span_grid(g->engine);
  g->opt = *o;
  if (span_as_reported) g->opt.span_grid = span_request;
  if (g->devices_set && !g->group) g->opt.device = g->device_one;  // (sim3opt_set_devices chose it)
  for_engines(g, [&](Engine* e) { engine_set_options(e, g->opt); });  // (an engine keeps its own device)
  return SIM3OPT_OK;
}

int sim3opt_get_options(const sim3opt_graph* g, sim3opt_options* o) {
  if (!g || !o) return SIM3OPT_ERR_ARG;
  *o = g->opt;
  if (g->engine && o->span_grid > 0) o->span_grid = engine_span_grid(g->engine);  // (as clamped for this graph)
  return SIM3OPT_OK;
}

const char* sim3opt_last_error(const sim3opt_graph* g) { return g ? g->err.c_str() : "null graph"; }

int sim3opt_add_vertex(sim3opt_graph* g, int32_t id, const double state[8], int32_t fixed) {
  try {
  if (!g || !state) return fail(g, SIM3OPT_ERR_ARG, "add_vertex: null argument");
  REFUSE_FINISHED(g);
  if (g->initialized) g->dirty = true;  // needs initializeOptimization() again, like g2o
  if (!state_ok(state)) return fail(g, SIM3OPT_ERR_ARG, "add_vertex: non-finite state or scale <= 0");
  HostGraph& h = g->host;
  if (!h.id2idx.emplace(id, (int32_t)h.vid.size()).second)
    return fail(g, SIM3OPT_ERR_ARG, "add_vertex: duplicate id");  // g2o addVertex returns false
  h.vid.push_back(id);
  h.states.push_back(to_sim3(state));
  h.fixed.push_back(fixed ? 1 : 0);
  return SIM3OPT_OK;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return fail(g, SIM3OPT_ERR_ARG, "add_vertex: out of host memory or internal error");
  }
}

int sim3opt_add_vertices(sim3opt_graph* g, int32_t n, const int32_t* ids, const double* states,
                         const uint8_t* fixed) {
  try {
  if (!g || n < 0 || (n > 0 && !states)) return fail(g, SIM3OPT_ERR_ARG, "add_vertices: bad argument");
  HostGraph& h = g->host;
  h.vid.reserve(h.vid.size() + n);
  h.states.reserve(h.states.size() + n);
  h.fixed.reserve(h.fixed.size() + n);
  h.id2idx.reserve(h.id2idx.size() + n);
  const int32_t base = (int32_t)h.vid.size();
  for (int32_t k = 0; k < n; ++k) {
    const int rc = sim3opt_add_vertex(g, ids ? ids[k] : base + k, states + 8 * (size_t)k,
                                      fixed ? fixed[k] : 0);
    if (rc != SIM3OPT_OK) return rc;
  }
  return SIM3OPT_OK;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return fail(g, SIM3OPT_ERR_ARG, "add_vertices: out of host memory or internal error");
  }
}

int sim3opt_add_edge(sim3opt_graph* g, int32_t id_v0, int32_t id_v1, const double meas[8],
                     const double* info77, int32_t kernel, double kernel_delta) {
  try {
  if (!g || !meas) return fail(g, SIM3OPT_ERR_ARG, "add_edge: null argument");
  REFUSE_FINISHED(g);
  if (g->initialized) g->dirty = true;
  return add_edge_impl(g, id_v0, id_v1, meas, info77, kernel, kernel_delta);
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return fail(g, SIM3OPT_ERR_ARG, "add_edge: out of host memory or internal error");
  }
}

int sim3opt_add_edges(sim3opt_graph* g, int32_t m, const int32_t* id_v0, const int32_t* id_v1,
                      const double* meas, const double* info, int32_t kernel,
                      double kernel_delta) {
  try {
  if (!g || m < 0 || (m > 0 && (!id_v0 || !id_v1 || !meas)))
    return fail(g, SIM3OPT_ERR_ARG, "add_edges: bad argument");
  REFUSE_FINISHED(g);
  if (g->initialized) g->dirty = true;
  HostGraph& h = g->host;
  h.ev0.reserve(h.ev0.size() + m);
  h.ev1.reserve(h.ev1.size() + m);
  h.meas.reserve(h.meas.size() + m);
  for (int32_t k = 0; k < m; ++k) {
    const int rc = add_edge_impl(g, id_v0[k], id_v1[k], meas + 8 * (size_t)k,
                                 info ? info + 49 * (size_t)k : nullptr, kernel, kernel_delta);
    if (rc != SIM3OPT_OK) return rc;
  }
  return SIM3OPT_OK;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return fail(g, SIM3OPT_ERR_ARG, "add_edges: out of host memory or internal error");
  }
}

int sim3opt_set_edge_kernels(sim3opt_graph* g, int32_t n, const int32_t* edges, const int32_t* kinds,
                             const double* deltas) {
  try {
  if (!g) return SIM3OPT_ERR_ARG;
  if (n < 0 || (n > 0 && (!kinds || !deltas))) return fail(g, SIM3OPT_ERR_ARG, "set_edge_kernels: bad argument");
  REFUSE_FINISHED(g);
  HostGraph& h = g->host;
  const int32_t m = h.ne();
  bool any = false;
  for (int32_t i = 0; i < n; ++i) {  // the whole call is checked before anything changes
    const int32_t k = edges ? edges[i] : i;
    if (k < 0 || k >= m) return fail(g, SIM3OPT_ERR_ARG, "set_edge_kernels: edge index out of range");
    if (!kernel_ok(kinds[i], deltas[i]))
      return fail(g, SIM3OPT_ERR_ARG, "set_edge_kernels: unknown kind, or delta not finite and > 0");
    any = any || kinds[i] != SIM3OPT_KERNEL_NONE;
  }
  if (!any && !h.has_kernel) return SIM3OPT_OK;  // NONE on a kernel-free graph: nothing changes
  materialise_kernels(h);
  for (int32_t i = 0; i < n; ++i) {  // (later entries win)
    const int32_t k = edges ? edges[i] : i;
    h.kkind[k] = (uint8_t)kinds[i];
    h.kdelta[k] = kinds[i] == SIM3OPT_KERNEL_NONE ? 0.0 : deltas[i];
  }
  // an initialised graph takes the new kernels at once; a changed one gets them at its next initialize
  if (g->initialized && !g->dirty)
    return on_ranks(g, [&](Engine* e, int, std::string& err) { return engine_set_kernels(e, h, err); });
  return SIM3OPT_OK;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return fail(g, SIM3OPT_ERR_ARG, "set_edge_kernels: out of host memory or internal error");
  }
}

int sim3opt_get_edge_kernels(const sim3opt_graph* g, int32_t* kinds, double* deltas) {
  if (!g) return SIM3OPT_ERR_ARG;
  const HostGraph& h = g->host;
  for (int32_t k = 0; k < h.ne(); ++k) {
    if (kinds) kinds[k] = h.has_kernel ? (int32_t)h.kkind[k] : SIM3OPT_KERNEL_NONE;
    if (deltas) deltas[k] = h.has_kernel ? h.kdelta[k] : 0.0;
  }
  return SIM3OPT_OK;
}

int sim3opt_robustify(int32_t kind, double delta, double e2, double rho[2]) {
  if (!rho || !kernel_ok(kind, delta) || !(e2 >= 0.0)) return SIM3OPT_ERR_ARG;
  robustify(kind, delta, e2, rho[0], rho[1]);
  return SIM3OPT_OK;
}

int32_t sim3opt_num_vertices(const sim3opt_graph* g) { return g ? g->host.nv() : 0; }
int32_t sim3opt_num_edges(const sim3opt_graph* g) { return g ? g->host.ne() : 0; }

int sim3opt_get_edge(const sim3opt_graph* g, int32_t k, int32_t* id_v0, int32_t* id_v1,
                     double meas[8]) {
  try {
  if (!g || k < 0 || k >= g->host.ne()) return SIM3OPT_ERR_ARG;
  if (id_v0) *id_v0 = g->host.vid[g->host.ev0[k]];
  if (id_v1) *id_v1 = g->host.vid[g->host.ev1[k]];
  if (meas) from_sim3(g->host.meas[k], meas);
  return SIM3OPT_OK;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return SIM3OPT_ERR_ARG;
  }
}

int sim3opt_initialize(sim3opt_graph* g) {
  try {
  if (!g) return SIM3OPT_ERR_ARG;
  REFUSE_FINISHED(g);
  const bool trace = std::getenv("SIM3OPT_INIT_TRACE") != nullptr;
  auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  double t1 = t0, t2 = t0;
  if (g->initialized) {  // g2o allows re-initialisation: rebuild from the current estimates
    int rc = sync_host_states(g);
    if (rc) return rc;
    if (g->group) {  // every rank keeps its communicator (and its mailboxes) for the next engine
      g->engine = nullptr;
      rc = g->group->run([](RankCtx& c) {
        engine_take_comm(c.engine, &c.comm);
        engine_destroy(c.engine);
        c.engine = nullptr;
        return (int)SIM3OPT_OK;
      }, g->err);
      if (rc) return rc;
    } else {
    engine_take_comm(g->engine, &g->comm);  // a multi-GPU graph stays partitioned after re-init
    g->comm_set = g->comm.world > 1 || g->comm.force;
    engine_destroy(g->engine);
    g->engine = nullptr;
    }
    g->initialized = false;
    g->dirty = false;
  }
  t1 = now();
  {
    // a graph that is row-partitioned over several ranks gets its block rows in locality order
    // (contiguous rank spans are then slabs of the graph: few cut edges, a small halo); one rank
    // keeps g2o's insertion order (options.row_order overrides: tests, measurements).
    apply_env_overrides(g->opt);
    const bool local = g->opt.row_order >= 0 ? g->opt.row_order == 1 : (g->group || (g->comm_set && g->comm.world > 1));
    std::vector<int32_t> order;
    if (local) locality_order(g->host, order);
    if (!build_structure(g->host, g->structure, g->err, local ? &order : nullptr)) return SIM3OPT_ERR_STATE;
  }
  t2 = now();
  int status = SIM3OPT_OK;
  if (g->group) {  // the host graph and the structure are shared, read-only; every rank builds its own share
    status = g->group->run([&](RankCtx& c) {
      if (!c.connected) {
        const int rc = comm_local_connect(c.comm, c.err);
        if (rc) return rc;
        c.connected = true;
      }
      sim3opt_options o = g->opt;
      o.device = c.device;
      int st = SIM3OPT_OK;
      c.engine = engine_create(g->host, g->structure, o, &c.comm, c.err, st);
      return c.engine ? (int)SIM3OPT_OK : st;
    }, g->err);
    g->engine = status == SIM3OPT_OK ? g->group->ctx(0).engine : nullptr;
  } else
  g->engine = engine_create(g->host, g->structure, g->opt, g->comm_set ? &g->comm : nullptr,
                            g->err, status);
  if (trace)
    std::fprintf(stderr, "sim3opt_initialize: tear-down %.2f ms, structure %.2f ms, engine %.2f ms\n", t1 - t0, t2 - t1,
                 now() - t2);
  g->comm_set = false;
  if (!g->engine) return status;
  g->initialized = true;
  return SIM3OPT_OK;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return fail(g, SIM3OPT_ERR_ARG, "initialize: out of host memory or internal error");
  }
}

int sim3opt_optimize(sim3opt_graph* g, int32_t max_iters) {
  try {
  if (!g) return 0;
  if (finished(g)) { g->err = FINISHED; return 0; }
  if (!g->initialized) {
    // g2o: optimize() on an uninitialised / empty problem returns -1
    if (g->host.ne() == 0 || g->host.nv() == 0) { g->err = "optimize: nothing to optimise"; return -1; }
    g->err = "optimize: call sim3opt_initialize first";
    return 0;
  }
  if (max_iters <= 0) return 0;
  if (g->dirty) { g->err = "optimize: graph changed, call sim3opt_initialize again"; return 0; }
  g->last_algorithm = g->opt.algorithm;
  if (g->group) {
    const int rc = g->group->run([&](RankCtx& c) {
      const int it = engine_optimize(c.engine, max_iters, c.stats, c.err);
      engine_trust_region_stats(c.engine, c.tr_stats);
      return it;
    }, g->err);
    g->stats = g->group->ctx(0).stats;
    g->tr_stats = g->group->ctx(0).tr_stats;
    return rc < 0 ? 0 : rc;
  }
  const int rc = engine_optimize(g->engine, max_iters, g->stats, g->err);
  engine_trust_region_stats(g->engine, g->tr_stats);
  return rc < 0 ? 0 : rc;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    (void)fail(g, SIM3OPT_ERR_ARG, "optimize: out of host memory or internal error"); return 0;
  }
}

int sim3opt_get_vertex(sim3opt_graph* g, int32_t id, double state[8]) {
  if (!g || !state) return fail(g, SIM3OPT_ERR_ARG, "get_vertex: null argument");
  REFUSE_FINISHED(g);
  auto it = g->host.id2idx.find(id);
  if (it == g->host.id2idx.end()) return fail(g, SIM3OPT_ERR_ARG, "get_vertex: unknown id");
  int rc = sync_host_states(g);
  if (rc) return rc;
  from_sim3(g->host.states[it->second], state);
  return SIM3OPT_OK;
}

int sim3opt_set_vertex(sim3opt_graph* g, int32_t id, const double state[8]) {
  if (!g || !state) return fail(g, SIM3OPT_ERR_ARG, "set_vertex: null argument");
  REFUSE_FINISHED(g);
  auto it = g->host.id2idx.find(id);
  if (it == g->host.id2idx.end()) return fail(g, SIM3OPT_ERR_ARG, "set_vertex: unknown id");
  if (!state_ok(state)) return fail(g, SIM3OPT_ERR_ARG, "set_vertex: non-finite state or scale <= 0");
  int rc = sync_host_states(g);
  if (rc) return rc;
  g->host.states[it->second] = to_sim3(state);
  if (g->initialized) return push_host_states(g);
  return SIM3OPT_OK;
}

int sim3opt_get_vertices(sim3opt_graph* g, double* states) {
  if (!g || !states) return fail(g, SIM3OPT_ERR_ARG, "get_vertices: null argument");
  REFUSE_FINISHED(g);
  int rc = sync_host_states(g);
  if (rc) return rc;
  for (size_t k = 0; k < g->host.states.size(); ++k) from_sim3(g->host.states[k], states + 8 * k);
  return SIM3OPT_OK;
}

int sim3opt_set_vertices(sim3opt_graph* g, const double* states) {
  if (!g || !states) return fail(g, SIM3OPT_ERR_ARG, "set_vertices: null argument");
  REFUSE_FINISHED(g);
  for (size_t k = 0; k < g->host.states.size(); ++k)
    if (!state_ok(states + 8 * k)) return fail(g, SIM3OPT_ERR_ARG, "set_vertices: bad state");
  for (size_t k = 0; k < g->host.states.size(); ++k) g->host.states[k] = to_sim3(states + 8 * k);
  if (g->initialized) return push_host_states(g);
  return SIM3OPT_OK;
}

int sim3opt_chi2(sim3opt_graph* g, double* chi2) {
  if (!g || !chi2) return fail(g, SIM3OPT_ERR_ARG, "chi2: null argument");
  REFUSE_FINISHED(g);
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "chi2: call sim3opt_initialize first");
  return on_ranks(g, [&](Engine* e, int rank, std::string& err) {
    double other = 0.0;  // (every rank computes the same sum)
    return engine_chi2(e, rank == 0 ? chi2 : &other, err);
  });
}

int32_t sim3opt_num_iterations(const sim3opt_graph* g) { return g ? (int32_t)g->stats.size() : 0; }

int sim3opt_get_stats(const sim3opt_graph* g, int32_t iter, sim3opt_iter_stats* out) {
  if (!g || !out || iter < 0 || iter >= (int32_t)g->stats.size()) return SIM3OPT_ERR_ARG;
  *out = g->stats[iter];
  return SIM3OPT_OK;
}

int sim3opt_get_trust_region_stats(const sim3opt_graph* g, int32_t iter, sim3opt_tr_stats* out) {
  if (!g || !out) return SIM3OPT_ERR_ARG;
  if (g->last_algorithm != SIM3OPT_ALGORITHM_DOGLEG) return SIM3OPT_ERR_STATE;
  if (iter < 0 || iter >= (int32_t)g->tr_stats.size()) return SIM3OPT_ERR_ARG;
  *out = g->tr_stats[iter];
  return SIM3OPT_OK;
}

int sim3opt_get_kernel_times(sim3opt_graph* g, sim3opt_kernel_times* out) {
  if (!g || !out) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return fail(g, SIM3OPT_ERR_STATE, "kernel_times: not initialized");
  return engine_kernel_times(g->engine, out, false);
}

int sim3opt_get_comm_times(sim3opt_graph* g, sim3opt_comm_times* out) {
  if (!g || !out) return SIM3OPT_ERR_ARG;
  REFUSE_FINISHED(g);
  if (!g->initialized) return fail(g, SIM3OPT_ERR_STATE, "comm_times: not initialized");
  return on_ranks(g, [&](Engine* e, int, std::string&) { return engine_comm_times(e, out); }, false);
}

int sim3opt_reset_kernel_times(sim3opt_graph* g) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return fail(g, SIM3OPT_ERR_STATE, "kernel_times: not initialized");
  for_engines(g, [](Engine* e) { (void)engine_kernel_times(e, nullptr, true); });
  return SIM3OPT_OK;
}

int sim3opt_pcg_schedule_stats(sim3opt_graph* g, int64_t out[4], int32_t reset) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return fail(g, SIM3OPT_ERR_STATE, "pcg_schedule_stats: not initialized");
  engine_pcg_schedule_stats(g->engine, out, reset != 0);
  if (g->group && reset)
    for (int32_t r = 1; r < g->group->size(); ++r) engine_pcg_schedule_stats(g->group->ctx(r).engine, nullptr, true);
  return SIM3OPT_OK;
}

int sim3opt_edge_errors(sim3opt_graph* g, double* e_out) {
  if (!g || !e_out) return fail(g, SIM3OPT_ERR_ARG, "edge_errors: null argument");
  REFUSE_FINISHED(g);
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "edge_errors: call sim3opt_initialize first");
  return on_ranks(g, [&](Engine* e, int, std::string& err) { return engine_edge_errors(e, e_out, err); }, false);
}

int sim3opt_edge_chi2(sim3opt_graph* g, double* chi2, double* rho, double* weight) {
  if (!g) return SIM3OPT_ERR_ARG;
  REFUSE_FINISHED(g);
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "edge_chi2: call sim3opt_initialize first");
  return on_ranks(g, [&](Engine* e, int, std::string& err) { return engine_edge_chi2(e, chi2, rho, weight, err); },
                  false);
}

int sim3opt_edge_jacobians(sim3opt_graph* g, double* e_out, double* J_out) {
  if (!g || !e_out || !J_out) return fail(g, SIM3OPT_ERR_ARG, "edge_jacobians: null argument");
  if (g->opt.fix_small_angle_b != 1)
    return fail(g, SIM3OPT_ERR_ARG, "edge_jacobians: needs fix_small_angle_b = 1 (closed form of the exact map)");
  if (!g->initialized || g->dirty)
    return fail(g, SIM3OPT_ERR_STATE, "edge_jacobians: call sim3opt_initialize first");
  REFUSE_FINISHED(g);
  return on_ranks(g, [&](Engine* e, int, std::string& err) { return engine_edge_jacobians(e, e_out, J_out, err); },
                  false);
}

int sim3opt_sim3_edge_jacobian(const double meas[8], const double s0[8], const double s1[8],
                               const sim3opt_options* o, double e[7], double J[98]) {
  if (!meas || !s0 || !s1 || !e || !J) return SIM3OPT_ERR_ARG;
  if (!state_ok(meas) || !state_ok(s0) || !state_ok(s1)) return SIM3OPT_ERR_ARG;
  sim3opt_options d;
  if (!o) {
    sim3opt_options_default(&d);
    o = &d;
  }
  if (o->fix_small_angle_b != 1 || !(o->exp_eps > 0)) return SIM3OPT_ERR_ARG;
  const sim3::Opts mo{o->exp_eps, o->small_rot_half, o->fix_small_angle_b};
  sim3::edge_jacobians(to_sim3(meas), to_sim3(s0), to_sim3(s1), mo, o->dof_mask, e, J);
  return SIM3OPT_OK;
}

int sim3opt_linearize(sim3opt_graph* g) {
  if (!g) return SIM3OPT_ERR_ARG;
  REFUSE_FINISHED(g);
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "linearize: call sim3opt_initialize first");
  return on_ranks(g, [&](Engine* e, int, std::string& err) { return engine_linearize(e, err); });
}

int sim3opt_debug_linearization_dims(sim3opt_graph* g, int32_t* n_active, int32_t* n_incidences) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!n_active || !n_incidences) return fail(g, SIM3OPT_ERR_ARG, "debug_linearization_dims: null argument");
  if (!g->initialized || g->dirty)
    return fail(g, SIM3OPT_ERR_STATE, "debug_linearization_dims: call sim3opt_initialize first");
  engine_debug_linearization_dims(g->engine, n_active, n_incidences);
  return SIM3OPT_OK;
}

int sim3opt_debug_linearization(sim3opt_graph* g, double* J, double* w, int32_t* active, double* scratch,
                                int32_t* incptr, int32_t* inc0, int32_t* inc1, int32_t* slot01, int32_t* slot10,
                                double* trace, double* maxdiag) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!J || !w || !active || !scratch || !incptr || !inc0 || !inc1 || !slot01 || !slot10 || !trace || !maxdiag)
    return fail(g, SIM3OPT_ERR_ARG, "debug_linearization: null argument");
  if (!g->initialized || g->dirty)
    return fail(g, SIM3OPT_ERR_STATE, "debug_linearization: call sim3opt_initialize first");
  REFUSE_RANKS(g, "debug_linearization");
  return engine_debug_linearization(g->engine, J, w, active, scratch, incptr, inc0, inc1, slot01, slot10, trace,
                                    maxdiag, g->err);
}

int sim3opt_debug_update(sim3opt_graph* g, const double* x, double lambda, int32_t with_fail, int32_t grid,
                         double* states_out, double* backup_out, double* chi2, double* scale) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!x) return fail(g, SIM3OPT_ERR_ARG, "debug_update: null step");
  if (!states_out && !backup_out && !chi2 && !scale) return fail(g, SIM3OPT_ERR_ARG, "debug_update: every output is null");
  if (!std::isfinite(lambda)) return fail(g, SIM3OPT_ERR_ARG, "debug_update: lambda is not finite");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "debug_update: call sim3opt_initialize first");
  REFUSE_RANKS(g, "debug_update");
  return engine_debug_update(g->engine, x, lambda, with_fail != 0, grid, states_out, backup_out, chi2, scale, g->err);
}

int sim3opt_debug_dogleg(sim3opt_graph* g, const double* h_gn, double ca, double cg, int32_t with_fail, int32_t grid,
                         int64_t j0, int64_t j1, double* scalars, double* states_out, double* backup_out) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!h_gn) return fail(g, SIM3OPT_ERR_ARG, "debug_dogleg: null h_gn");
  if (!scalars && !states_out && !backup_out) return fail(g, SIM3OPT_ERR_ARG, "debug_dogleg: every output is null");
  if (!std::isfinite(ca) || !std::isfinite(cg)) return fail(g, SIM3OPT_ERR_ARG, "debug_dogleg: a coefficient is not finite");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "debug_dogleg: call sim3opt_initialize first");
  REFUSE_RANKS(g, "debug_dogleg");
  return engine_debug_dogleg(g->engine, h_gn, ca, cg, with_fail != 0, grid, j0, j1, scalars, states_out, backup_out,
                             g->err);
}

int sim3opt_dogleg_rule(const double scalars[6], double delta, double model[3], double trial[4], int32_t* step) {
  if (!scalars || !model || !trial || !step) return SIM3OPT_ERR_ARG;
  engine_dogleg_rule(scalars, delta, model, trial, step);
  return SIM3OPT_OK;
}

int sim3opt_debug_column_vectors(sim3opt_graph* g, int32_t kernel, int32_t grid, int64_t n, int32_t K, const int64_t* at,
                                 int32_t system, const double* a, const double* b, int32_t first, int32_t count,
                                 int32_t col, const int32_t* rows, int32_t n_blocks, double* out) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!out) return fail(g, SIM3OPT_ERR_ARG, "debug_column_vectors: null output");
  if (!g->initialized || g->dirty)
    return fail(g, SIM3OPT_ERR_STATE, "debug_column_vectors: call sim3opt_initialize first");
  REFUSE_RANKS(g, "debug_column_vectors");
  return engine_debug_column_vectors(g->engine, kernel, grid, n, K, at, system, a, b, first, count, col, rows, n_blocks,
                                     out, g->err);
}

int sim3opt_debug_factor_dims(sim3opt_graph* g, int32_t context, int32_t* n_block_rows, int64_t* n_blocks_L,
                              int64_t* n_blocks) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!n_block_rows || !n_blocks_L || !n_blocks) return fail(g, SIM3OPT_ERR_ARG, "debug_factor_dims: null argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "debug_factor_dims: call sim3opt_initialize first");
  REFUSE_RANKS(g, "debug_factor_dims");
  return engine_debug_factor_dims(g->engine, context, n_block_rows, n_blocks_L, n_blocks, g->err);
}

int sim3opt_debug_factor(sim3opt_graph* g, int32_t context, double lambda, const double* vals, const double* b,
                         int32_t with_solve, int32_t with_selinv, double* Aperm, double* bp, double* L, double* Dinv,
                         double* y, double* xp, double* x, int32_t* fail_word, double* Z, int32_t* singular,
                         int32_t* bord, int32_t* brow) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!Aperm || !bp || !L || !Dinv || !y || !fail_word || (with_solve && (!xp || !x)) ||
      (with_selinv && (!Z || !singular)))
    return fail(g, SIM3OPT_ERR_ARG, "debug_factor: null argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "debug_factor: call sim3opt_initialize first");
  REFUSE_RANKS(g, "debug_factor");
  return engine_debug_factor(g->engine, context, lambda, vals, b, with_solve != 0, with_selinv != 0, Aperm, bp, L, Dinv,
                             y, xp, x, fail_word, Z, singular, bord, brow, g->err);
}

int sim3opt_system_dims(const sim3opt_graph* g, int32_t* n_block_rows, int64_t* n_blocks) {
  if (!g || !g->initialized) return SIM3OPT_ERR_STATE;
  if (n_block_rows) *n_block_rows = g->structure.nb;
  if (n_blocks) *n_blocks = g->structure.nnzb;
  return SIM3OPT_OK;
}

int sim3opt_system_pattern(sim3opt_graph* g, int32_t* n_block_rows, int64_t* n_blocks,
                           int32_t* rowptr, int32_t* colidx) {
  try {
  if (!g) return SIM3OPT_ERR_ARG;
  Structure st;
  if (!build_structure(g->host, st, g->err)) return SIM3OPT_ERR_STATE;
  if (n_block_rows) *n_block_rows = st.nb;
  if (n_blocks) *n_blocks = st.nnzb;
  if (rowptr) std::memcpy(rowptr, st.rowptr.data(), sizeof(int32_t) * (size_t)(st.nb + 1));
  if (colidx) std::memcpy(colidx, st.colidx.data(), sizeof(int32_t) * (size_t)st.nnzb);
  return SIM3OPT_OK;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return fail(g, SIM3OPT_ERR_ARG, "system_pattern: out of host memory or internal error");
  }
}

int sim3opt_get_system(sim3opt_graph* g, int32_t* rowptr, int32_t* colidx, double* values,
                       double* b) {
  if (!g) return SIM3OPT_ERR_ARG;
  REFUSE_FINISHED(g);
  if (!g->initialized) return fail(g, SIM3OPT_ERR_STATE, "get_system: call sim3opt_initialize first");
  // (rank 0's rows, as a rank of a graph partitioned over processes answers)
  return on_ranks(g, [&](Engine* e, int, std::string& err) { return engine_get_system(e, rowptr, colidx, values, b, err); },
                  false);
}

int sim3opt_solve(sim3opt_graph* g, double lambda, double* x, int32_t* iters, double* rel_res) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return fail(g, SIM3OPT_ERR_STATE, "solve: call sim3opt_initialize first");
  REFUSE_RANKS(g, "solve");
  return engine_solve(g->engine, lambda, x, iters, rel_res, g->err);
}

int sim3opt_bench_spmv(sim3opt_graph* g, int32_t reps, double* ms_mean) {
  if (!g || !ms_mean || reps < 1) return fail(g, SIM3OPT_ERR_ARG, "bench_spmv: bad argument");
  if (!g->initialized) return fail(g, SIM3OPT_ERR_STATE, "bench_spmv: call sim3opt_initialize first");
  REFUSE_RANKS(g, "bench_spmv");
  return engine_bench_spmv(g->engine, reps, ms_mean, g->err);
}

int sim3opt_preconditioner_in_use(const sim3opt_graph* g) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return SIM3OPT_ERR_STATE;
  return engine_preconditioner(g->engine);
}

int sim3opt_amg_in_use(const sim3opt_graph* g, int32_t* n_levels, int32_t* n_partitioned, int32_t visits[4]) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return SIM3OPT_ERR_STATE;
  engine_amg_in_use(g->engine, n_levels, n_partitioned, visits);
  return SIM3OPT_OK;
}

int sim3opt_device_bytes(const sim3opt_graph* g, int64_t bytes[2]) {
  if (!g || !bytes) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return SIM3OPT_ERR_STATE;
  engine_device_bytes(g->engine, bytes);
  return SIM3OPT_OK;
}

int sim3opt_linear_solver_in_use(const sim3opt_graph* g) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return SIM3OPT_ERR_STATE;
  return engine_linear_solver(g->engine);
}

int sim3opt_direct_plan(sim3opt_graph* g, int64_t max_pairs, int64_t dims[8], int32_t* perm,
                        int32_t* colptr, int32_t* lrow, int32_t* srcptr, int32_t* src,
                        int32_t* pairptr, int32_t* pa, int32_t* pb, int32_t* gptr, int32_t* lcolp,
                        int32_t* rptr, int32_t* cells) {
  try {
  if (!g || !dims) return fail(g, SIM3OPT_ERR_ARG, "direct_plan: bad argument");
  Structure st;
  if (!build_structure(g->host, st, g->err)) return SIM3OPT_ERR_STATE;
  DirectPlan P;
  std::string why;
  if (!build_direct_plan(st.nb, st.rowptr.data(), st.colidx.data(), max_pairs > 0 ? max_pairs : 300000, 0,
                         P, why)) {
    g->err = "direct_plan: " + why;
    return SIM3OPT_ERR_STATE;
  }
  dims[0] = P.nb; dims[1] = P.nL; dims[2] = P.npairs; dims[3] = P.height; dims[4] = P.ngroups();
  dims[5] = (int64_t)P.lcolp.size() - 1; dims[6] = (int64_t)P.src.size();
  dims[7] = (int64_t)P.cells.size() / DirectPlan::CELL_STRIDE;
  auto out = [](int32_t* dst, const std::vector<int32_t>& v) {
    if (dst && !v.empty()) std::memcpy(dst, v.data(), sizeof(int32_t) * v.size());
  };
  out(perm, P.perm); out(colptr, P.colptr); out(lrow, P.lrow); out(srcptr, P.srcptr); out(src, P.src);
  out(pairptr, P.pairptr); out(pa, P.pa); out(pb, P.pb); out(gptr, P.gptr); out(lcolp, P.lcolp);
  out(rptr, P.rptr); out(cells, P.cells);
  return SIM3OPT_OK;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return fail(g, SIM3OPT_ERR_ARG, "direct_plan: out of host memory or internal error");
  }
}

int sim3opt_marginals(sim3opt_graph* g, double lambda, int32_t n, const int32_t* id_a,
                      const int32_t* id_b, double* cov) {
  try {
  if (!g || n < 0 || (n > 0 && (!id_a || !id_b || !cov))) return fail(g, SIM3OPT_ERR_ARG, "marginals: bad argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "marginals: call sim3opt_initialize first");
  REFUSE_RANKS(g, "marginals");
  std::vector<int32_t> ra(std::max(n, 1)), rb(std::max(n, 1));
  for (int32_t q = 0; q < n; ++q) {
    const auto a = g->host.id2idx.find(id_a[q]), b = g->host.id2idx.find(id_b[q]);
    if (a == g->host.id2idx.end() || b == g->host.id2idx.end()) return fail(g, SIM3OPT_ERR_ARG, "marginals: unknown vertex id");
    ra[q] = g->structure.hidx[a->second];
    rb[q] = g->structure.hidx[b->second];
    if (ra[q] < 0 || rb[q] < 0) return fail(g, SIM3OPT_ERR_ARG, "marginals: fixed vertex in a pair");
  }
  return engine_marginals(g->engine, lambda, n, ra.data(), rb.data(), cov, g->err);
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "marginals: out of host memory or internal error");
  }
}

// a column call that failed on one column names the vertex by its position; the caller knows it by its id
static int name_failed_column(sim3opt_graph* g, int rc) {
  if (rc != SIM3OPT_ERR_STATE || g->opt.cov_solver == 0) return rc;
  int64_t counts[5];
  double res[2];
  int32_t v = -1;
  engine_covariance_columns_stats(g->engine, counts, res, &v);
  if (v >= 0 && v < g->host.nv()) g->err += " [vertex id " + std::to_string(g->host.vid[v]) + "]";
  return rc;
}

int sim3opt_covariances(sim3opt_graph* g, double lambda, int32_t n, const int32_t* id_a,
                        const int32_t* id_b, double* cov) {
  try {
  if (!g || n < 0 || (n > 0 && (!id_a || !id_b || !cov))) return fail(g, SIM3OPT_ERR_ARG, "covariances: bad argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "covariances: call sim3opt_initialize first");
  REFUSE_RANKS(g, "covariances");
  std::vector<int32_t> ra(std::max(n, 1)), rb(std::max(n, 1));
  for (int32_t q = 0; q < n; ++q) {
    const auto a = g->host.id2idx.find(id_a[q]), b = g->host.id2idx.find(id_b[q]);
    if (a == g->host.id2idx.end() || b == g->host.id2idx.end()) return fail(g, SIM3OPT_ERR_ARG, "covariances: unknown vertex id");
    ra[q] = g->structure.hidx[a->second];
    rb[q] = g->structure.hidx[b->second];
    if (ra[q] < 0 || rb[q] < 0) return fail(g, SIM3OPT_ERR_ARG, "covariances: fixed vertex in a pair");
  }
  return name_failed_column(g, engine_covariances(g->engine, lambda, n, ra.data(), rb.data(), cov, g->err));
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "covariances: out of host memory or internal error");
  }
}

int sim3opt_covariance_stats(const sim3opt_graph* g, int64_t out[6]) {
  if (!g || !out) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return SIM3OPT_ERR_STATE;
  engine_covariance_stats(g->engine, out);
  return SIM3OPT_OK;
}

int sim3opt_covariance_columns_stats(const sim3opt_graph* g, int64_t counts[5], double res[2]) {
  if (!g || !counts || !res) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return SIM3OPT_ERR_STATE;
  engine_covariance_columns_stats(g->engine, counts, res, nullptr);
  return SIM3OPT_OK;
}

int sim3opt_covariance_columns_plan(sim3opt_graph* g, int32_t n, const int32_t* id_a, const int32_t* id_b,
                                    int32_t* n_vertices, int32_t* vertices) {
  try {
  if (!g || n < 0 || !n_vertices || (n > 0 && (!id_a || !id_b)))
    return fail(g, SIM3OPT_ERR_ARG, "covariance_columns_plan: bad argument");
  Structure st;
  if (!build_structure(g->host, st, g->err)) return SIM3OPT_ERR_STATE;
  std::vector<int32_t> ra(std::max(n, 1)), rb(std::max(n, 1));
  for (int32_t q = 0; q < n; ++q) {
    const auto a = g->host.id2idx.find(id_a[q]), b = g->host.id2idx.find(id_b[q]);
    if (a == g->host.id2idx.end() || b == g->host.id2idx.end())
      return fail(g, SIM3OPT_ERR_ARG, "covariance_columns_plan: unknown vertex id");
    ra[q] = st.hidx[a->second];
    rb[q] = st.hidx[b->second];
    if (ra[q] < 0 || rb[q] < 0) return fail(g, SIM3OPT_ERR_ARG, "covariance_columns_plan: fixed vertex in a pair");
  }
  ColumnCover C;
  covariance_columns_cover(st.nb, n, ra.data(), rb.data(), C);
  *n_vertices = (int32_t)C.chosen.size();
  if (vertices)
    for (size_t k = 0; k < C.chosen.size(); ++k) vertices[k] = g->host.vid[st.row2vertex[C.chosen[k]]];
  return SIM3OPT_OK;
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "covariance_columns_plan: out of host memory or internal error");
  }
}

int sim3opt_gate_edges(sim3opt_graph* g, double lambda, int32_t n, const int32_t* id_v0, const int32_t* id_v1,
                       const double* meas, const double* info, double* e, double* S, double* d2) {
  try {
  if (!g || n < 0 || (n > 0 && (!id_v0 || !id_v1 || !meas || !e || !S || !d2)))
    return fail(g, SIM3OPT_ERR_ARG, "gate_edges: bad argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "gate_edges: call sim3opt_initialize first");
  REFUSE_RANKS(g, "gate_edges");
  const size_t m = (size_t)std::max(n, 1);
  std::vector<int32_t> v0(m), v1(m), r0(m), r1(m);
  std::vector<sim3::Sim3> cm(m);
  std::vector<double> oi(49 * m, 0.0);
  for (int32_t q = 0; q < n; ++q) {
    const auto a = g->host.id2idx.find(id_v0[q]), b = g->host.id2idx.find(id_v1[q]);
    if (a == g->host.id2idx.end() || b == g->host.id2idx.end()) return fail(g, SIM3OPT_ERR_ARG, "gate_edges: unknown vertex id");
    if (a->second == b->second) return fail(g, SIM3OPT_ERR_ARG, "gate_edges: identical endpoints");
    if (!state_ok(meas + 8 * (size_t)q)) return fail(g, SIM3OPT_ERR_ARG, "gate_edges: non-finite measurement or scale <= 0");
    v0[q] = a->second; v1[q] = b->second;
    r0[q] = g->structure.hidx[a->second]; r1[q] = g->structure.hidx[b->second];
    cm[q] = to_sim3(meas + 8 * (size_t)q);
    double* W = &oi[49 * (size_t)q];  // Omega^-1, column-major
    if (!info) {
      for (int d = 0; d < 7; ++d) W[8 * d] = 1.0;
      continue;
    }
    // Omega = L L^T (symmetric, positive definite: else refused), Omega^-1 = L^-T L^-1
    const double* Om = info + 49 * (size_t)q;
    double Lc[7][7] = {}, Li[7][7] = {};
    double amax = 0.0;
    for (int k = 0; k < 49; ++k) {
      if (!std::isfinite(Om[k])) return fail(g, SIM3OPT_ERR_ARG, "gate_edges: non-finite information matrix");
      amax = std::max(amax, std::fabs(Om[k]));
    }
    for (int c = 0; c < 7; ++c)
      for (int r = 0; r < c; ++r)
        if (std::fabs(Om[r + 7 * c] - Om[c + 7 * r]) > 1e-12 * amax)
          return fail(g, SIM3OPT_ERR_ARG, "gate_edges: information matrix is not symmetric");
    for (int j = 0; j < 7; ++j) {
      double d = Om[8 * j];
      for (int k = 0; k < j; ++k) d -= Lc[j][k] * Lc[j][k];
      if (!(d > 0.0)) return fail(g, SIM3OPT_ERR_ARG, "gate_edges: information matrix is not positive definite");
      Lc[j][j] = std::sqrt(d);
      for (int r = j + 1; r < 7; ++r) {
        double v = Om[r + 7 * j];
        for (int k = 0; k < j; ++k) v -= Lc[r][k] * Lc[j][k];
        Lc[r][j] = v / Lc[j][j];
      }
    }
    for (int c = 0; c < 7; ++c)
      for (int r = c; r < 7; ++r) {
        double v = r == c ? 1.0 : 0.0;
        for (int k = c; k < r; ++k) v -= Lc[r][k] * Li[k][c];
        Li[r][c] = v / Lc[r][r];
      }
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c <= r; ++c) {
        double v = 0.0;
        for (int k = r; k < 7; ++k) v += Li[k][r] * Li[k][c];
        W[r + 7 * c] = v;
        W[c + 7 * r] = v;
      }
  }
  return name_failed_column(g, engine_gate_edges(g->engine, lambda, n, v0.data(), v1.data(), r0.data(), r1.data(),
                                                 cm.data(), oi.data(), e, S, d2, g->err));
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "gate_edges: out of host memory or internal error");
  }
}

int sim3opt_marginal_covariances(sim3opt_graph* g, double lambda, double* cov) {
  try {
  if (!g || !cov) return fail(g, SIM3OPT_ERR_ARG, "marginal_covariances: bad argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "marginal_covariances: call sim3opt_initialize first");
  REFUSE_RANKS(g, "marginal_covariances");
  std::vector<int32_t> rows;  // free vertices in insertion order
  for (int32_t v = 0; v < g->host.nv(); ++v)
    if (g->structure.hidx[v] >= 0) rows.push_back(g->structure.hidx[v]);
  return engine_marginals(g->engine, lambda, (int32_t)rows.size(), rows.data(), rows.data(), cov, g->err);
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "marginal_covariances: out of host memory or internal error");
  }
}

int sim3opt_marginal_plan(sim3opt_graph* g, int64_t max_pairs, int64_t dims[6], int32_t* perm,
                          int32_t* colptr, int32_t* lrow, int32_t* gptr, int32_t* lcolp, int32_t* zptr,
                          int32_t* za, int32_t* zt, int32_t* zl) {
  try {
  if (!g || !dims) return fail(g, SIM3OPT_ERR_ARG, "marginal_plan: bad argument");
  Structure st;
  if (!build_structure(g->host, st, g->err)) return SIM3OPT_ERR_STATE;
  DirectPlan P;
  SelinvPlan S;
  std::string why;
  if (!build_direct_plan(st.nb, st.rowptr.data(), st.colidx.data(), max_pairs > 0 ? max_pairs : 30000000, 0, P, why) ||
      !build_selinv_plan(P, S, why)) {
    g->err = "marginal_plan: " + why;
    return SIM3OPT_ERR_STATE;
  }
  dims[0] = P.nb; dims[1] = P.nL; dims[2] = S.nprod; dims[3] = P.height; dims[4] = P.ngroups();
  dims[5] = (int64_t)P.lcolp.size() - 1;
  auto out = [](int32_t* dst, const std::vector<int32_t>& v) {
    if (dst && !v.empty()) std::memcpy(dst, v.data(), sizeof(int32_t) * v.size());
  };
  out(perm, P.perm); out(colptr, P.colptr); out(lrow, P.lrow); out(gptr, P.gptr); out(lcolp, P.lcolp);
  out(zptr, S.zptr); out(za, S.za); out(zt, S.zt); out(zl, S.zl);
  return SIM3OPT_OK;
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "marginal_plan: out of host memory or internal error");
  }
}

// the hierarchy sim3opt_initialize would build on ONE rank with the handle's options: row order, matching passes,
// dense-level cap and, with amg_virtual_ranks, the aggregation of an N-rank partition (host only)
static int host_hierarchy(sim3opt_graph* g, const char* who, Structure& st, std::vector<AmgLevelHost>& levels) {
  sim3opt_options o = g->opt;
  apply_env_overrides(o);
  std::vector<int32_t> order;
  if (o.row_order == 1) locality_order(g->host, order);
  if (!build_structure(g->host, st, g->err, o.row_order == 1 ? &order : nullptr)) return SIM3OPT_ERR_STATE;
  std::string why;
  AmgBuildOptions bo;
  bo.max_coarsest = o.amg_coarsest;
  for (int k = 0; k < 3; ++k) bo.passes[k] = o.amg_passes[k];
  std::vector<int32_t> vbegin;
  if (o.amg_virtual_ranks > 1) {
    bo.world = o.amg_virtual_ranks;
    bo.shard_rows = std::max(1, o.amg_shard_rows);
    vbegin.resize(bo.world + 1);
    partition_rows_equal(st.nb, bo.world, vbegin.data());
    bo.row_begin = vbegin.data();
  }
  if (!build_amg_hierarchy(st.nb, st.rowptr.data(), st.colidx.data(), levels, why, bo)) {
    g->err = std::string(who) + ": " + why;
    return SIM3OPT_ERR_STATE;
  }
  return SIM3OPT_OK;
}

int sim3opt_amg_hierarchy(sim3opt_graph* g, int32_t capacity, int32_t* n_levels, int32_t* rows,
                          int64_t* blocks, int32_t* aggregate_of_row) {
  try {
  if (!g || !n_levels || capacity < 0) return fail(g, SIM3OPT_ERR_ARG, "amg_hierarchy: bad argument");
  Structure st;
  std::vector<AmgLevelHost> levels;
  const int rc = host_hierarchy(g, "amg_hierarchy", st, levels);
  if (rc) return rc;
  *n_levels = (int32_t)levels.size();
  for (int32_t l = 0; l < *n_levels && l < capacity; ++l) {
    if (rows) rows[l] = levels[l].nb;
    if (blocks) blocks[l] = levels[l].nnzb;
  }
  if (aggregate_of_row) std::memcpy(aggregate_of_row, levels[0].agg.data(), sizeof(int32_t) * (size_t)st.nb);
  return SIM3OPT_OK;
  } catch (...) {  // (std::bad_alloc, std::length_error ...: nothing crosses the C boundary)
    return fail(g, SIM3OPT_ERR_ARG, "amg_hierarchy: out of host memory or internal error");
  }
}

int sim3opt_amg_level_structure(sim3opt_graph* g, int32_t level, int32_t* n_levels, int32_t* n_block_rows,
                                int64_t* n_blocks, int32_t* rowptr, int32_t* colidx, int32_t* aggregate_of_row) {
  try {
  if (!g || level < 0) return fail(g, SIM3OPT_ERR_ARG, "amg_level_structure: bad argument");
  Structure st;
  std::vector<AmgLevelHost> levels;
  const int rc = host_hierarchy(g, "amg_level_structure", st, levels);
  if (rc) return rc;
  if (n_levels) *n_levels = (int32_t)levels.size();
  if (level >= (int32_t)levels.size()) return fail(g, SIM3OPT_ERR_ARG, "amg_level_structure: no such level");
  const AmgLevelHost& L = levels[level];
  if (n_block_rows) *n_block_rows = L.nb;
  if (n_blocks) *n_blocks = L.nnzb;
  const int32_t* rp = level == 0 ? st.rowptr.data() : L.rowptr.data();
  const int32_t* ci = level == 0 ? st.colidx.data() : L.colidx.data();
  if (rowptr) std::memcpy(rowptr, rp, sizeof(int32_t) * (size_t)(L.nb + 1));
  if (colidx) std::memcpy(colidx, ci, sizeof(int32_t) * (size_t)L.nnzb);
  if (aggregate_of_row && !L.agg.empty()) std::memcpy(aggregate_of_row, L.agg.data(), sizeof(int32_t) * (size_t)L.nb);
  return SIM3OPT_OK;
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "amg_level_structure: out of host memory or internal error");
  }
}

int sim3opt_amg_level_numbers(sim3opt_graph* g, double lambda, int32_t level, int32_t* rowptr, int32_t* colidx,
                              double* values, float* values32, double* W, double* diagH, double* Minv, double* P) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "amg_level_numbers: call sim3opt_initialize first");
  if (!std::isfinite(lambda) || lambda < 0.0) return fail(g, SIM3OPT_ERR_ARG, "amg_level_numbers: bad lambda");
  REFUSE_RANKS(g, "amg_level_numbers");
  return engine_amg_level_numbers(g->engine, lambda, level, rowptr, colidx, values, values32, W, diagH, Minv, P, g->err);
}

int sim3opt_amg_coarsest_inverse(sim3opt_graph* g, double lambda, double* Ainv) {
  if (!g || !Ainv) return fail(g, SIM3OPT_ERR_ARG, "amg_coarsest_inverse: null argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "amg_coarsest_inverse: call sim3opt_initialize first");
  if (!std::isfinite(lambda) || lambda < 0.0) return fail(g, SIM3OPT_ERR_ARG, "amg_coarsest_inverse: bad lambda");
  REFUSE_RANKS(g, "amg_coarsest_inverse");
  return engine_amg_coarsest_inverse(g->engine, lambda, Ainv, g->err);
}

int sim3opt_preconditioner_apply(sim3opt_graph* g, int32_t prec, double lambda, int32_t nrhs, const double* r,
                                 double* z) {
  if (!g || !r || !z || nrhs < 1 || prec < 0 || prec > 2 || !std::isfinite(lambda) || lambda < 0.0)
    return fail(g, SIM3OPT_ERR_ARG, "preconditioner_apply: bad argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "preconditioner_apply: call sim3opt_initialize first");
  REFUSE_RANKS(g, "preconditioner_apply");
  return engine_precond_apply(g->engine, prec, lambda, nrhs, r, z, g->err);
}

int sim3opt_spmv_spans(sim3opt_graph* g, int32_t* n_spans, int32_t* wrow) {
  if (!g || !n_spans) return fail(g, SIM3OPT_ERR_ARG, "spmv_spans: bad argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "spmv_spans: call sim3opt_initialize first");
  REFUSE_RANKS(g, "spmv_spans");
  return engine_spmv_spans(g->engine, n_spans, wrow, g->err);
}

int sim3opt_spmv_variant(sim3opt_graph* g, int32_t* chunk, int32_t* non_temporal) {
  if (!g || !chunk || !non_temporal) return fail(g, SIM3OPT_ERR_ARG, "spmv_variant: bad argument");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "spmv_variant: call sim3opt_initialize first");
  engine_spmv_variant(g->engine, chunk, non_temporal);
  return SIM3OPT_OK;
}

int sim3opt_operator_apply(sim3opt_graph* g, int32_t nrhs, const double* lambda, const double* p, const double* rvec,
                           double* q, double* pq, double* rp) {
  if (!g || !lambda || !p || !q || !pq || nrhs < 1 || nrhs > 4 || (rvec == nullptr) != (rp == nullptr))
    return fail(g, SIM3OPT_ERR_ARG, "operator_apply: bad argument");
  for (int32_t s = 0; s < nrhs; ++s)
    if (!std::isfinite(lambda[s]) || lambda[s] < 0.0) return fail(g, SIM3OPT_ERR_ARG, "operator_apply: bad lambda");
  if (!g->initialized || g->dirty) return fail(g, SIM3OPT_ERR_STATE, "operator_apply: call sim3opt_initialize first");
  REFUSE_RANKS(g, "operator_apply");
  return engine_operator_apply(g->engine, nrhs, lambda, p, rvec, q, pq, rp, g->err);
}

int sim3opt_partition_plan(sim3opt_graph* g, int32_t world, int32_t locality, int32_t* vertex_of_row,
                           int32_t* row_begin, int32_t* boundary_rows_of_rank, int64_t* cut_edges) {
  try {
    if (!g || world < 1) return fail(g, SIM3OPT_ERR_ARG, "partition_plan: bad argument");
    std::vector<int32_t> order;
    if (locality) locality_order(g->host, order);
    Structure st;
    if (!build_structure(g->host, st, g->err, locality ? &order : nullptr)) return SIM3OPT_ERR_STATE;
    std::vector<int32_t> begin(world + 1), rows, seg;
    partition_rows_equal(st.nb, world, begin.data());
    boundary_rows(st.nb, st.rowptr.data(), st.colidx.data(), world, begin.data(), rows, seg);
    if (vertex_of_row) std::memcpy(vertex_of_row, st.row2vertex.data(), sizeof(int32_t) * (size_t)st.nb);
    if (row_begin) std::memcpy(row_begin, begin.data(), sizeof(int32_t) * (size_t)(world + 1));
    if (boundary_rows_of_rank)
      for (int32_t r = 0; r < world; ++r) boundary_rows_of_rank[r] = seg[r + 1] - seg[r];
    if (cut_edges) {
      auto owner = [&](int32_t row) {
        return (int32_t)(std::upper_bound(begin.begin(), begin.end(), row) - begin.begin()) - 1;
      };
      int64_t cut = 0;
      for (int32_t k : st.active) {
        const int32_t a = st.hidx[g->host.ev0[k]], b = st.hidx[g->host.ev1[k]];
        if (a >= 0 && b >= 0 && owner(a) != owner(b)) ++cut;
      }
      *cut_edges = cut;
    }
    return SIM3OPT_OK;
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "partition_plan: out of host memory or internal error");
  }
}

int sim3opt_bench_stream(sim3opt_graph* g, int32_t mode, int32_t reps, double* ms_mean) {
  if (!g || !ms_mean || reps < 1 || mode < 0 || mode > 2) return fail(g, SIM3OPT_ERR_ARG, "bench_stream: bad argument");
  if (!g->initialized) return fail(g, SIM3OPT_ERR_STATE, "bench_stream: call sim3opt_initialize first");
  REFUSE_RANKS(g, "bench_stream");
  return engine_bench_stream(g->engine, mode, reps, ms_mean, g->err);
}

int sim3opt_partition_rows(int32_t n_block_rows, const int32_t* rowptr, int32_t world,
                           int32_t* row_begin) {
  if (n_block_rows < 0 || !rowptr || world < 1 || !row_begin) return SIM3OPT_ERR_ARG;
  partition_rows(n_block_rows, rowptr, world, row_begin);
  return SIM3OPT_OK;
}

int sim3opt_partition_rows_equal(int32_t n_block_rows, int32_t world, int32_t* row_begin) {
  if (n_block_rows < 0 || world < 1 || !row_begin) return SIM3OPT_ERR_ARG;
  partition_rows_equal(n_block_rows, world, row_begin);
  return SIM3OPT_OK;
}

int sim3opt_comm_allgather_plan(int32_t n_block_rows, int32_t world, int32_t* row_begin,
                                int64_t* count, int64_t* padded_len) {
  if (n_block_rows < 0 || world < 1) return SIM3OPT_ERR_ARG;
  std::vector<int32_t> rb(world + 1);
  partition_rows_equal(n_block_rows, world, rb.data());
  std::vector<int64_t> offs(world + 1);
  for (int r = 0; r <= world; ++r) offs[r] = 7 * (int64_t)rb[r];
  if (row_begin) std::memcpy(row_begin, rb.data(), sizeof(int32_t) * (size_t)(world + 1));
  return allgather_equal_plan(offs.data(), world, count, padded_len) ? 1 : 0;
}

int sim3opt_comm_unique_id(uint8_t id_out[128]) {
  if (!id_out) return SIM3OPT_ERR_ARG;
  std::string err;
  return comm_unique_id(id_out, err);
}

int sim3opt_comm_init(sim3opt_graph* g, int32_t rank, int32_t world, const uint8_t unique_id[128]) {
  if (!g || world < 1 || rank < 0 || rank >= world) return fail(g, SIM3OPT_ERR_ARG, "comm_init: bad rank/world");
  if (g->initialized) return fail(g, SIM3OPT_ERR_STATE, "comm_init: call before sim3opt_initialize");
  if (g->devices_set) return fail(g, SIM3OPT_ERR_STATE, "comm_init: sim3opt_set_devices has given the handle its ranks");
  g->comm_called = true;
  // options.force_collectives: build the communicator and run every collective even with one rank
  // (self-test of the RCCL transport on a single-GPU machine)
  apply_env_overrides(g->opt);
  const bool force = g->opt.force_collectives != 0;
  if (world == 1 && !force) return SIM3OPT_OK;
  if (!unique_id) return fail(g, SIM3OPT_ERR_ARG, "comm_init: null unique id");
  if (g->opt.device >= 0 && hipSetDevice(g->opt.device) != hipSuccess)
    return fail(g, SIM3OPT_ERR_HIP, "comm_init: hipSetDevice failed");
  g->comm.release();
  const int rc = comm_init_rccl(g->comm, rank, world, unique_id, g->err);
  g->comm.force = force;
  g->comm_set = rc == SIM3OPT_OK;
  return rc;
}

int sim3opt_comm_init_callbacks(sim3opt_graph* g, int32_t rank, int32_t world,
                                sim3opt_allreduce_fn allreduce, sim3opt_allgatherv_fn allgatherv,
                                void* ctx) {
  if (!g || world < 1 || rank < 0 || rank >= world || !allreduce || !allgatherv)
    return fail(g, SIM3OPT_ERR_ARG, "comm_init_callbacks: bad argument");
  if (g->initialized) return fail(g, SIM3OPT_ERR_STATE, "comm_init_callbacks: call before sim3opt_initialize");
  if (g->devices_set)
    return fail(g, SIM3OPT_ERR_STATE, "comm_init_callbacks: sim3opt_set_devices has given the handle its ranks");
  g->comm_called = true;
  g->comm.release();
  g->comm.rank = rank;
  g->comm.world = world;
  g->comm.kind = 2;
  g->comm.cb_allreduce = allreduce;
  g->comm.cb_allgatherv = allgatherv;
  g->comm.cb_ctx = ctx;
  g->comm_set = world > 1;
  return SIM3OPT_OK;
}

int sim3opt_halo_plan(sim3opt_graph* g, int32_t world, int32_t rank, int32_t* n_send, int32_t* n_recv,
                      int32_t* send_rows, int32_t* send_seg, int32_t* recv_rows, int32_t* recv_seg) {
  try {
    if (!g || world < 1 || rank < 0 || rank >= world) return fail(g, SIM3OPT_ERR_ARG, "halo_plan: bad argument");
    std::vector<int32_t> order;
    locality_order(g->host, order);
    Structure st;
    if (!build_structure(g->host, st, g->err, &order)) return SIM3OPT_ERR_STATE;
    std::vector<int32_t> begin(world + 1), sr, ss, rr, rs;
    partition_rows_equal(st.nb, world, begin.data());
    halo_plan(st.nb, st.rowptr.data(), st.colidx.data(), world, begin.data(), rank, sr, ss, rr, rs);
    if (n_send) *n_send = (int32_t)sr.size();
    if (n_recv) *n_recv = (int32_t)rr.size();
    if (send_rows) std::memcpy(send_rows, sr.data(), sizeof(int32_t) * sr.size());
    if (recv_rows) std::memcpy(recv_rows, rr.data(), sizeof(int32_t) * rr.size());
    if (send_seg) std::memcpy(send_seg, ss.data(), sizeof(int32_t) * ss.size());
    if (recv_seg) std::memcpy(recv_seg, rs.data(), sizeof(int32_t) * rs.size());
    return SIM3OPT_OK;
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "halo_plan: out of host memory or internal error");
  }
}

int sim3opt_comm_set_alltoallv(sim3opt_graph* g, sim3opt_alltoallv_fn alltoallv) {
  if (!g) return SIM3OPT_ERR_ARG;
  if (g->initialized) return fail(g, SIM3OPT_ERR_STATE, "comm_set_alltoallv: call before sim3opt_initialize");
  if (g->comm.kind != 2) return fail(g, SIM3OPT_ERR_STATE, "comm_set_alltoallv: call sim3opt_comm_init_callbacks first");
  g->comm.cb_alltoallv = alltoallv;
  return SIM3OPT_OK;
}

int sim3opt_local_rows(const sim3opt_graph* g, int32_t* begin, int32_t* end) {
  if (!g || !g->initialized) return SIM3OPT_ERR_STATE;
  engine_local_rows(g->engine, begin, end);
  return SIM3OPT_OK;
}

int sim3opt_set_devices(sim3opt_graph* g, int32_t n, const int32_t* devices, double collective_timeout_s) {
  try {
  if (!g) return SIM3OPT_ERR_ARG;
  if (n < 1 || n > 8 || !devices) return fail(g, SIM3OPT_ERR_ARG, "set_devices: 1 to 8 device ordinals, please");
  if (g->initialized) return fail(g, SIM3OPT_ERR_STATE, "set_devices: call before sim3opt_initialize");
  if (g->comm_called) return fail(g, SIM3OPT_ERR_STATE, "set_devices: sim3opt_comm_init* has given the handle its ranks");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(g, SIM3OPT_ERR_NO_DEVICE, "set_devices: no usable HIP device");
  for (int32_t r = 0; r < n; ++r)
    if (devices[r] < 0 || devices[r] >= ndev) return fail(g, SIM3OPT_ERR_ARG, "set_devices: device ordinal out of range");
  g->group.reset();  // (a second call replaces the first)
  g->devices_set = true;
  if (n == 1) {  // the plain one-rank graph on that device
    g->device_one = g->opt.device = devices[0];
    return SIM3OPT_OK;
  }
  g->group.reset(new RankGroup(n, devices, collective_timeout_s));
  return SIM3OPT_OK;
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "set_devices: out of host memory or internal error");
  }
}

int sim3opt_rank_count(const sim3opt_graph* g) {
  if (!g) return SIM3OPT_ERR_ARG;
  return g->group ? g->group->size() : 1;  // (ranks THIS handle drives; a rank of a multi-process run is one)
}

int sim3opt_local_rows_of_rank(const sim3opt_graph* g, int32_t rank, int32_t* begin, int32_t* end) {
  if (!g || !g->initialized) return SIM3OPT_ERR_STATE;
  if (rank < 0 || rank >= (g->group ? g->group->size() : 1)) return SIM3OPT_ERR_ARG;
  engine_local_rows(g->group ? g->group->ctx(rank).engine : g->engine, begin, end);
  return SIM3OPT_OK;
}

int sim3opt_device_bytes_of_rank(const sim3opt_graph* g, int32_t rank, int64_t bytes[2]) {
  if (!g || !bytes) return SIM3OPT_ERR_ARG;
  if (!g->initialized) return SIM3OPT_ERR_STATE;
  if (rank < 0 || rank >= (g->group ? g->group->size() : 1)) return SIM3OPT_ERR_ARG;
  engine_device_bytes(g->group ? g->group->ctx(rank).engine : g->engine, bytes);
  return SIM3OPT_OK;
}

// ---- diagnostic read-outs of the in-process transport: everything is decided here, on the host and for all ranks at
// once, before any rank enters the collective -- a refusal leaves the ranks in step and the handle as it was
static int comm_apply_ready(sim3opt_graph* g, const char* who) {
  REFUSE_FINISHED(g);
  if (!g->group || !g->initialized) {
    g->err = std::string(who) + ": needs an initialised handle that sim3opt_set_devices gave more than one rank";
    return SIM3OPT_ERR_STATE;
  }
  return SIM3OPT_OK;
}

int sim3opt_comm_apply_allreduce(sim3opt_graph* g, int64_t n, int32_t op, int32_t phase, const double* in, double* out) {
  try {
  if (!g) return SIM3OPT_ERR_ARG;
  int rc = comm_apply_ready(g, "comm_apply_allreduce");
  if (rc) return rc;
  const std::string bad = comm_check_allreduce(n, op, phase, in, out);
  if (!bad.empty()) return fail(g, SIM3OPT_ERR_ARG, bad.c_str());
  return on_ranks(g, [&](Engine* e, int rank, std::string& err) {
    return engine_comm_apply_allreduce(e, (int32_t)n, op, phase, in + (int64_t)rank * n, out + (int64_t)rank * n, err);
  });
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "comm_apply_allreduce: out of host memory or internal error");
  }
}

int sim3opt_comm_apply_allgatherv(sim3opt_graph* g, const int64_t* offs, int32_t phase, const double* in, double* out) {
  try {
  if (!g) return SIM3OPT_ERR_ARG;
  int rc = comm_apply_ready(g, "comm_apply_allgatherv");
  if (rc) return rc;
  const int32_t world = g->group->size();
  const std::string bad = comm_check_allgatherv(offs, world, phase, in, out);
  if (!bad.empty()) return fail(g, SIM3OPT_ERR_ARG, bad.c_str());
  const int64_t total = offs[world];
  return on_ranks(g, [&](Engine* e, int rank, std::string& err) {
    return engine_comm_apply_allgatherv(e, offs, phase, in + (int64_t)rank * total, out + (int64_t)rank * total, err);
  });
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "comm_apply_allgatherv: out of host memory or internal error");
  }
}

int sim3opt_comm_apply_exchange(sim3opt_graph* g, const int64_t* soffs, const int64_t* roffs, int32_t send_phase,
                                int32_t recv_phase, const double* send, double* recv) {
  try {
  if (!g) return SIM3OPT_ERR_ARG;
  int rc = comm_apply_ready(g, "comm_apply_exchange");
  if (rc) return rc;
  const int32_t world = g->group->size();
  std::vector<int64_t> sbase, rbase;  // where rank r's buffers start in send / recv
  const std::string bad = comm_check_exchange(soffs, roffs, world, send_phase, recv_phase, send, recv, sbase, rbase);
  if (!bad.empty()) return fail(g, SIM3OPT_ERR_ARG, bad.c_str());
  return on_ranks(g, [&](Engine* e, int rank, std::string& err) {
    return engine_comm_apply_exchange(e, soffs + (int64_t)rank * (world + 1), roffs + (int64_t)rank * (world + 1),
                                      send_phase, recv_phase, send + sbase[rank], recv + rbase[rank], err);
  });
  } catch (...) {
    return fail(g, SIM3OPT_ERR_ARG, "comm_apply_exchange: out of host memory or internal error");
  }
}

int sim3opt_comm_local_state(sim3opt_graph* g, int64_t out[2]) {
  if (!g) return SIM3OPT_ERR_ARG;
  int rc = comm_apply_ready(g, "comm_local_state");
  if (rc) return rc;
  if (!out) return fail(g, SIM3OPT_ERR_ARG, "comm_local_state: null argument");
  // (the workers are idle between two commands: rank 0's record is read from here)
  return engine_comm_local_state(g->engine, out) ? SIM3OPT_OK
                                                 : fail(g, SIM3OPT_ERR_STATE, "comm_local_state: not the in-process transport");
}

}  // extern "C"
