// algorithms_conformance.cpp -- conformance test of the algorithm part of include/sim3opt_g2o.hpp: the
// g2o::OptimizationAlgorithmGaussNewton / OptimizationAlgorithmDogleg classes and SparseOptimizer::setAlgorithm, in
// the call forms a g2o pose-graph back end uses (optimizer.setAlgorithm(new g2o::OptimizationAlgorithmDogleg(...))).
//
//   algorithms_conformance host    defaults, setters, ownership, what reaches sim3opt_options (no GPU)
//   algorithms_conformance gpu     dogleg and Gauss-Newton through the shim against the C-ABI on the same graph
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <Eigen/Core>

#include "sim3opt_g2o.hpp"

namespace {

int g_failed = 0, g_checked = 0;
void expect(bool ok, const char* what, int line) {
  ++g_checked;
  if (!ok) {
    ++g_failed;
    std::fprintf(stderr, "FAILED line %d: %s\n", line, what);
  }
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)

constexpr int N = 8;
int id_of(int i) { return 20 + i; }

// a ring of N poses with two chords whose measurements are off by half a metre
struct EdgeSpec {
  int a, b;
  double meas[8];
};
std::vector<EdgeSpec> edges() {
  std::vector<EdgeSpec> es;
  for (int i = 0; i < N + 2; ++i) {
    const int a = i < N ? i : i - N, b = i < N ? (i + 1) % N : i - N + 4;
    const double ang = 0.05 + 0.003 * i;
    EdgeSpec e{a, b, {0.0, std::sin(ang / 2), 0.0, std::cos(ang / 2), 0.7, 0.04 * i, 0.01, 1.02}};
    if (i >= N) e.meas[4] += 0.5;
    es.push_back(e);
  }
  return es;
}
void state_of(int i, double s[8]) {
  const double a = 0.07 * i;
  const double v[8] = {0.0, std::sin(a / 2), 0.0, std::cos(a / 2), 0.9 * i, 0.2 * i, 0.0, 1.0 + 0.02 * i};
  for (int k = 0; k < 8; ++k) s[k] = v[k];
}

void build(g2o::SparseOptimizer& opt) {
  for (int i = 0; i < N; ++i) {
    auto* v = new vio::VertexSim3Expmap();
    g2o::Sim3 s;
    state_of(i, s.v.data());
    v->setEstimate(s);
    v->setId(id_of(i));
    v->setFixed(i == 0);
    opt.addVertex(v);
  }
  for (const EdgeSpec& es : edges()) {
    auto* e = new vio::EdgeSim3();
    e->setVertex(0, opt.vertex(id_of(es.a)));
    e->setVertex(1, opt.vertex(id_of(es.b)));
    g2o::Sim3 m;
    for (int c = 0; c < 8; ++c) m.v[c] = es.meas[c];
    e->setMeasurement(m);
    opt.addEdge(e);
  }
}

sim3opt_graph* build_c(const sim3opt_options& o) {
  sim3opt_graph* g = sim3opt_create();
  sim3opt_set_options(g, &o);
  for (int i = 0; i < N; ++i) {
    double s[8];
    state_of(i, s);
    sim3opt_add_vertex(g, id_of(i), s, i == 0);
  }
  for (const EdgeSpec& es : edges()) sim3opt_add_edge(g, id_of(es.a), id_of(es.b), es.meas, nullptr, 0, 0.0);
  return g;
}

std::unique_ptr<g2o::BlockSolverX> block_solver() {
  auto linear = g2o::make_unique<g2o::LinearSolverEigen<g2o::BlockSolverX::PoseMatrixType>>();
  std::unique_ptr<g2o::BlockSolverX::LinearSolverType> as_base = std::move(linear);
  return g2o::make_unique<g2o::BlockSolverX>(std::move(as_base));
}

void host_part() {
  // defaults are g2o's, in the options and in the class
  sim3opt_options d;
  sim3opt_options_default(&d);
  EXPECT(d.algorithm == SIM3OPT_ALGORITHM_LM && d.dl_max_trials == 100 && d.dl_delta_init == 1e4 &&
         d.dl_lambda_init == 1e-7 && d.dl_lambda_factor == 10.0);
  {
    g2o::OptimizationAlgorithmDogleg loose(block_solver());
    EXPECT(loose.userDeltaInit() == 1e4 && loose.maxTrialsAfterFailure() == 100 && loose.initialLambda() == 1e-7 &&
           loose.lamdbaFactor() == 10.0);
    EXPECT(loose.lastStep() == g2o::OptimizationAlgorithmDogleg::STEP_UNDEFINED);
    EXPECT(loose.currentDelta() == 1e4 && loose.wasPDInAllIterations());
  }
  // step names and numbers (g2o's enum)
  EXPECT(g2o::OptimizationAlgorithmDogleg::STEP_SD == 1 && g2o::OptimizationAlgorithmDogleg::STEP_GN == 2 &&
         g2o::OptimizationAlgorithmDogleg::STEP_DL == 3);
  EXPECT(std::strcmp(g2o::OptimizationAlgorithmDogleg::stepType2Str(g2o::OptimizationAlgorithmDogleg::STEP_SD),
                     "Descent") == 0);
  EXPECT(std::strcmp(g2o::OptimizationAlgorithmDogleg::stepType2Str(g2o::OptimizationAlgorithmDogleg::STEP_GN),
                     "GN") == 0);
  EXPECT(std::strcmp(g2o::OptimizationAlgorithmDogleg::stepType2Str(g2o::OptimizationAlgorithmDogleg::STEP_DL),
                     "Dogleg") == 0);
  EXPECT(std::strcmp(g2o::OptimizationAlgorithmDogleg::stepType2Str(0), "Undefined") == 0);

  // setters before setAlgorithm land at setAlgorithm, setters after it at once
  g2o::SparseOptimizer opt;
  auto* dl = new g2o::OptimizationAlgorithmDogleg(block_solver());
  dl->setUserDeltaInit(250.0);
  dl->setMaxTrialsAfterFailure(7);
  opt.setAlgorithm(dl);  // owned from here on
  sim3opt_options o;
  sim3opt_get_options(opt.handle(), &o);
  EXPECT(o.algorithm == SIM3OPT_ALGORITHM_DOGLEG && o.dl_delta_init == 250.0 && o.dl_max_trials == 7);
  EXPECT(o.dl_lambda_init == 1e-7 && o.dl_lambda_factor == 10.0);
  dl->setInitialLambda(1e-5);
  dl->setLamdbaFactor(4.0);
  sim3opt_get_options(opt.handle(), &o);
  EXPECT(o.dl_lambda_init == 1e-5 && o.dl_lambda_factor == 4.0 && o.dl_delta_init == 250.0);
  // an out-of-range value is refused by the library: the options keep the last good one
  dl->setLamdbaFactor(-1.0);
  sim3opt_get_options(opt.handle(), &o);
  EXPECT(o.dl_lambda_factor == 4.0);
  // no optimize() yet: nothing to report
  sim3opt_tr_stats t;
  EXPECT(sim3opt_get_trust_region_stats(opt.handle(), 0, &t) != SIM3OPT_OK);
  EXPECT(dl->lastStep() == g2o::OptimizationAlgorithmDogleg::STEP_UNDEFINED);

  // Gauss-Newton replaces dogleg (and frees it); Levenberg goes back to algorithm 0 and keeps its settings
  opt.setAlgorithm(new g2o::OptimizationAlgorithmGaussNewton(block_solver()));
  sim3opt_get_options(opt.handle(), &o);
  EXPECT(o.algorithm == SIM3OPT_ALGORITHM_GAUSS_NEWTON);
  auto* lm = new g2o::OptimizationAlgorithmLevenberg(block_solver());
  lm->setMaxTrialsAfterFailure(6);
  opt.setAlgorithm(lm);
  sim3opt_get_options(opt.handle(), &o);
  EXPECT(o.algorithm == SIM3OPT_ALGORITHM_LM && o.max_trials == 6);
  // the C-ABI refuses what the shim's setters cannot reach
  sim3opt_graph* g = sim3opt_create();
  sim3opt_options bad = d;
  bad.algorithm = 3;
  EXPECT(sim3opt_set_options(g, &bad) == SIM3OPT_ERR_ARG);
  bad = d;
  bad.dl_delta_init = INFINITY;
  EXPECT(sim3opt_set_options(g, &bad) == SIM3OPT_ERR_ARG);
  sim3opt_destroy(g);
}

int gpu_part() {
  // dogleg through the shim, started with a small trust radius, against the C-ABI with the same options
  g2o::SparseOptimizer opt;
  build(opt);
  auto* dl = new g2o::OptimizationAlgorithmDogleg(block_solver());
  dl->setUserDeltaInit(0.05);
  opt.setAlgorithm(dl);
  if (!opt.initializeOptimization()) {
    std::fprintf(stderr, "initializeOptimization: %s\n", opt.lastError());
    return 3;
  }
  sim3opt_options o;
  sim3opt_options_default(&o);
  o.algorithm = SIM3OPT_ALGORITHM_DOGLEG;
  o.dl_delta_init = 0.05;
  sim3opt_graph* g = build_c(o);
  if (sim3opt_initialize(g) != SIM3OPT_OK) {
    std::fprintf(stderr, "sim3opt_initialize: %s\n", sim3opt_last_error(g));
    sim3opt_destroy(g);
    return 3;
  }
  const int it_shim = opt.optimize(10), it_c = sim3opt_optimize(g, 10);
  EXPECT(it_shim == it_c && it_shim > 0);
  double c = -1.0;
  EXPECT(sim3opt_chi2(g, &c) == SIM3OPT_OK);
  EXPECT(opt.chi2() == c);
  sim3opt_tr_stats t;
  EXPECT(sim3opt_get_trust_region_stats(g, it_c - 1, &t) == SIM3OPT_OK);
  EXPECT(dl->lastStep() == t.step && dl->currentDelta() == t.delta_after);
  EXPECT(dl->wasPDInAllIterations());
  std::printf("dogleg after %d iterations: shim %.17g, C-ABI %.17g, last step %s, delta %.6g\n", it_shim, opt.chi2(),
              c, g2o::OptimizationAlgorithmDogleg::stepType2Str(dl->lastStep()), dl->currentDelta());
  // Gauss-Newton on both sides from the same start
  opt.setAlgorithm(new g2o::OptimizationAlgorithmGaussNewton(block_solver()));
  sim3opt_get_options(g, &o);
  o.algorithm = SIM3OPT_ALGORITHM_GAUSS_NEWTON;
  sim3opt_set_options(g, &o);
  std::vector<double> s(8 * N);
  for (int i = 0; i < N; ++i) state_of(i, s.data() + 8 * i);
  EXPECT(sim3opt_set_vertices(g, s.data()) == SIM3OPT_OK);
  EXPECT(sim3opt_set_vertices(opt.handle(), s.data()) == SIM3OPT_OK);
  const int gn_shim = opt.optimize(5), gn_c = sim3opt_optimize(g, 5);
  EXPECT(gn_shim == 5 && gn_c == 5);
  EXPECT(sim3opt_chi2(g, &c) == SIM3OPT_OK);
  EXPECT(opt.chi2() == c);
  EXPECT(sim3opt_get_trust_region_stats(g, 0, &t) == SIM3OPT_ERR_STATE);  // not a dogleg run
  std::printf("Gauss-Newton after 5 iterations: shim %.17g, C-ABI %.17g\n", opt.chi2(), c);
  sim3opt_destroy(g);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "host";
  int rc = 0;
  if (mode == "host") host_part();
  else if (mode == "gpu") rc = gpu_part();
  else {
    std::fprintf(stderr, "usage: algorithms_conformance host|gpu\n");
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return rc ? rc : (g_failed ? 1 : 0);
}
