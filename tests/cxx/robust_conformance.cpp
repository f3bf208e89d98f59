// robust_conformance.cpp -- conformance test of the robust-kernel part of include/sim3opt_g2o.hpp: the
// g2o::RobustKernel* classes and Edge::setRobustKernel, in the call forms a g2o pose-graph back end uses
// (e->setRobustKernel(new g2o::RobustKernelCauchy); rk->setDelta(d)), on a six-vertex ring with two loops.
//
//   robust_conformance host    classes, defaults, ownership, what reaches the graph (no GPU)
//   robust_conformance gpu     the shim's chi2 against the C-ABI's on the same graph, before and after a
//                              kernel changes on an added edge (GPU)
#include <cmath>
#include <cstdio>
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

constexpr int N = 6;
int id_of(int i) { return 10 + i; }

struct EdgeSpec {
  int a, b;
  double meas[8];
};

// a ring 0 - 1 - ... - 5 - 0 plus the chords 0 - 3 and 1 - 4, the chords' measurements off by a metre
std::vector<EdgeSpec> edges() {
  std::vector<EdgeSpec> es;
  for (int i = 0; i < N + 2; ++i) {
    const int a = i < N ? i : i - N, b = i < N ? (i + 1) % N : i - N + 3;
    const double ang = 0.03 + 0.002 * i;
    EdgeSpec e{a, b, {0.0, std::sin(ang / 2), 0.0, std::cos(ang / 2), 0.8, 0.05 * i, 0.0, 1.01}};
    if (i >= N) e.meas[4] += 1.0;
    es.push_back(e);
  }
  return es;
}

void state_of(int i, double s[8]) {
  const double a = 0.04 * i;
  const double v[8] = {0.0, std::sin(a / 2), 0.0, std::cos(a / 2), 1.0 * i, 0.1 * i, 0.0, 1.0 + 0.01 * i};
  for (int k = 0; k < 8; ++k) s[k] = v[k];
}

g2o::RobustKernel* make_kernel(int kind) {
  switch (kind) {
    case SIM3OPT_KERNEL_HUBER: return new g2o::RobustKernelHuber;
    case SIM3OPT_KERNEL_PSEUDO_HUBER: return new g2o::RobustKernelPseudoHuber;
    case SIM3OPT_KERNEL_CAUCHY: return new g2o::RobustKernelCauchy;
    case SIM3OPT_KERNEL_GEMAN_MCCLURE: return new g2o::RobustKernelGemanMcClure;
    case SIM3OPT_KERNEL_WELSCH: return new g2o::RobustKernelWelsch;
    case SIM3OPT_KERNEL_FAIR: return new g2o::RobustKernelFair;
    case SIM3OPT_KERNEL_TUKEY: return new g2o::RobustKernelTukey;
    case SIM3OPT_KERNEL_SATURATED: return new g2o::RobustKernelSaturated;
    case SIM3OPT_KERNEL_DCS: return new g2o::RobustKernelDCS;
    default: return nullptr;
  }
}

// kinds / deltas the edges of build() get: NONE .. WELSCH round the ring, Cauchy and DCS on the chords
int kind_of(int k) { return k < N ? k % 10 : (k == N ? SIM3OPT_KERNEL_CAUCHY : SIM3OPT_KERNEL_DCS); }
double delta_of(int k) { return 0.05 + 0.1 * k; }

// the graph through the shim; edge pointers returned (the optimizer owns them, as in g2o)
std::vector<vio::EdgeSim3*> build(g2o::SparseOptimizer& opt) {
  for (int i = 0; i < N; ++i) {
    auto* v = new vio::VertexSim3Expmap();
    g2o::Sim3 s;
    state_of(i, s.v.data());
    v->setEstimate(s);
    v->setId(id_of(i));
    v->setFixed(i == 0);
    opt.addVertex(v);
  }
  std::vector<vio::EdgeSim3*> out;
  const std::vector<EdgeSpec> es = edges();
  for (size_t k = 0; k < es.size(); ++k) {
    auto* e = new vio::EdgeSim3();
    e->setVertex(0, opt.vertex(id_of(es[k].a)));
    e->setVertex(1, opt.vertex(id_of(es[k].b)));
    g2o::Sim3 m;
    for (int c = 0; c < 8; ++c) m.v[c] = es[k].meas[c];
    e->setMeasurement(m);
    if (g2o::RobustKernel* rk = make_kernel(kind_of((int)k))) {
      rk->setDelta(delta_of((int)k));
      e->setRobustKernel(rk);
    }
    opt.addEdge(e);
    out.push_back(e);
  }
  return out;
}

// the same graph through the C-ABI
sim3opt_graph* build_c() {
  sim3opt_graph* g = sim3opt_create();
  for (int i = 0; i < N; ++i) {
    double s[8];
    state_of(i, s);
    sim3opt_add_vertex(g, id_of(i), s, i == 0);
  }
  const std::vector<EdgeSpec> es = edges();
  for (size_t k = 0; k < es.size(); ++k) {
    const int kind = kind_of((int)k);
    sim3opt_add_edge(g, id_of(es[k].a), id_of(es[k].b), es[k].meas, nullptr, kind,
                     kind == SIM3OPT_KERNEL_NONE ? 0.0 : delta_of((int)k));
  }
  return g;
}

void host_part() {
  // every class: its kind, delta 1 by default (g2o), setDelta, robustify = sim3opt_robustify
  for (int kind = 1; kind < 10; ++kind) {
    std::unique_ptr<g2o::RobustKernel> rk(make_kernel(kind));
    EXPECT(rk && rk->kind() == kind && rk->delta() == 1.0);
    rk->setDelta(2.5);
    EXPECT(rk->delta() == 2.5);
    Eigen::Vector3d rho;
    rk->robustify(3.0, rho);
    double ref[2];
    EXPECT(sim3opt_robustify(kind, 2.5, 3.0, ref) == SIM3OPT_OK);
    EXPECT(rho[0] == ref[0] && rho[1] == ref[1] && rho[2] == 0.0);
  }
  {  // Cauchy by hand: d^2 log(1 + e2/d^2), 1 / (1 + e2/d^2)
    g2o::RobustKernelCauchy c;
    c.setDelta(2.0);
    double rho[3];
    c.robustify(12.0, rho);
    EXPECT(std::fabs(rho[0] - 4.0 * std::log(4.0)) < 1e-14 && std::fabs(rho[1] - 0.25) < 1e-16);
  }
  // an edge owns its kernel and replaces it; setRobustKernelHuber stays
  vio::EdgeSim3 loose;
  EXPECT(loose.robustKernel() == nullptr);
  loose.setRobustKernel(new g2o::RobustKernelTukey);
  EXPECT(loose.robustKernel() && loose.robustKernel()->kind() == SIM3OPT_KERNEL_TUKEY);
  loose.setRobustKernelHuber(0.7);
  EXPECT(loose.robustKernel()->kind() == SIM3OPT_KERNEL_HUBER && loose.robustKernel()->delta() == 0.7);
  loose.setRobustKernel(nullptr);
  EXPECT(loose.robustKernel() == nullptr);
  // what reaches the graph at addEdge, and a kernel set on an added edge (before initializeOptimization)
  g2o::SparseOptimizer opt;
  std::vector<vio::EdgeSim3*> es = build(opt);
  const int m = sim3opt_num_edges(opt.handle());
  EXPECT(m == N + 2);
  std::vector<int32_t> kinds(m);
  std::vector<double> deltas(m);
  EXPECT(sim3opt_get_edge_kernels(opt.handle(), kinds.data(), deltas.data()) == SIM3OPT_OK);
  for (int k = 0; k < m; ++k) {
    EXPECT(kinds[k] == kind_of(k));
    EXPECT(deltas[k] == (kind_of(k) == SIM3OPT_KERNEL_NONE ? 0.0 : delta_of(k)));
  }
  auto* w = new g2o::RobustKernelWelsch;
  w->setDelta(3.0);
  es[2]->setRobustKernel(w);
  es[N]->setRobustKernel(nullptr);
  EXPECT(sim3opt_get_edge_kernels(opt.handle(), kinds.data(), deltas.data()) == SIM3OPT_OK);
  EXPECT(kinds[2] == SIM3OPT_KERNEL_WELSCH && deltas[2] == 3.0);
  EXPECT(kinds[N] == SIM3OPT_KERNEL_NONE && deltas[N] == 0.0);
  EXPECT(kinds[N + 1] == SIM3OPT_KERNEL_DCS);
}

int gpu_part() {
  g2o::SparseOptimizer opt;
  std::vector<vio::EdgeSim3*> es = build(opt);
  if (!opt.initializeOptimization()) {
    std::fprintf(stderr, "initializeOptimization: %s\n", opt.lastError());
    return 3;
  }
  sim3opt_graph* g = build_c();
  if (sim3opt_initialize(g) != SIM3OPT_OK) {
    std::fprintf(stderr, "sim3opt_initialize: %s\n", sim3opt_last_error(g));
    sim3opt_destroy(g);
    return 3;
  }
  double c = -1.0;
  EXPECT(sim3opt_chi2(g, &c) == SIM3OPT_OK);
  const double s0 = opt.activeRobustChi2();
  EXPECT(s0 == c && c > 0.0);
  std::printf("robust chi2: shim %.17g, C-ABI %.17g\n", s0, c);
  // a kernel changed on an added edge after initializeOptimization: both sides see it at the next chi2
  auto* t = new g2o::RobustKernelTukey;
  t->setDelta(0.2);
  es[N]->setRobustKernel(t);
  const int32_t idx = N, kind = SIM3OPT_KERNEL_TUKEY;
  const double d = 0.2;
  EXPECT(sim3opt_set_edge_kernels(g, 1, &idx, &kind, &d) == SIM3OPT_OK);
  EXPECT(sim3opt_chi2(g, &c) == SIM3OPT_OK);
  const double s1 = opt.activeRobustChi2();
  EXPECT(s1 == c && s1 != s0);
  // and the same LM run
  const int it_shim = opt.optimize(5), it_c = sim3opt_optimize(g, 5);
  EXPECT(it_shim == it_c && it_shim > 0);
  EXPECT(sim3opt_chi2(g, &c) == SIM3OPT_OK);
  EXPECT(opt.chi2() == c);
  std::printf("after 5 iterations: shim %.17g, C-ABI %.17g\n", opt.chi2(), c);
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
    std::fprintf(stderr, "usage: robust_conformance host|gpu\n");
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return rc ? rc : (g_failed ? 1 : 0);
}
