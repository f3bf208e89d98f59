// single_process_conformance.cpp -- SparseOptimizer::setDevices of include/sim3opt_g2o.hpp against sim3opt_set_devices of
// the C-ABI: the same graph, four ranks on device 0 each way, every estimate bit for bit.
//
//   single_process_conformance gpu <graph file>
// The graph file is text: "V E", then V lines "fixed s0 .. s7", then E lines "v0 v1 m0 .. m7" (%.17g: exact doubles);
// tests/test_gpu_single_process_shim.py writes the suite's 300-vertex Manhattan graph into it.
#include <cstdio>
#include <cstring>
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

struct GraphFile {
  std::vector<int> fixed, v0, v1;
  std::vector<double> states, meas;  // 8 per vertex / edge
  int nv() const { return (int)fixed.size(); }
  int ne() const { return (int)v0.size(); }
};

bool read_graph(const char* path, GraphFile& g) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return false;
  int V = 0, E = 0;
  bool ok = std::fscanf(f, "%d %d", &V, &E) == 2 && V > 0 && E > 0;
  if (ok) {
    g.fixed.resize(V); g.states.resize(8 * (size_t)V);
    g.v0.resize(E); g.v1.resize(E); g.meas.resize(8 * (size_t)E);
  }
  for (int i = 0; ok && i < V; ++i) {
    ok = std::fscanf(f, "%d", &g.fixed[i]) == 1;
    for (int k = 0; ok && k < 8; ++k) ok = std::fscanf(f, "%lf", &g.states[8 * (size_t)i + k]) == 1;
  }
  for (int e = 0; ok && e < E; ++e) {
    ok = std::fscanf(f, "%d %d", &g.v0[e], &g.v1[e]) == 2;
    for (int k = 0; ok && k < 8; ++k) ok = std::fscanf(f, "%lf", &g.meas[8 * (size_t)e + k]) == 1;
  }
  std::fclose(f);
  return ok;
}

// the way testDirectSim3Optimization builds its graph (kitti_surf.cpp:560-670), the suite's options on top
void build(g2o::SparseOptimizer& opt, const GraphFile& g) {
  sim3opt_options o;
  sim3opt_get_options(opt.handle(), &o);
  o.fix_small_angle_b = 1;
  o.fd_delta = 1e-6;
  o.pcg_rel_tol = 1e-12;
  o.preconditioner = 0;
  sim3opt_set_options(opt.handle(), &o);
  for (int i = 0; i < g.nv(); ++i) {
    auto* v = new vio::VertexSim3Expmap();
    g2o::Sim3 s;
    for (int k = 0; k < 8; ++k) s.v[k] = g.states[8 * (size_t)i + k];
    v->setEstimate(s);
    v->setId(i);
    v->setFixed(g.fixed[i] != 0);
    opt.addVertex(v);
  }
  for (int e = 0; e < g.ne(); ++e) {
    auto* ed = new vio::EdgeSim3();
    ed->setVertex(0, opt.vertex(g.v0[e]));
    ed->setVertex(1, opt.vertex(g.v1[e]));
    g2o::Sim3 m;
    for (int k = 0; k < 8; ++k) m.v[k] = g.meas[8 * (size_t)e + k];
    ed->setMeasurement(m);
    opt.addEdge(ed);
  }
}

int gpu_part(const char* path) {
  GraphFile g;
  if (!read_graph(path, g)) {
    std::fprintf(stderr, "cannot read the graph file %s\n", path);
    return 3;
  }
  // through the shim: the two-line change of testDirectSim3Optimization
  g2o::SparseOptimizer shim;
  build(shim, g);
  EXPECT(!shim.setDevices({}));  // (refused: the graph stays as it is)
  EXPECT(shim.setDevices({0, 0, 0, 0}));
  EXPECT(sim3opt_rank_count(shim.handle()) == 4);
  if (!shim.initializeOptimization()) {
    std::fprintf(stderr, "initializeOptimization: %s\n", shim.lastError());
    return 3;
  }
  // the same through the C-ABI
  g2o::SparseOptimizer capi;
  build(capi, g);
  const int32_t devices[4] = {0, 0, 0, 0};
  EXPECT(sim3opt_set_devices(capi.handle(), 4, devices, 0.0) == SIM3OPT_OK);
  if (sim3opt_initialize(capi.handle()) != SIM3OPT_OK) {
    std::fprintf(stderr, "sim3opt_initialize: %s\n", sim3opt_last_error(capi.handle()));
    return 3;
  }
  const int it_shim = shim.optimize(4), it_c = sim3opt_optimize(capi.handle(), 4);
  EXPECT(it_shim == 4 && it_c == 4);
  std::vector<double> a(8 * (size_t)g.nv()), b(a.size());
  EXPECT(sim3opt_get_vertices(shim.handle(), a.data()) == SIM3OPT_OK);
  EXPECT(sim3opt_get_vertices(capi.handle(), b.data()) == SIM3OPT_OK);
  EXPECT(std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
  int moved = 0;
  for (int i = 0; i < g.nv(); ++i) {  // ... and as the caller reads them: vertex(i)->estimate()
    const g2o::Sim3 s = static_cast<vio::VertexSim3Expmap*>(shim.vertex(i))->estimate();
    const g2o::Sim3 c = static_cast<vio::VertexSim3Expmap*>(capi.vertex(i))->estimate();
    bool same = true;
    for (int k = 0; k < 8; ++k) same = same && std::memcmp(&s.v[k], &c.v[k], sizeof(double)) == 0 && s.v[k] == b[8 * (size_t)i + k];
    EXPECT(same);
    moved += std::memcmp(&b[8 * (size_t)i], &g.states[8 * (size_t)i], sizeof(double) * 8) != 0;
  }
  EXPECT(moved > g.nv() / 2);  // (the optimiser did something)
  EXPECT(shim.chi2() == capi.chi2());
  int32_t lo = -1, hi = -1, next = 0;
  for (int r = 0; r < 4; ++r) {  // the ranks' rows tile the system
    EXPECT(sim3opt_local_rows_of_rank(shim.handle(), r, &lo, &hi) == SIM3OPT_OK && lo == next && hi >= lo);
    next = hi;
  }
  int32_t nb = 0;
  EXPECT(sim3opt_system_dims(shim.handle(), &nb, nullptr) == SIM3OPT_OK && next == nb);
  std::printf("4 ranks on device 0, 4 LM iterations: chi2 %.17g (shim) %.17g (C-ABI), %d of %d vertices moved\n", shim.chi2(),
              capi.chi2(), moved, g.nv());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3 || std::string(argv[1]) != "gpu") {
    std::fprintf(stderr, "usage: single_process_conformance gpu <graph file>\n");
    return 2;
  }
  const int rc = gpu_part(argv[2]);
  std::printf("%d passed, %d failed\n", g_checked - g_failed, g_failed);
  return rc ? rc : (g_failed ? 1 : 0);
}
