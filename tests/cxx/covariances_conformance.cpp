// covariances_conformance.cpp -- conformance test of the any-pair covariances and the edge gate of
// include/sim3opt_g2o.hpp: SparseOptimizer::computeMarginals for pairs no edge joins (sim3opt_covariances) and
// SparseOptimizer::gateEdge (sim3opt_gate_edges), on a ten-vertex chain with one loop and one fixed vertex.
//
//   covariances_conformance host    what is refused without a GPU: no initializeOptimization, foreign edges
//   covariances_conformance gpu     the shim against the C-ABI, bit for bit (GPU)
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
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

using Block = Eigen::Matrix<double, 7, 7>;
constexpr int N = 10;
int id_of(int i) { return 100 + 10 * i; }

g2o::Sim3 step_measurement(int i) {
  g2o::Sim3 m;
  const double a = 0.04 + 0.003 * i;
  m.v = {{0.0, std::sin(a / 2), 0.01, std::cos(a / 2), 0.9, -0.05, 0.02, 0.99}};
  const double n = std::sqrt(m.v[1] * m.v[1] + m.v[2] * m.v[2] + m.v[3] * m.v[3]);
  for (int c = 0; c < 4; ++c) m.v[c] /= n;
  return m;
}

// a chain 0 - 1 - ... - 9 plus the loop 9 - 0; vertex 0 fixed; a small rotation and scale drift per step
void build(g2o::SparseOptimizer& opt) {
  for (int i = 0; i < N; ++i) {
    auto* v = new vio::VertexSim3Expmap();
    g2o::Sim3 s;
    const double a = 0.05 * i;
    s.v = {{0.0, std::sin(a / 2), 0.0, std::cos(a / 2), 1.0 * i, 0.1 * i, 0.0, 1.0 + 0.01 * i}};
    v->setEstimate(s);
    v->setId(id_of(i));
    v->setFixed(i == 0);
    opt.addVertex(v);
  }
  for (int i = 0; i < N; ++i) {
    auto* e = new vio::EdgeSim3();
    e->setVertex(0, opt.vertex(id_of(i)));
    e->setVertex(1, opt.vertex(id_of((i + 1) % N)));
    e->setMeasurement(step_measurement(i));
    opt.addEdge(e);
  }
}

// a candidate closure between vertices i and j, never added
void candidate(g2o::SparseOptimizer& opt, vio::EdgeSim3& e, int i, int j, bool with_info) {
  e.setVertex(0, opt.vertex(id_of(i)));
  e.setVertex(1, opt.vertex(id_of(j)));
  g2o::Sim3 m = step_measurement(3);
  m.v[4] = -1.0 * (j - i);
  e.setMeasurement(m);
  if (with_info) {
    Block info;
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) info(r, c) = r == c ? 2.0 + 0.25 * r : 0.05;
    e.information() = info;
  }
}

void host_part() {
  g2o::SparseOptimizer opt;
  build(opt);
  vio::EdgeSim3 cand, loose;
  candidate(opt, cand, 2, 7, false);
  double d2 = -1.0;
  Block S;
  S(0, 0) = -2.0;
  EXPECT(!opt.gateEdge(cand, d2, &S));  // before initializeOptimization
  EXPECT(!opt.gateEdge(loose, d2));     // no vertices
  EXPECT(d2 == -1.0 && S(0, 0) == -2.0);
  g2o::SparseBlockMatrix<Block> spinv;
  EXPECT(!opt.computeMarginals(spinv, std::vector<std::pair<int, int>>{{0, 5}}));  // not initialised
  EXPECT(!opt.computeMarginals(spinv, std::vector<std::pair<int, int>>{{0, N - 1}}));  // out of range
  EXPECT(spinv.nonZeroBlocks() == 0);
}

int gpu_part() {
  g2o::SparseOptimizer opt;
  build(opt);
  if (!opt.initializeOptimization()) {
    std::fprintf(stderr, "initializeOptimization: %s\n", opt.lastError());
    return 3;
  }
  opt.optimize(5);
  // a pair of free vertices outside the factor's pattern: the one sim3opt_marginals refuses
  int oi = -1, oj = -1;
  std::vector<double> cov(49);
  for (int i = 1; i < N && oi < 0; ++i)
    for (int j = i + 2; j < N && oi < 0; ++j) {
      const int32_t a = id_of(i), b = id_of(j);
      if (sim3opt_marginals(opt.handle(), 0.0, 1, &a, &b, cov.data()) == SIM3OPT_ERR_ARG) { oi = i; oj = j; }
    }
  EXPECT(oi > 0);
  if (oi < 0) return 0;
  const int hi = opt.vertex(id_of(oi))->hessianIndex(), hj = opt.vertex(id_of(oj))->hessianIndex();
  g2o::SparseBlockMatrix<Block> spinv;
  const bool ok = opt.computeMarginals(spinv, std::vector<std::pair<int, int>>{{hi, hj}, {hj, hi}, {0, 1}, {0, 0}});
  EXPECT(ok);
  if (!ok) {
    std::fprintf(stderr, "computeMarginals: %s\n", opt.lastError());
    return 0;
  }
  EXPECT(spinv.nonZeroBlocks() == 4);
  const Block *zij = spinv.block(hi, hj), *zji = spinv.block(hj, hi), *e01 = spinv.block(0, 1), *d00 = spinv.block(0, 0);
  EXPECT(zij && zji && e01 && d00);
  if (!zij || !zji || !e01 || !d00) return 0;
  {  // the pair outside the pattern: sim3opt_covariances' bits, the reversed pair its transpose, not zero
    const int32_t a = id_of(oi), b = id_of(oj);
    EXPECT(sim3opt_covariances(opt.handle(), 0.0, 1, &a, &b, cov.data()) == SIM3OPT_OK);
    bool same = true, tr = true, nonzero = false;
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) {
        same = same && (*zij)(r, c) == cov[r + 7 * c];
        tr = tr && (*zij)(r, c) == (*zji)(c, r);
        nonzero = nonzero || (*zij)(r, c) != 0.0;
      }
    EXPECT(same);
    EXPECT(tr);
    EXPECT(nonzero);
  }
  {  // pairs on the pattern: sim3opt_marginals' bits, as before
    std::vector<double> m2(2 * 49);
    const int32_t a[2] = {id_of(1), id_of(1)}, b[2] = {id_of(2), id_of(1)};
    EXPECT(sim3opt_marginals(opt.handle(), 0.0, 2, a, b, m2.data()) == SIM3OPT_OK);
    bool edge = true, diag = true;
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) {
        edge = edge && (*e01)(r, c) == m2[r + 7 * c];
        diag = diag && (*d00)(r, c) == m2[49 + r + 7 * c];
      }
    EXPECT(edge);
    EXPECT(diag);
  }
  // gateEdge against sim3opt_gate_edges, without and with an information matrix
  double shown = 0.0;
  for (int with_info = 0; with_info < 2; ++with_info) {
    vio::EdgeSim3 cand;
    candidate(opt, cand, oi, oj, with_info != 0);
    double d2 = -1.0, d2_only = -1.0;
    Block S;
    EXPECT(opt.gateEdge(cand, d2, &S));
    EXPECT(opt.gateEdge(cand, d2_only));
    g2o::Sim3 m = step_measurement(3);
    m.v[4] = -1.0 * (oj - oi);
    double info[49], e[7], Sv[49], dref = -2.0;
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) info[r + 7 * c] = r == c ? 2.0 + 0.25 * r : 0.05;
    const int32_t a = id_of(oi), b = id_of(oj);
    EXPECT(sim3opt_gate_edges(opt.handle(), 0.0, 1, &a, &b, m.v.data(), with_info ? info : nullptr, e, Sv, &dref) ==
           SIM3OPT_OK);
    bool same = true;
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) same = same && S(r, c) == Sv[r + 7 * c];
    EXPECT(same);
    EXPECT(d2 == dref && d2_only == dref && d2 > 0.0);
    shown = d2;
  }
  std::printf("covariances: pair (%d, %d) outside the pattern, gate d2 %.6e\n", id_of(oi), id_of(oj), shown);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  int rc = 0;
  if (mode == "host") host_part();
  else if (mode == "gpu") rc = gpu_part();
  else {
    std::fprintf(stderr, "usage: %s host | gpu\n", argv[0]);
    return 2;
  }
  if (rc) return rc;
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
