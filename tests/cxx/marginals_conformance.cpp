// marginals_conformance.cpp -- conformance test of the marginal-covariance part of include/sim3opt_g2o.hpp:
// Vertex::hessianIndex, g2o::SparseBlockMatrix and SparseOptimizer::computeMarginals (the g2o calls a
// caller makes to read pose uncertainties), on a six-vertex chain with one loop and one fixed vertex.
//
//   marginals_conformance host    numbering and container semantics (no GPU)
//   marginals_conformance gpu     computeMarginals against the C-ABI's sim3opt_marginals (GPU)
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
constexpr int N = 6;
int id_of(int i) { return 100 + 10 * i; }

// a chain 0 - 1 - ... - 5 plus the loop 5 - 0; vertex 0 fixed; a small rotation and scale drift per step
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
    const int j = (i + 1) % N;
    auto* e = new vio::EdgeSim3();
    e->setVertex(0, opt.vertex(id_of(i)));
    e->setVertex(1, opt.vertex(id_of(j)));
    g2o::Sim3 m;
    const double a = 0.04 + 0.003 * i;
    m.v = {{0.0, std::sin(a / 2), 0.01, std::cos(a / 2), 0.9, -0.05, 0.02, 0.99}};
    const double n = std::sqrt(m.v[1] * m.v[1] + m.v[2] * m.v[2] + m.v[3] * m.v[3]);
    for (int c = 0; c < 4; ++c) m.v[c] /= n;
    e->setMeasurement(m);
    opt.addEdge(e);
  }
}

void host_part() {
  g2o::SparseOptimizer opt;
  build(opt);
  // hessianIndex: the k-th free vertex in insertion order, -1 for the fixed one
  EXPECT(opt.vertex(id_of(0))->hessianIndex() == -1);
  for (int i = 1; i < N; ++i) EXPECT(opt.vertex(id_of(i))->hessianIndex() == i - 1);
  vio::VertexSim3Expmap loose;
  EXPECT(loose.hessianIndex() == -1);  // not added
  // SparseBlockMatrix: absent blocks are null unless allocated (then zero)
  g2o::SparseBlockMatrix<Block> spinv;
  EXPECT(spinv.block(0, 0) == nullptr);
  Block* b = spinv.block(2, 3, true);
  EXPECT(b != nullptr && spinv.nonZeroBlocks() == 1 && spinv.block(2, 3) == b);
  bool zero = true;
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) zero = zero && (*b)(r, c) == 0.0;
  EXPECT(zero);
  spinv.clear();
  EXPECT(spinv.nonZeroBlocks() == 0);
  // before initializeOptimization, or for a fixed vertex / an index out of range: false, spinv unchanged
  EXPECT(!opt.computeMarginals(spinv, opt.vertex(id_of(1))));
  EXPECT(!opt.computeMarginals(spinv, opt.vertex(id_of(0))));
  EXPECT(!opt.computeMarginals(spinv, std::vector<std::pair<int, int>>{{0, N}}));
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
  g2o::SparseBlockMatrix<Block> spinv;
  const vio::VertexSim3Expmap* v1 = static_cast<vio::VertexSim3Expmap*>(opt.vertex(id_of(1)));
  const bool ok = opt.computeMarginals(spinv, v1);
  EXPECT(ok);
  if (!ok) std::fprintf(stderr, "computeMarginals: %s\n", opt.lastError());
  const Block* m = spinv.block(0, 0);
  EXPECT(m != nullptr && spinv.nonZeroBlocks() == 1);
  if (!m) return 0;
  // the same block through the C-ABI: the same bits (column-major there)
  std::vector<double> cov(2 * 49);
  const int32_t a[2] = {id_of(1), id_of(1)}, b[2] = {id_of(1), id_of(2)};  // (1, 1) and the edge (1, 2)
  EXPECT(sim3opt_marginals(opt.handle(), 0.0, 2, a, b, cov.data()) == SIM3OPT_OK);
  bool same = true, sym = true;
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) {
      same = same && (*m)(r, c) == cov[r + 7 * c];
      sym = sym && (*m)(r, c) == (*m)(c, r);
    }
  EXPECT(same);
  EXPECT(sym);
  EXPECT((*m)(0, 0) > 0.0 && (*m)(6, 6) > 0.0);
  // an edge pair (hessian indices 0, 1 = vertices 1, 2) and its transpose
  EXPECT(opt.computeMarginals(spinv, std::vector<std::pair<int, int>>{{0, 1}, {1, 0}}));
  const Block* e01 = spinv.block(0, 1);
  const Block* e10 = spinv.block(1, 0);
  EXPECT(e01 && e10);
  if (e01 && e10) {
    bool tr = true, cabi = true;
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) {
        tr = tr && (*e01)(r, c) == (*e10)(c, r);
        cabi = cabi && (*e01)(r, c) == cov[49 + r + 7 * c];
      }
    EXPECT(tr);
    EXPECT(cabi);
  }
  std::printf("marginals: vertex %d, sigma(0,0) %.6e, sigma(6,6) %.6e\n", id_of(1), (*m)(0, 0), (*m)(6, 6));
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
