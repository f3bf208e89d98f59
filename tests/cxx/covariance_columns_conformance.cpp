// covariance_columns_conformance.cpp -- conformance test of the column path of include/sim3opt_g2o.hpp:
// SparseOptimizer::setCovarianceSolver (options.cov_solver / cov_rel_tol) and, behind it, computeMarginals and gateEdge
// with the blocks of H^-1 taken from columns of the inverse solved by the PCG, on a ten-vertex chain with one loop and
// one fixed vertex that is kept on the PCG path.
//
//   covariance_columns_conformance host    the setter's validation and the column plan (no GPU)
//   covariance_columns_conformance gpu     the shim against the C-ABI bit for bit, and against the exact path (GPU)
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

void candidate(g2o::SparseOptimizer& opt, vio::EdgeSim3& e, int i, int j) {
  e.setVertex(0, opt.vertex(id_of(i)));
  e.setVertex(1, opt.vertex(id_of(j)));
  g2o::Sim3 m = step_measurement(3);
  m.v[4] = -1.0 * (j - i);
  e.setMeasurement(m);
}

void host_part() {
  g2o::SparseOptimizer opt;
  build(opt);
  sim3opt_options o;
  sim3opt_get_options(opt.handle(), &o);
  EXPECT(o.cov_solver == 0 && o.cov_rel_tol == 1e-8);
  EXPECT(opt.setCovarianceSolver(1, 1e-6));
  EXPECT(!opt.setCovarianceSolver(3));
  EXPECT(!opt.setCovarianceSolver(-1));
  EXPECT(!opt.setCovarianceSolver(1, 0.5));
  EXPECT(!opt.setCovarianceSolver(1, 0.0));
  sim3opt_get_options(opt.handle(), &o);
  EXPECT(o.cov_solver == 1 && o.cov_rel_tol == 1e-6);
  EXPECT(opt.setCovarianceSolver(2));
  sim3opt_get_options(opt.handle(), &o);
  EXPECT(o.cov_solver == 2 && o.cov_rel_tol == 1e-8);
  // the plan of a full block column is its one vertex; a fixed vertex is refused
  std::vector<int32_t> a, b;
  for (int i = 1; i < N; ++i) {
    a.push_back(id_of(i));
    b.push_back(id_of(4));
  }
  int32_t nv = -1, verts[N];
  EXPECT(sim3opt_covariance_columns_plan(opt.handle(), (int32_t)a.size(), a.data(), b.data(), &nv, nullptr) == SIM3OPT_OK);
  EXPECT(nv == 1);
  EXPECT(sim3opt_covariance_columns_plan(opt.handle(), (int32_t)a.size(), a.data(), b.data(), &nv, verts) == SIM3OPT_OK);
  EXPECT(nv == 1 && verts[0] == id_of(4));
  a[0] = id_of(0);
  EXPECT(sim3opt_covariance_columns_plan(opt.handle(), (int32_t)a.size(), a.data(), b.data(), &nv, nullptr) == SIM3OPT_ERR_ARG);
}

int gpu_part() {
  g2o::SparseOptimizer opt;
  build(opt);
  sim3opt_options o;
  sim3opt_get_options(opt.handle(), &o);
  o.linear_solver = 0;  // the PCG path, as on a graph too large to factor
  o.fix_small_angle_b = 1;
  o.fd_delta = 1e-6;
  EXPECT(sim3opt_set_options(opt.handle(), &o) == SIM3OPT_OK);
  EXPECT(opt.setCovarianceSolver(1));
  if (!opt.initializeOptimization()) {
    std::fprintf(stderr, "initializeOptimization: %s\n", opt.lastError());
    return 3;
  }
  EXPECT(sim3opt_linear_solver_in_use(opt.handle()) == 0);
  opt.optimize(5);
  const int oi = 2, oj = 7;
  const int hi = opt.vertex(id_of(oi))->hessianIndex(), hj = opt.vertex(id_of(oj))->hessianIndex();
  g2o::SparseBlockMatrix<Block> spinv;
  const bool ok = opt.computeMarginals(spinv, std::vector<std::pair<int, int>>{{hi, hj}, {hj, hi}, {0, 0}});
  EXPECT(ok);
  if (!ok) {
    std::fprintf(stderr, "computeMarginals: %s\n", opt.lastError());
    return 0;
  }
  int64_t counts[5];
  double res[2];
  EXPECT(sim3opt_covariance_columns_stats(opt.handle(), counts, res) == SIM3OPT_OK);
  EXPECT(counts[0] == 2 && counts[1] == 14 && res[0] <= 1e-8 && res[1] == 1e-8);
  const Block *zij = spinv.block(hi, hj), *zji = spinv.block(hj, hi), *d00 = spinv.block(0, 0);
  EXPECT(zij && zji && d00);
  if (!zij || !zji || !d00) return 0;
  std::vector<double> cov(3 * 49);
  const int32_t a[3] = {id_of(oi), id_of(oj), id_of(1)}, b[3] = {id_of(oj), id_of(oi), id_of(1)};
  EXPECT(sim3opt_covariances(opt.handle(), 0.0, 3, a, b, cov.data()) == SIM3OPT_OK);
  bool same = true, tr = true, sym = true, nonzero = false;
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) {
      same = same && (*zij)(r, c) == cov[r + 7 * c] && (*d00)(r, c) == cov[98 + r + 7 * c];
      tr = tr && (*zij)(r, c) == (*zji)(c, r);
      sym = sym && (*d00)(r, c) == (*d00)(c, r);
      nonzero = nonzero || (*zij)(r, c) != 0.0;
    }
  EXPECT(same);
  EXPECT(tr);
  EXPECT(sym);
  EXPECT(nonzero);
  // gateEdge against sim3opt_gate_edges on the column path, then against the exact path
  vio::EdgeSim3 cand;
  candidate(opt, cand, oi, oj);
  double d2 = -1.0, dref = -2.0, e[7], Sv[49];
  Block S;
  EXPECT(opt.gateEdge(cand, d2, &S));
  g2o::Sim3 m = step_measurement(3);
  m.v[4] = -1.0 * (oj - oi);
  const int32_t ca = id_of(oi), cb = id_of(oj);
  EXPECT(sim3opt_gate_edges(opt.handle(), 0.0, 1, &ca, &cb, m.v.data(), nullptr, e, Sv, &dref) == SIM3OPT_OK);
  bool sameS = true;
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) sameS = sameS && S(r, c) == Sv[r + 7 * c];
  EXPECT(sameS);
  EXPECT(d2 == dref && d2 > 0.0);
  EXPECT(opt.setCovarianceSolver(0));
  double d2_exact = -1.0;
  EXPECT(opt.gateEdge(cand, d2_exact));
  EXPECT(std::fabs(d2_exact - d2) <= 1e-6 * d2_exact);
  std::printf("covariance columns: pair (%d, %d), gate d2 %.9e by columns, %.9e exact\n", id_of(oi), id_of(oj), d2,
              d2_exact);
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
