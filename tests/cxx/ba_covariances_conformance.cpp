// ba_covariances_conformance.cpp -- conformance test of the covariance part of include/sim3opt_g2o_ba.hpp:
// Vertex::hessianIndex, the header's SparseBlockMatrix and SparseOptimizer::computeMarginals (both overloads), on a
// four-camera scene with noisy observations whose first two cameras are fixed.
//
//   ba_covariances_conformance host     numbering and container semantics (no GPU)
//   ba_covariances_conformance gpu      computeMarginals against sim3opt_ba_covariances on the same handle (GPU)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include <Eigen/Core>
#include <Eigen/Geometry>

#include "sim3opt_g2o_ba.hpp"

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

const double kFocal = 718.856, kCx = 607.1928, kCy = 185.2157;
const int kCams = 4, kPoints = 12;

struct Scene {
  std::unique_ptr<g2o::SparseOptimizer> opt;
  std::vector<g2o::VertexSE3Expmap*> cams;
  std::vector<g2o::VertexSBAPointXYZ*> points;
};

// camera c has id 10 + 3 c, point p has id 100 + p: ascending ids are cameras, then points.  Point p is seen by
// cameras p % 4 and (p + 1) % 4, and by a third one when p is even.
Scene build() {
  Scene s;
  s.opt.reset(new g2o::SparseOptimizer());
  std::unique_ptr<g2o::BlockSolver_6_3::LinearSolverType> linear =
      g2o::make_unique<g2o::LinearSolverEigen<g2o::BlockSolver_6_3::PoseMatrixType>>();
  s.opt->setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<g2o::BlockSolver_6_3>(std::move(linear))));
  auto* K = new g2o::CameraParameters(kFocal, Eigen::Vector2d(kCx, kCy), 0.0);
  K->setId(0);
  EXPECT(s.opt->addParameter(K));
  std::vector<g2o::SE3Quat> T;
  for (int c = 0; c < kCams; ++c) {
    T.emplace_back(Eigen::Quaterniond(1.0, 0.0, 0.0, 0.0), Eigen::Vector3d(-0.5 * c, 0.02 * c, 0.0));
    auto* v = new g2o::VertexSE3Expmap();
    v->setId(10 + 3 * c);
    v->setEstimate(T.back());
    v->setFixed(c < 2);
    EXPECT(s.opt->addVertex(v));
    s.cams.push_back(v);
  }
  for (int p = 0; p < kPoints; ++p) {
    const Eigen::Vector3d X(-2.0 + 0.4 * p, -1.0 + 0.2 * (p % 5), 7.0 + 0.9 * (p % 4));
    auto* v = new g2o::VertexSBAPointXYZ();
    v->setId(100 + p);
    v->setMarginalized(true);
    v->setEstimate(Eigen::Vector3d(X[0] + 0.01 * (p % 3), X[1] - 0.01, X[2] + 0.02 * (p % 2)));
    EXPECT(s.opt->addVertex(v));
    s.points.push_back(v);
    for (int k = 0; k < (p % 2 == 0 ? 3 : 2); ++k) {
      const int c = (p + k) % kCams;
      const auto Y = T[c].map(X);
      auto* e = new g2o::EdgeProjectXYZ2UV();
      e->setVertex(0, v);
      e->setVertex(1, s.cams[c]);
      e->setMeasurement(Eigen::Vector2d(kFocal * Y[0] / Y[2] + kCx + 0.3 * ((p + k) % 3 - 1),
                                        kFocal * Y[1] / Y[2] + kCy - 0.2 * ((p + 2 * k) % 3 - 1)));
      e->setInformation(Eigen::Matrix2d::Identity());
      auto* rk = new g2o::RobustKernelHuber;
      rk->setDelta(2.5);
      e->setRobustKernel(rk);
      EXPECT(e->setParameterId(0, 0));
      EXPECT(s.opt->addEdge(e));
    }
  }
  return s;
}

void host_part() {
  g2o::SparseBlockMatrix M;
  EXPECT(M.block(0, 0) == nullptr && M.nonZeroBlocks() == 0);
  g2o::SparseBlockMatrix::Block& B = M.set(2, 5, 3, 6);
  B(2, 4) = 7.0;
  EXPECT(M.block(2, 5) != nullptr && M.block(5, 2) == nullptr && M.nonZeroBlocks() == 1);
  EXPECT(M.block(2, 5)->rows() == 3 && M.block(2, 5)->cols() == 6 && (*M.block(2, 5))(2, 4) == 7.0);
  EXPECT(M.block(2, 5)->data()[2 + 3 * 4] == 7.0 && (*M.block(2, 5))(0, 0) == 0.0);  // column-major, zero-filled
  M.clear();
  EXPECT(M.nonZeroBlocks() == 0);

  Scene s = build();
  for (auto* c : s.cams) EXPECT(c->hessianIndex() == -1);  // before initializeOptimization
  g2o::SparseBlockMatrix spinv;
  EXPECT(!s.opt->computeMarginals(spinv, std::vector<std::pair<int, int>>{{0, 0}}));
  EXPECT(s.opt->initializeOptimization());
  // g2o's numbering: the free cameras in ascending id, then the points; -1 for the fixed ones
  EXPECT(s.cams[0]->hessianIndex() == -1 && s.cams[1]->hessianIndex() == -1);
  EXPECT(s.cams[2]->hessianIndex() == 0 && s.cams[3]->hessianIndex() == 1);
  for (int p = 0; p < kPoints; ++p) EXPECT(s.points[p]->hessianIndex() == 2 + p);
  // refusals that need no device
  EXPECT(!s.opt->computeMarginals(spinv, s.cams[0]));  // fixed
  EXPECT(!s.opt->computeMarginals(spinv, std::vector<std::pair<int, int>>{{0, 2 + kPoints}}));  // out of range
  EXPECT(!s.opt->computeMarginals(spinv, std::vector<std::pair<int, int>>{{2, 3}}));            // two different points
  EXPECT(spinv.nonZeroBlocks() == 0);
}

int gpu_part() {
  Scene s = build();
  if (!s.opt->initializeOptimization()) {
    std::fprintf(stderr, "initializeOptimization failed: %s\n", s.opt->lastError());
    return 3;
  }
  const int h2 = s.cams[2]->hessianIndex(), h3 = s.cams[3]->hessianIndex();
  const int hp = s.points[4]->hessianIndex(), hq = s.points[7]->hessianIndex();
  // point 4 is seen by cameras 0, 1, 2; point 7 by cameras 3 and 0
  const std::vector<std::pair<int, int>> want = {{h2, h2}, {h2, h3}, {h3, h2}, {hp, hp}, {hq, hq}, {hp, h2}, {h2, hp}, {hq, h3}};
  g2o::SparseBlockMatrix spinv;
  if (!s.opt->computeMarginals(spinv, want)) {
    std::fprintf(stderr, "computeMarginals failed: %s\n", s.opt->lastError());
    return 3;
  }
  EXPECT(spinv.nonZeroBlocks() == want.size());
  // the same blocks through the C-ABI, on the same handle
  const int32_t ca[3] = {2, 2, 3}, cb[3] = {2, 3, 2}, pt[2] = {4, 7}, qp[2] = {4, 7}, qc[2] = {2, 3};
  double cc[3 * 36], pp[2 * 9], pc[2 * 18];
  EXPECT(sim3opt_ba_covariances(s.opt->handle(), 0.0, 3, ca, cb, cc, 2, pt, pp, 2, qp, qc, pc) == SIM3OPT_OK);
  auto same = [&](int r, int c, int rows, int cols, const double* src) {
    const g2o::SparseBlockMatrix::Block* B = spinv.block(r, c);
    if (!B || B->rows() != rows || B->cols() != cols) return false;
    return std::memcmp(B->data(), src, sizeof(double) * rows * cols) == 0;
  };
  EXPECT(same(h2, h2, 6, 6, cc) && same(h2, h3, 6, 6, cc + 36) && same(h3, h2, 6, 6, cc + 72));
  EXPECT(same(hp, hp, 3, 3, pp) && same(hq, hq, 3, 3, pp + 9));
  EXPECT(same(hp, h2, 3, 6, pc) && same(hq, h3, 3, 6, pc + 18));
  // (camera, point) is the transpose of (point, camera); (h3, h2) of (h2, h3)
  const g2o::SparseBlockMatrix::Block *A = spinv.block(h2, hp), *At = spinv.block(hp, h2);
  EXPECT(A && At && A->rows() == 6 && A->cols() == 3);
  bool transposed = A && At;
  for (int r = 0; transposed && r < 6; ++r)
    for (int c = 0; c < 3; ++c) transposed = transposed && (*A)(r, c) == (*At)(c, r);
  EXPECT(transposed);
  const g2o::SparseBlockMatrix::Block *E = spinv.block(h2, h3), *Et = spinv.block(h3, h2);
  bool sym = E && Et;
  for (int r = 0; sym && r < 6; ++r)
    for (int c = 0; c < 6; ++c) sym = sym && (*E)(r, c) == (*Et)(c, r);
  EXPECT(sym);
  // a variance is positive; the single-vertex overload gives the same block
  EXPECT((*spinv.block(h2, h2))(0, 0) > 0.0 && (*spinv.block(hp, hp))(2, 2) > 0.0);
  g2o::SparseBlockMatrix one;
  EXPECT(s.opt->computeMarginals(one, s.points[4]) && one.nonZeroBlocks() == 1 && one.block(hp, hp) != nullptr);
  EXPECT(one.block(hp, hp) && std::memcmp(one.block(hp, hp)->data(), pp, sizeof(double) * 9) == 0);
  std::printf("ba covariances: camera %d var(omega_x) %.6e, point %d var(z) %.6e\n", s.cams[2]->id(),
              (*spinv.block(h2, h2))(0, 0), s.points[4]->id(), (*spinv.block(hp, hp))(2, 2));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "host";
  int rc = 0;
  if (mode == "host") host_part();
  else if (mode == "gpu") rc = gpu_part();
  else { std::fprintf(stderr, "usage: ba_covariances_conformance host|gpu\n"); return 2; }
  std::printf("%d checked, %d failed\n", g_checked, g_failed);
  return rc ? rc : (g_failed ? 1 : 0);
}
