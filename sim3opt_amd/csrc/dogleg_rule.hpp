// dogleg_rule.hpp -- the step rule of Powell's dogleg as host arithmetic (no device code, no engine state): what
// Engine::optimize_dogleg makes of the six scalars of an iteration and the trust radius (DESIGN.md 5h;
// g2o OptimizationAlgorithmDogleg::solve).  Included by engine_algorithms.hip only: the optimiser and
// sim3opt_dogleg_rule run the same compiled functions.
#pragma once

#include <algorithm>
#include <cmath>

#include "../../include/sim3opt.h"

namespace sim3opt {

// the scalars in the order of DL_* (algo_kernels.hpp): b.b, b^T H b, g.g, b.g, (Hb).g, g^T H g for g = h_gn
struct DoglegScalars {
  double bb, bHb, gg, bg, hbg, gHg;
};

// per iteration: h_sd = alpha b and the two norms
struct DoglegModel {
  double alpha, norm_sd, norm_gn;
};

// per trial: h_dl = ca b + cg h_gn, its kind and norm, and the gain the quadratic model predicts for it
struct DoglegTrial {
  double ca, cg, norm_dl, linear_gain;
  int32_t step;  // SIM3OPT_STEP_*
};

inline DoglegModel dogleg_model(const DoglegScalars& s) {
  DoglegModel m;
  m.alpha = s.bb / s.bHb;
  m.norm_sd = std::fabs(m.alpha) * std::sqrt(s.bb);
  m.norm_gn = std::sqrt(s.gg);
  return m;
}

inline DoglegTrial dogleg_trial(const DoglegScalars& s, const DoglegModel& m, double delta) {
  const double alpha = m.alpha;
  DoglegTrial t;
  t.ca = 0.0;
  t.cg = 0.0;
  if (m.norm_gn < delta) {
    t.cg = 1.0;
    t.step = SIM3OPT_STEP_GN;
  } else if (m.norm_sd > delta) {
    t.ca = delta / m.norm_sd * alpha;
    t.step = SIM3OPT_STEP_SD;
  } else {
    // h_sd + beta (h_gn - h_sd), ||.|| = delta; g2o's two numerically stable forms of the root
    const double hsd2 = alpha * alpha * s.bb;
    const double c = alpha * s.bg - hsd2;                    // h_sd . (h_gn - h_sd)
    const double bma2 = s.gg - 2.0 * alpha * s.bg + hsd2;    // ||h_gn - h_sd||^2
    const double d2 = delta * delta - hsd2;
    double beta;
    if (c <= 0.0) beta = (-c + std::sqrt(c * c + bma2 * d2)) / bma2;
    else beta = d2 / (c + std::sqrt(c * c + bma2 * d2));
    t.ca = (1.0 - beta) * alpha;
    t.cg = beta;
    t.step = SIM3OPT_STEP_DL;
  }
  // ||h_dl||^2, b.h_dl and h_dl^T H h_dl as quadratic forms in (ca, cg)
  const double dl2 = t.ca * t.ca * s.bb + 2.0 * t.ca * t.cg * s.bg + t.cg * t.cg * s.gg;
  const double bh = t.ca * s.bb + t.cg * s.bg;
  const double hHh = t.ca * t.ca * s.bHb + 2.0 * t.ca * t.cg * s.hbg + t.cg * t.cg * s.gHg;
  t.linear_gain = 2.0 * bh - hHh;
  t.norm_dl = std::sqrt(std::max(0.0, dl2));
  return t;
}

}  // namespace sim3opt
