// lm_damping.hpp -- g2o's Levenberg-Marquardt damping rule (OptimizationAlgorithmLevenberg::solve and
// computeLambdaInit): the pose-graph LM (engine.hip) and the bundle adjuster (ba.hip) run it on the host, the
// batched two-view bundle adjuster (ba_batch.hip) runs the same statements inside its kernel.
#pragma once
#include <algorithm>
#include <cmath>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define SIM3OPT_LM_HD __host__ __device__
#else
#define SIM3OPT_LM_HD
#endif

namespace sim3opt {

struct LmDamping {
  double lambda = 0.0, ni = 2.0;

  SIM3OPT_LM_HD void start(double user_init, double tau, double maxdiag) {  // lambda_0: the user's, else tau * max |H_dd|
    lambda = user_init > 0 ? user_init : tau * maxdiag;
    ni = 2.0;
  }

  // One trial, scale = x.(lambda x + b): sets the gain ratio rho, returns whether the step is accepted
  SIM3OPT_LM_HD bool update(double chi_old, double chi_new, double scale, double lower, double upper, double& rho) {
    rho = chi_old - chi_new;
    scale += 1e-3;
    rho /= scale;
    if (rho > 0 && std::isfinite(chi_new)) {
      double alpha = 1.0 - std::pow(2 * rho - 1, 3);
      alpha = std::min(alpha, upper);
      lambda *= std::max(lower, alpha);
      ni = 2.0;
      return true;
    }
    lambda *= ni;
    ni *= 2.0;
    return false;
  }

  // Terminate, after an iteration of `trials` trials, the last with gain ratio rho
  SIM3OPT_LM_HD bool terminate(int trials, int max_trials, double rho) const {
    return trials == max_trials || rho == 0 || !std::isfinite(lambda);
  }
};

}  // namespace sim3opt
