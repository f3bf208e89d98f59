// robust.hpp -- the per-edge robust kernels (g2o RobustKernel*::robustify, robust_kernel_impl.cpp), host + device.
//
// robustify(kind, delta, e2, rho, w) returns rho(e2) and w = rho'(e2) of the edge's kernel at e2 = e^T Omega e
// (d = delta below):
//
//   kind               rho(e2)                                         w = rho'(e2)
//   0 NONE             e2                                              1
//   1 HUBER            e2 <= d^2: e2;  else 2 d sqrt(e2) - d^2          1;  d / sqrt(e2)
//   2 PSEUDO_HUBER     2 d^2 (sqrt(1 + e2/d^2) - 1)                    1 / sqrt(1 + e2/d^2)
//   3 CAUCHY           d^2 log(1 + e2/d^2)                             1 / (1 + e2/d^2)
//   4 GEMAN_MCCLURE    d e2 / (d + e2)                                 d^2 / (d + e2)^2
//   5 WELSCH           d^2 (1 - exp(-e2/d^2))                          exp(-e2/d^2)
//   6 FAIR             2 d^2 (a - log(1 + a)),  a = sqrt(e2) / d       1 / (1 + a)
//   7 TUKEY            e2 <= d^2: d^2/3 (1 - (1 - e2/d^2)^3); else d^2/3   (1 - e2/d^2)^2;  0
//   8 SATURATED        e2 <= d^2: e2;  else d^2                        1;  0
//   9 DCS              s = 2d / (d + e2);  s >= 1: e2;  else s^2 e2    1;  s^2
//
// Geman-McClure and DCS take delta unsquared, as g2o does; DCS's rho is not the integral of its w (g2o's
// definition, kept).  Only first-order terms are used, as in g2o: an edge contributes w J^T Omega J and
// -w J^T Omega e, the chi2 sums rho, rho'' is ignored.  huber() is the arithmetic the Huber-only engine ran
// (same operations, same order): a Huber edge gives the same bits through robustify().
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sim3opt.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RK_HD __host__ __device__ __forceinline__
#else
#define RK_HD inline
#endif

namespace sim3opt {

constexpr int ROBUST_KINDS = 10;  // SIM3OPT_KERNEL_NONE .. SIM3OPT_KERNEL_DCS

// g2o RobustKernelHuber: rho(e2) and rho'(e2)
RK_HD void huber(double e2, double delta, double& rho, double& w) {
  const double dsqr = delta * delta;
  if (e2 <= dsqr) {
    rho = e2;
    w = 1.0;
  } else {
    const double sq = sqrt(e2);
    rho = 2 * sq * delta - dsqr;
    w = delta / sq;
  }
}

RK_HD void robustify(int kind, double delta, double e2, double& rho, double& w) {
  const double dsqr = delta * delta;
  switch (kind) {
    case SIM3OPT_KERNEL_HUBER:
      huber(e2, delta, rho, w);
      break;
    case SIM3OPT_KERNEL_PSEUDO_HUBER: {
      const double r = sqrt(1.0 + e2 / dsqr);
      rho = 2.0 * dsqr * (r - 1.0);
      w = 1.0 / r;
      break;
    }
    case SIM3OPT_KERNEL_CAUCHY: {
      const double a = 1.0 + e2 / dsqr;
      rho = dsqr * log(a);
      w = 1.0 / a;
      break;
    }
    case SIM3OPT_KERNEL_GEMAN_MCCLURE: {
      const double a = delta + e2;
      rho = delta * e2 / a;
      w = dsqr / (a * a);
      break;
    }
    case SIM3OPT_KERNEL_WELSCH: {
      const double x = exp(-e2 / dsqr);
      rho = dsqr * (1.0 - x);
      w = x;
      break;
    }
    case SIM3OPT_KERNEL_FAIR: {
      const double a = sqrt(e2) / delta;
      rho = 2.0 * dsqr * (a - log(1.0 + a));
      w = 1.0 / (1.0 + a);
      break;
    }
    case SIM3OPT_KERNEL_TUKEY:
      if (e2 <= dsqr) {
        const double a = 1.0 - e2 / dsqr;
        rho = dsqr / 3.0 * (1.0 - a * a * a);
        w = a * a;
      } else {
        rho = dsqr / 3.0;
        w = 0.0;
      }
      break;
    case SIM3OPT_KERNEL_SATURATED:
      if (e2 <= dsqr) {
        rho = e2;
        w = 1.0;
      } else {
        rho = dsqr;
        w = 0.0;
      }
      break;
    case SIM3OPT_KERNEL_DCS: {
      const double s = 2.0 * delta / (delta + e2);
      if (s >= 1.0) {
        rho = e2;
        w = 1.0;
      } else {
        const double s2 = s * s;
        rho = s2 * e2;
        w = s2;
      }
      break;
    }
    default:  // SIM3OPT_KERNEL_NONE
      rho = e2;
      w = 1.0;
  }
}

}  // namespace sim3opt
