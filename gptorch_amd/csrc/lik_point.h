// The point functions of the non-Gaussian likelihoods -- ONE definition shared by the Gauss-Hermite expectation (lik.hip)
// and the derivatives of LaplaceGP's Newton steps (laplace.hip).
#pragma once
#include "gpn_common.h"

namespace gpn {

constexpr double LK_INV_SQRT_PI = 0.56418958354775628695;      // pi^-1/2
constexpr double LK_SQRT_2_OVER_PI = 0.79788456080286535588;   // sqrt(2 / pi)
constexpr double LK_INV_SQRT_2PI = 0.39894228040143267794;     // (2 pi)^-1/2
constexpr double LK_SQRT_HALF = 0.70710678118654752440;
constexpr double LK_PI = 3.14159265358979323846;

// what a kind needs once per thread
struct LikConst {
  double nu, s2, c;   // Student-t: df, scale^2, lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi s2) / 2
};

// logp(f, y), d logp / d f and d logp / d param at one point; r = y - f, formed by the caller as (y - mu) - sqrt(2 v) x_h (where
// the target is close to the mean, y - f rounded from f would lose what y - mu keeps exactly)
template <int KIND>
__device__ inline void lik_point(const LikConst& k, double f, double r, double y, double& lp, double& dlp, double& dpar) {
  dpar = 0.0;
  if (KIND == GPN_LIK_PROBIT) {
    // log Phi(z), z = (2y - 1) f, stable in both tails: z < 0 through the scaled complementary error function
    // (log Phi = log(erfcx(-z / sqrt 2) / 2) - z^2 / 2, phi / Phi = sqrt(2 / pi) / erfcx(-z / sqrt 2)), z >= 0 through log1p
    const double s = 2.0 * y - 1.0, z = s * f, t = z * LK_SQRT_HALF;
    double ratio;                                          // phi(z) / Phi(z)
    if (z < 0.0) {
      const double e = erfcx(-t);
      lp = log(0.5 * e) - 0.5 * z * z;
      ratio = LK_SQRT_2_OVER_PI / e;
    } else {
      const double c = 0.5 * erfc(t);
      lp = log1p(-c);
      ratio = exp(-0.5 * z * z) * LK_INV_SQRT_2PI / (1.0 - c);
    }
    dlp = s * ratio;
  } else if (KIND == GPN_LIK_LOGIT) {
    // log sigma(t) = min(t, 0) - log1p(exp(-|t|)), t = (2y - 1) f: nothing overflows at any |t|
    const double s = 2.0 * y - 1.0, t = s * f;
    const double e = exp(-fabs(t));
    lp = fmin(t, 0.0) - log1p(e);
    dlp = s * ((t >= 0.0 ? e : 1.0) / (1.0 + e));          // sigma(-t)
  } else {
    // Student-t: c - (nu + 1) / 2 log1p(r^2 / (nu s2)); param = s2
    const double q = k.nu * k.s2, rr = r * r;
    lp = k.c - 0.5 * (k.nu + 1.0) * log1p(rr / q);
    dlp = (k.nu + 1.0) * r / (q + rr);
    dpar = 0.5 * (k.nu + 1.0) * rr / (k.s2 * (q + rr)) - 0.5 / k.s2;
  }
}

}  // namespace gpn
