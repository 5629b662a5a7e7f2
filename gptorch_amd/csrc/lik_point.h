// The point functions of the non-Gaussian likelihoods -- ONE definition shared by the Gauss-Hermite expectation (lik.hip),
// the derivatives of LaplaceGP's Newton steps (laplace.hip) and, built on them, EPGP's tilted moments (ep.hip).
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

// ---- expectation propagation (ep.hip): the tilted distribution p(y | f) N(f | mu_c, v_c) of one point ----------------------------
// What a site update needs, in forms that neither cancel nor divide by a site parameter (t = 2y - 1, tau_c = 1 / v_c):
//   lz = log Z^,  mu_hat, s2_hat (> 0 for every finite input),
//   tau_full = 1 / s2_hat - tau_c  and  nu_full = mu_hat / s2_hat - mu_c tau_c, the sites that would match the moments.
struct EpMoments {
  double lz, mu_hat, s2_hat, tau_full, nu_full;
};

constexpr int EP_MILLS_TERMS = 200;       // continued-fraction levels of the left tail (converged to 1e-17 at z = -1.5)
constexpr double EP_MILLS_FROM = -1.5;    // z below which z + phi / Phi comes from the continued fraction

// probit (R&W eqs. 3.58 and 3.82): z = t mu_c / sqrt(1 + v_c), r = phi(z) / Phi(z), D = z + r, w = r D in (0, 1), h = 1 + z D;
//   mu_hat = mu_c + t v_c r / sqrt(1 + v_c),   s2_hat = v_c (1 + v_c (1 - w)) / (1 + v_c),
//   tau_full = w / (1 + v_c (1 - w)),          nu_full = t r h sqrt(1 + v_c) / (1 + v_c (1 - w))      (= mu_hat tau_full + t r / sqrt(1 + v_c),
//                                                                                                     which cancels for a point far on the wrong side).
// In the left tail r ~ -z and D, 1 - w, h are differences of large numbers; there they come from Laplace's continued fraction of
// the Mills ratio, 1 / r = 1 / (x + 1 / (x + 2 / (x + 3 / ...))) with x = -z:
//   D = 1 / (x + E),  E = 2 / (x + 3 / (x + ...)),  h = 1 - x D = E D,  1 - w = D (E - D),  t mu_hat = (D v_c - x) / sqrt(1 + v_c)
// (every term positive but the last, which is small only where mu_hat is).  log Phi and r themselves: lik_point's erfcx branch.
__device__ inline EpMoments ep_moments_probit(double t, double mu_c, double v_c) {
  const double d = 1.0 + v_c, rs = 1.0 / sqrt(d), z = t * mu_c * rs;
  const LikConst none = {0.0, 0.0, 0.0};
  double lp, r, dpar;
  lik_point<GPN_LIK_PROBIT>(none, z, 0.0, 1.0, lp, r, dpar);
  EpMoments m;
  double w, omw, h;
  if (z < EP_MILLS_FROM) {
    const double x = -z;
    double e = 0.0;
    for (int k = EP_MILLS_TERMS; k >= 2; --k) e = (double)k / (x + e);
    const double D = 1.0 / (x + e);
    r = x + D;
    w = r * D;
    omw = D * (e - D);
    h = e * D;
    m.mu_hat = t * (D * v_c - x) * rs;
  } else {
    const double D = z + r;
    w = r * D;
    omw = 1.0 - w;
    h = 1.0 + z * D;
    m.mu_hat = mu_c + v_c * (t * r * rs);
  }
  const double q = 1.0 + v_c * omw;
  m.lz = lp;
  m.s2_hat = v_c * q / d;
  m.tau_full = w / q;
  m.nu_full = t * r * h / (rs * q);
  return m;
}

// logit: the three moments by the H-node Gauss-Hermite rule (physicists' nodes x_h, weights w_h), f_h = mu_c + sqrt(2 v_c) x_h,
// g_h = w_h sigma(t f_h) / max_h sigma(t f_h) (log sigma: lik_point's overflow-free form; nothing underflows to a zero sum):
//   Z^ = pi^-1/2 sum g,  m1 = sum g u / sum g (u = sqrt 2 x),  m2 = sum g (u - m1)^2 / sum g > 0 (a second pass: no cancellation),
//   mu_hat = mu_c + sqrt(v_c) m1,  s2_hat = v_c m2,  tau_full = (1 - m2) / (m2 v_c),  nu_full = mu_hat tau_full + m1 / sqrt(v_c).
// nodes, weights: readable by every lane (LDS).
__device__ inline EpMoments ep_moments_logit(double t, double mu_c, double v_c, const double* nodes, const double* weights, int H) {
  const LikConst none = {0.0, 0.0, 0.0};
  const double sd = sqrt(v_c), step = sd * 1.41421356237309504880;
  double top = -1.0e300;
  for (int h = 0; h < H; ++h) top = fmax(top, t * nodes[h]);
  double lmax, dlp, dpar;
  lik_point<GPN_LIK_LOGIT>(none, t * mu_c + step * top, 0.0, 1.0, lmax, dlp, dpar);
  double s0 = 0.0, s1 = 0.0;
  for (int h = 0; h < H; ++h) {
    double lp;
    lik_point<GPN_LIK_LOGIT>(none, t * (mu_c + step * nodes[h]), 0.0, 1.0, lp, dlp, dpar);
    const double g = weights[h] * exp(lp - lmax);
    s0 += g;
    s1 += g * nodes[h];
  }
  const double m1 = 1.41421356237309504880 * (s1 / s0);
  double s2 = 0.0, sm = 0.0;
  for (int h = 0; h < H; ++h) {
    double lp;
    lik_point<GPN_LIK_LOGIT>(none, t * (mu_c + step * nodes[h]), 0.0, 1.0, lp, dlp, dpar);
    const double g = weights[h] * exp(lp - lmax), c = 1.41421356237309504880 * nodes[h] - m1;
    s2 += g * (c * c);
    sm += g * (1.0 - c * c);
  }
  const double m2 = s2 / s0;
  EpMoments m;
  m.lz = lmax + log(s0 * LK_INV_SQRT_PI);
  m.mu_hat = mu_c + sd * m1;
  m.s2_hat = v_c * m2;
  m.tau_full = (sm / s2) / v_c;
  m.nu_full = m.mu_hat * m.tau_full + m1 / sd;
  return m;
}

}  // namespace gpn
