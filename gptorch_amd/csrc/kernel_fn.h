// The stationary kernels as functions of the scaled squared distance -- ONE definition of the formulas and ONE place where a
// run-time kind becomes a template argument:
//   kernel_of_r2  the assembly (kmat.hip), the refinement's residual pass (refine.hip), which must reproduce the assembled
//                 entries bit for bit, LaplaceGP's row sweeps (laplace.hip) and the expression leaves (kexpr.hip)
//   k_and_base    the gradient sweeps (grad.hip, laplace.hip, loo.hip, kexpr.hip)
//   with_kind     every host function of those files that launches a kernel instantiated per kind
#pragma once
#include <type_traits>
#include "gpn_common.h"

namespace gpn {

// f(std::integral_constant<int, KIND>{}) for the run-time kind; -2 (the kind's argument position in every entry point) for a
// kind that is not served: anything out of range, and GPN_SQDIST unless SQDIST_TOO (the assembly and the gradient sweeps have
// a SqDist instantiation, nothing that factors or solves against K does: kind_is_covariance, gpn_common.h).  f runs only for
// a served kind, so whatever it opens (a profile record) it also closes.
template <bool SQDIST_TOO = false, class F>
inline int with_kind(int kind, F&& f) {
  switch (kind) {
    case GPN_RBF: return f(std::integral_constant<int, GPN_RBF>{});
    case GPN_MATERN52: return f(std::integral_constant<int, GPN_MATERN52>{});
    case GPN_MATERN32: return f(std::integral_constant<int, GPN_MATERN32>{});
    case GPN_EXP: return f(std::integral_constant<int, GPN_EXP>{});
    case GPN_PERIODIC: return f(std::integral_constant<int, GPN_PERIODIC>{});
    case GPN_SQDIST:
      if constexpr (SQDIST_TOO) return f(std::integral_constant<int, GPN_SQDIST>{});
      else return -2;
    default: return -2;
  }
}

template <int KIND>
__device__ __forceinline__ double kernel_of_r2(double r2, double var) {
  if constexpr (KIND == GPN_SQDIST) {
    return r2;                                         // util.py:73-88 (lengthscale-scaled)
  } else if constexpr (KIND == GPN_RBF) {
    return var * exp(-0.5 * r2);                       // kernels.py:220-222
  } else {
    const double r = sqrt(fmax(r2, 1e-40));            // kernels.py:172
    if constexpr (KIND == GPN_MATERN52) {
      const double s5 = 2.23606797749978969641;        // sqrt(5), kernels.py:204-212
      return var * (1.0 + s5 * r + 5.0 / 3.0 * r * r) * exp(-s5 * r);
    } else if constexpr (KIND == GPN_MATERN32) {
      const double r3 = 1.73205080756887729353 * r;    // kernels.py:196-201
      return var * (1.0 + r3) * exp(-r3);
    } else if constexpr (KIND == GPN_PERIODIC) {
      return var * cos(r);                             // kernels.py:228-235
    } else {
      return var * exp(-r);                            // kernels.py:189-190
    }
  }
}

// K and the base B of its length-scale derivative, dK/d(ell_d) = B(r) s_d / ell_d with s_d = ((x_id - x_jd) / ell_d)^2 -- the
// gradient sweeps (grad.hip, laplace.hip)
template <int KIND>
__device__ __forceinline__ void k_and_base(double r2, double var, double& K, double& B) {
  if constexpr (KIND == GPN_RBF) {
    K = var * exp(-0.5 * r2);
    B = K;
  } else if constexpr (KIND == GPN_SQDIST) {
    // util.squared_distance itself (util.py:73-88): K = r^2, no variance.  B = -2 dK/d(r^2) = -2
    // everywhere, also at r = 0 (direct differences: nothing is clamped, so the second derivative
    // the reference guards with its detach() trick, test_util.py:78-106, is the plain 2)
    K = 0.0;
    B = -2.0;
  } else {
    const bool dead = r2 < 1e-40;                 // kernels.py:172 clamp: no gradient below it
    const double r = sqrt(fmax(r2, 1e-40));
    if constexpr (KIND == GPN_MATERN52) {
      const double s5 = 2.23606797749978969641;
      const double e = exp(-s5 * r);
      K = var * (1.0 + s5 * r + 5.0 / 3.0 * r * r) * e;
      B = dead ? 0.0 : var * (5.0 / 3.0) * (1.0 + s5 * r) * e;
    } else if constexpr (KIND == GPN_MATERN32) {
      const double s3 = 1.73205080756887729353;
      const double e = exp(-s3 * r);
      K = var * (1.0 + s3 * r) * e;
      B = dead ? 0.0 : 3.0 * var * e;
    } else if constexpr (KIND == GPN_PERIODIC) {
      K = var * cos(r);
      B = dead ? 0.0 : var * sin(r) / r;
    } else {
      const double e = exp(-r);
      K = var * e;
      B = dead ? 0.0 : var * e / r;
    }
  }
}

}  // namespace gpn
