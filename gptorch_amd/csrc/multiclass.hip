// The robust-max likelihood of multi-class classification under Gaussian marginals (likelihoods.MultiClass; the data term and
// the predictive probabilities of SVGP with C latent columns).  C classes, a label y per row, one variance v per row shared by the
// row's C means mu_c, the H <= 64 physicists' Gauss-Hermite nodes x_h and weights w_h:
//   z_hc = (mu_y - mu_c) / sqrt(v) + sqrt(2) x_h  (c != y),   T_h = exp(sum_{c != y} log Phi(z_hc)),   P = pi^-1/2 sum_h w_h T_h
//   value = sum_rows [ P log(1 - eps) + (1 - P) log(eps / (C - 1)) ]
// and the exact derivatives of that discrete rule, D = log(1 - eps) - log(eps / (C - 1)), r = phi / Phi:
//   g_mean_c = -D pi^-1/2 / sqrt(v) sum_h w_h T_h r(z_hc)  (c != y),   g_mean_y = -sum_{c != y} g_mean_c
//   g_var    = -D pi^-1/2 / (2 v^(3/2)) sum_{c != y} (mu_y - mu_c) sum_h w_h T_h r(z_hc)
// ONE WAVEFRONT PER ROW, node h on lane h (H <= 64 = the lanes of a wavefront).  Pass one: lane h adds log Phi over the classes
// (the row's means: every lane reads the same address, a broadcast) and a shuffle tree over the lanes gives P.  Pass two, per
// class: the hazard again (nothing of size C is kept in registers) and a shuffle tree gives the class's gradient, which lane 0
// stores.  log Phi and the hazard are lik_point.h's probit point function (erfcx for z < 0): neither a product of underflowing
// Phi nor a quotient of two zeros appears; a lane whose T_h underflowed to 0 adds an exact 0.
// Sums in a fixed order -- a lane's own sum over the classes, the shuffle tree, the four rows of a workgroup as
// (r0 + r1) + (r2 + r3), per-workgroup partials in `work`, a second single-workgroup launch -- and no atomics: the same inputs
// give the same bits.
#include <math.h>
#include "rowkernels.h"
#include "lik_point.h"

namespace gpn {

constexpr int RM_WAVES = GPN_ROBUSTMAX_ROWS_PER_GROUP;   // rows of a workgroup, one per wavefront
constexpr int RM_THREADS = 64 * RM_WAVES;
constexpr int RM_MAX_H = 64;
constexpr double RM_SQRT_2 = 1.41421356237309504880;

// log Phi(z) and phi(z) / Phi(z), stable in both tails
__device__ inline void log_ndtr_hazard(double z, double& lp, double& r) {
  const LikConst none = {0.0, 0.0, 0.0};
  double dpar;
  lik_point<GPN_LIK_PROBIT>(none, z, 0.0, 1.0, lp, r, dpar);
}

// w_h prod_{c != k} Phi((mu_k - mu_c) rs + sx) on lane h (sx = sqrt(2) x_h; w = 0 on the lanes beyond H)
__device__ inline double weighted_product(const double* __restrict__ mu, int C, int k, double rs, double sx, double w, bool on) {
  const double muk = mu[k];
  double s = 0.0;
  for (int c = 0; c < C; ++c) {
    if (c == k) continue;
    double lp, r;
    log_ndtr_hazard(fma(muk - mu[c], rs, sx), lp, r);
    s += lp;
  }
  return on ? w * exp(s) : 0.0;
}

__global__ __launch_bounds__(RM_THREADS) void robustmax_expect_kernel(const double* __restrict__ f_mean, int64_t ldf,
                                                                      const double* __restrict__ f_var, const double* __restrict__ labels,
                                                                      int64_t rows, int C, double log_hit, double log_miss,
                                                                      const double* __restrict__ nodes, const double* __restrict__ weights,
                                                                      int H, double* __restrict__ g_mean, int64_t ldg,
                                                                      double* __restrict__ g_var, double* __restrict__ partials) {
  __shared__ double red[RM_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool on = lane < H;
  const double sx = on ? RM_SQRT_2 * nodes[lane] : 0.0, w = on ? weights[lane] : 0.0;
  const int64_t row = (int64_t)blockIdx.x * RM_WAVES + wave;           // (uniform over the wavefront, as every branch below)
  const double delta = log_hit - log_miss;
  double val = 0.0;
  if (row < rows) {
    const double* mu = f_mean + row * ldf;
    const double v = f_var[row], yl = labels[row];
    if (!(yl >= 0.0 && yl < (double)C && yl == floor(yl))) {           // no class (NaN included): NaN out, nothing read at it
      val = NAN;
      if (g_mean)
        for (int c = lane; c < C; c += 64) g_mean[row * ldg + c] = NAN;
      if (g_var && lane == 0) g_var[row] = NAN;
    } else {
      const int y = (int)yl;
      const double rs = v > 0.0 ? 1.0 / sqrt(v) : NAN;
      const double wT = weighted_product(mu, C, y, rs, sx, w, on);
      const double P = LK_INV_SQRT_PI * wave_sum_all(wT);
      val = P * log_hit + (1.0 - P) * log_miss;
      if (g_mean || g_var) {
        const double muy = mu[y], coef = -delta * LK_INV_SQRT_PI * rs;
        double gy = 0.0, gv = 0.0;
        for (int c = 0; c < C; ++c) {
          if (c == y) continue;
          const double d = muy - mu[c];
          double lp, r;
          log_ndtr_hazard(fma(d, rs, sx), lp, r);
          const double sum = wave_sum(wT == 0.0 ? 0.0 : wT * r);       // (lane 0 holds it)
          const double g = coef * sum;
          if (g_mean && lane == 0) g_mean[row * ldg + c] = g;
          gy -= g;
          gv = fma(sum, d, gv);
        }
        if (lane == 0) {
          if (g_mean) g_mean[row * ldg + y] = gy;
          if (g_var) g_var[row] = (0.5 * coef * (rs * rs)) * gv;
        }
      }
    }
  }
  if (lane == 0) red[wave] = val;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

static_assert(RM_WAVES == 4, "the workgroup's rows are combined as (r0 + r1) + (r2 + r3)");

// second stage: the workgroups' partials in a fixed order (one workgroup) -> value[0]
__global__ __launch_bounds__(256) void robustmax_sum_partials_kernel(const double* __restrict__ partials, int64_t count,
                                                                     double* __restrict__ value) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) a += partials[i];
  a = wave_sum(a);
  if (lane == 0) red[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) value[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// probs[row, k] = hit P_k + miss (1 - P_k), P_k = pi^-1/2 sum_h w_h prod_{c != k} Phi(z_hc) with class k in the label's place
__global__ __launch_bounds__(RM_THREADS) void robustmax_probs_kernel(const double* __restrict__ f_mean, int64_t ldf,
                                                                     const double* __restrict__ f_var, int64_t rows, int C, double hit,
                                                                     double miss, const double* __restrict__ nodes,
                                                                     const double* __restrict__ weights, int H, double* __restrict__ probs,
                                                                     int64_t ldp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool on = lane < H;
  const double sx = on ? RM_SQRT_2 * nodes[lane] : 0.0, w = on ? weights[lane] : 0.0;
  const int64_t row = (int64_t)blockIdx.x * RM_WAVES + wave;
  if (row >= rows) return;
  const double* mu = f_mean + row * ldf;
  const double v = f_var[row];
  const double rs = v > 0.0 ? 1.0 / sqrt(v) : NAN;
  for (int k = 0; k < C; ++k) {
    const double P = LK_INV_SQRT_PI * wave_sum(weighted_product(mu, C, k, rs, sx, w, on));
    if (lane == 0) probs[row * ldp + k] = hit * P + miss * (1.0 - P);
  }
}

}  // namespace gpn

using namespace gpn;

extern "C" int gpn_lik_expect_robustmax(void* stream, const double* f_mean, int64_t ldf, const double* f_var, const double* labels,
                                        int64_t rows, int num_classes, double eps, const double* nodes, const double* weights, int H,
                                        double* work, int64_t work_bytes, double* value, double* g_mean, int64_t ldg, double* g_var) {
  if (!f_mean) return -2;
  if (!f_var) return -4;
  if (!labels) return -5;
  if (rows <= 0) return -6;
  if (num_classes < 2) return -7;
  if (ldf < num_classes) return -3;
  if (!(eps > 0.0 && eps < 1.0)) return -8;
  if (!nodes) return -9;
  if (!weights) return -10;
  if (H < 1 || H > RM_MAX_H) return -11;
  if (!work) return -12;
  const int64_t blocks = (rows + RM_WAVES - 1) / RM_WAVES;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  if (work_bytes < 8 * blocks) return -13;
  if (g_mean && ldg < num_classes) return -16;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const double log_hit = log1p(-eps), log_miss = log(eps / (double)(num_classes - 1));
  hipLaunchKernelGGL(robustmax_expect_kernel, dim3((unsigned)blocks), dim3(RM_THREADS), 0, s, f_mean, ldf, f_var, labels, rows, num_classes,
                     log_hit, log_miss, nodes, weights, H, g_mean, ldg, g_var, work);
  GPN_LAUNCH_CHECK();
  if (value) {
    hipLaunchKernelGGL(robustmax_sum_partials_kernel, dim3(1), dim3(256), 0, s, work, blocks, value);
    GPN_LAUNCH_CHECK();
  }
  return GPN_OK;
}

extern "C" int gpn_lik_robustmax_probs(void* stream, const double* f_mean, int64_t ldf, const double* f_var, int64_t rows, int num_classes,
                                       double eps, const double* nodes, const double* weights, int H, double* probs, int64_t ldp) {
  if (!f_mean) return -2;
  if (!f_var) return -4;
  if (rows <= 0) return -5;
  if (num_classes < 2) return -6;
  if (ldf < num_classes) return -3;
  if (!(eps > 0.0 && eps < 1.0)) return -7;
  if (!nodes) return -8;
  if (!weights) return -9;
  if (H < 1 || H > RM_MAX_H) return -10;
  if (!probs) return -11;
  if (ldp < num_classes) return -12;
  const int64_t blocks = (rows + RM_WAVES - 1) / RM_WAVES;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  hipLaunchKernelGGL(robustmax_probs_kernel, dim3((unsigned)blocks), dim3(RM_THREADS), 0, static_cast<hipStream_t>(stream), f_mean, ldf,
                     f_var, rows, num_classes, 1.0 - eps, eps / (double)(num_classes - 1), nodes, weights, H, probs, ldp);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}
