// The expected log-likelihood of a non-Gaussian likelihood under Gaussian marginals (gptorch_amd/likelihoods.py; the data term of
// SVGP, sparse_gpr.py:276-283), by the Gauss-Hermite rule the reference's likelihoods.py names and leaves as a TODO:
//   value = sum_{i, k} pi^-1/2 sum_h w_h logp(f_ikh, y_ik),      f_ikh = mu_ik + sqrt(2 v_i) x_h
// with its EXACT derivatives (those of the discrete rule, not the second-derivative form of Opper & Archambeau):
//   g_mean_ik = pi^-1/2 sum_h w_h logp'(f_ikh)        g_var_i = sum_k pi^-1/2 sum_h w_h logp'(f_ikh) x_h / sqrt(2 v_i)
//   g_params  = sum_{i, k} pi^-1/2 sum_h w_h d logp / d param
// in ONE pass over the entries.  One thread per row: it walks the row's dy columns (they share v_i) and, per column, the H
// nodes, which the workgroup has staged in LDS (every lane reads the same address: a broadcast).  Poisson (log link) takes its
// closed form  y mu - exp(mu + v / 2) - lgamma(y + 1)  for the value and both gradients: no loop over the nodes.
// Sums in a fixed order -- a thread's own sequential sums, a shuffle tree per wavefront, the four wavefronts of a workgroup,
// per-workgroup partials in `work`, combined by a second single-workgroup launch -- and nothing is accumulated with atomics:
// the same inputs give the same bits.
#include "rowkernels.h"
#include "lik_point.h"

namespace gpn {

constexpr int LK_THREADS = GPN_LIK_ROWS_PER_GROUP;   // rows of a workgroup, one per thread
constexpr int LK_WAVES = LK_THREADS / 64;
constexpr int LK_MAX_H = 64;

template <int KIND>
__global__ __launch_bounds__(LK_THREADS) void lik_expect_kernel(const double* __restrict__ params, const double* __restrict__ f_mean,
                                                                int64_t ldf, const double* __restrict__ f_var,
                                                                const double* __restrict__ y, int64_t ldy, int64_t rows, int dy,
                                                                const double* __restrict__ nodes, const double* __restrict__ weights, int H,
                                                                double* __restrict__ g_mean, int64_t ldg, double* __restrict__ g_var,
                                                                double* __restrict__ partials) {
  __shared__ double xs[LK_MAX_H], ws[LK_MAX_H];
  __shared__ double red[LK_WAVES][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (KIND != GPN_LIK_POISSON) {
    if (tid < H) {
      xs[tid] = nodes[tid];
      ws[tid] = weights[tid];
    }
    __syncthreads();
  }
  LikConst k = {0.0, 0.0, 0.0};
  if (KIND == GPN_LIK_STUDENT_T) {
    k.nu = params[0];
    k.s2 = params[1];
    k.c = lgamma(0.5 * (k.nu + 1.0)) - lgamma(0.5 * k.nu) - 0.5 * log(k.nu * LK_PI * k.s2);
  }
  const int64_t row = (int64_t)blockIdx.x * LK_THREADS + tid;
  double val = 0.0, gpar = 0.0;
  if (row < rows) {
    const double v = f_var[row];
    double gv = 0.0;
    if (KIND == GPN_LIK_POISSON) {
      for (int c = 0; c < dy; ++c) {
        const double mu = f_mean[row * ldf + c], yy = y[row * ldy + c];
        const double m = exp(mu + 0.5 * v);
        val += yy * mu - m - lgamma(yy + 1.0);
        if (g_mean) g_mean[row * ldg + c] = yy - m;
        gv -= 0.5 * m;
      }
    } else {
      const double sd = sqrt(2.0 * v), inv = 1.0 / sd;      // (v < 0: NaN, as the sqrt of the torch route)
      for (int c = 0; c < dy; ++c) {
        const double mu = f_mean[row * ldf + c], yy = y[row * ldy + c], r0 = yy - mu;
        double a = 0.0, b = 0.0, cx = 0.0, d = 0.0;
#pragma unroll 1
        for (int h = 0; h < H; ++h) {
          const double x = xs[h], w = ws[h];
          double lp, dlp, dpar;
          lik_point<KIND>(k, fma(sd, x, mu), fma(-sd, x, r0), yy, lp, dlp, dpar);
          a = fma(w, lp, a);
          b = fma(w, dlp, b);
          cx = fma(w * x, dlp, cx);
          d = fma(w, dpar, d);
        }
        val += a * LK_INV_SQRT_PI;
        if (g_mean) g_mean[row * ldg + c] = b * LK_INV_SQRT_PI;
        gv += cx * LK_INV_SQRT_PI * inv;
        gpar += d * LK_INV_SQRT_PI;
      }
    }
    if (g_var) g_var[row] = gv;
  }
  val = wave_sum(val);
  gpar = wave_sum(gpar);
  if (lane == 0) {
    red[wave][0] = val;
    red[wave][1] = gpar;
  }
  __syncthreads();
  if (tid == 0) {
    partials[2 * (int64_t)blockIdx.x] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    partials[2 * (int64_t)blockIdx.x + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
  }
}

// second stage: the sums of the workgroups' partial pairs in a fixed order (one workgroup) -> value[0], g_params[0 .. 1]
__global__ __launch_bounds__(256) void lik_sum_partials_kernel(const double* __restrict__ partials, int64_t count, double* __restrict__ value,
                                                               double* __restrict__ g_params) {
  __shared__ double red[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) {
    a += partials[2 * i];
    b += partials[2 * i + 1];
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane == 0) {
    red[wave][0] = a;
    red[wave][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (value) value[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    if (g_params) {
      g_params[0] = 0.0;                                   // (params[0], Student-t's df, is a fixed shape parameter)
      g_params[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    }
  }
}

static_assert(LK_WAVES == 4, "the workgroup's partials are combined as (w0 + w1) + (w2 + w3)");

}  // namespace gpn

using namespace gpn;

extern "C" int gpn_lik_expect(void* stream, int kind, const double* params, const double* f_mean, int64_t ldf, const double* f_var,
                              const double* y, int64_t ldy, int64_t rows, int dy, const double* nodes, const double* weights, int H,
                              double* work, int64_t work_bytes, double* value, double* g_mean, int64_t ldg, double* g_var,
                              double* g_params) {
  if (kind < GPN_LIK_PROBIT || kind > GPN_LIK_STUDENT_T) return -2;
  if (kind == GPN_LIK_STUDENT_T && !params) return -3;
  if (!f_mean) return -4;
  if (!f_var) return -6;
  if (!y) return -7;
  if (rows <= 0) return -9;
  if (dy <= 0) return -10;
  if (ldf < dy) return -5;
  if (ldy < dy) return -8;
  if (kind != GPN_LIK_POISSON) {
    if (!nodes) return -11;
    if (!weights) return -12;
    if (H < 1 || H > LK_MAX_H) return -13;
  }
  if (!work) return -14;
  const int64_t blocks = (rows + LK_THREADS - 1) / LK_THREADS;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  if (work_bytes < 2 * 8 * blocks) return -15;
  if (g_mean && ldg < dy) return -18;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)blocks), block(LK_THREADS);
#define GPN_LIK_LAUNCH(K) \
  hipLaunchKernelGGL(lik_expect_kernel<K>, grid, block, 0, s, params, f_mean, ldf, f_var, y, ldy, rows, dy, nodes, weights, H, g_mean, ldg, \
                     g_var, work)
  switch (kind) {
    case GPN_LIK_PROBIT: GPN_LIK_LAUNCH(GPN_LIK_PROBIT); break;
    case GPN_LIK_LOGIT: GPN_LIK_LAUNCH(GPN_LIK_LOGIT); break;
    case GPN_LIK_POISSON: GPN_LIK_LAUNCH(GPN_LIK_POISSON); break;
    default: GPN_LIK_LAUNCH(GPN_LIK_STUDENT_T); break;
  }
#undef GPN_LIK_LAUNCH
  GPN_LAUNCH_CHECK();
  if (value || g_params) {
    hipLaunchKernelGGL(lik_sum_partials_kernel, dim3(1), dim3(256), 0, s, work, blocks, value, g_params);
    GPN_LAUNCH_CHECK();
  }
  return GPN_OK;
}
