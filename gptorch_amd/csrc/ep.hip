// EPGP (gptorch_amd/models/ep.py): the per-point half of one parallel EP sweep -- cavity, tilted moments, damped site update,
// the site part of the evidence and the stopping statistics, in ONE launch pair with no host work in between.  (The reference has
// no non-conjugate model, likelihoods.py:47-78: nothing here restates reference code.)  Everything else of a sweep is the
// factorisation pipeline and laplace.hip's kernels with the site precisions in the place of W.
//
//   ep_sites_kernel     one point per thread.  From the posterior marginal (mu_i, sigma2_i) and the site (tau_i, nu_i):
//                         cavity    tau_c = 1 / sigma2 - tau,  nu_c = mu / sigma2 - nu,  mu_c = nu_c / tau_c,  v_c = 1 / tau_c
//                         moments   lik_point.h ep_moments_probit (closed form) / ep_moments_logit (the Gauss-Hermite rule)
//                         update    tau <- max(tau + rho (tau_full - tau), 0),  nu <- nu + rho (nu_full - nu)      (unless moments_only)
//                         evidence  e_i = log Z^ + 1/2 log1p(tau / tau_c) + 1/2 (tau_c c (tau c - 2 w) - w^2) / (tau_c + tau),
//                                   c = mu_c - m_i, w = nu - tau m_i: R&W eqs. 3.73-3.74's site terms; nothing divides by tau
//                       and the workgroup's six statistics (two sums, four maxima) into its slot of the workspace.
//   ep_stats_kernel     one workgroup adds / maximises the workgroups' slots.
//   ep_sites_batched_kernel / ep_stats_batched_kernel     the same two bodies (ep_sites_body, ep_stats_body) for `batch` equal-length
//                       models (models/_ep_lockstep.py), the model on blockIdx.y, its operands at a stride and its own damping from a
//                       device array: the same points per thread and workgroup, the same trees, the same order over its own slots --
//                       row b carries the bits of gpn_ep_sites on model b alone.
// Sums and maxima: a thread's own value, the wavefront's shuffle tree, the four wavefronts as (w0 + w1) + (w2 + w3), then the
// workgroups' slots in a fixed strided order and the same tree -- no atomics, the same call twice gives the same bits.  A NaN
// wins every maximum, so that a non-finite input cannot pass the stopping rule.
// Block shape: 256 threads (four wavefronts), 1 KiB of LDS for the rule and 48 bytes for the tree; the kernel is bound by the
// fp64 special functions of n points, a vanishing part of a sweep whose factorisation costs n^3 / 3.
#include "lik_point.h"
#include "rowkernels.h"

namespace gpn {

constexpr int EP_THREADS = 256;
constexpr int EP_NSTATS = GPN_EP_NSTATS;
constexpr int EP_MAX_H = 64;      // the rule staged in LDS (likelihoods.MAX_GAUSS_HERMITE_POINTS)

__device__ inline double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

__device__ inline double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_down(v, off, 64));
  return v;
}

// the six statistics of a workgroup's threads -> out[k * stride], k < 6 (thread 0 writes)
__device__ __forceinline__ void ep_block_stats(double (&v)[EP_NSTATS], double* __restrict__ out, int64_t stride) {
  __shared__ double red[EP_NSTATS][EP_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < EP_NSTATS; ++k) {
    const double r = k < 2 ? wave_sum(v[k]) : wave_max(v[k]);
    if (lane == 0) red[k][wave] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < EP_NSTATS; ++k)
      out[k * stride] = k < 2 ? (red[k][0] + red[k][1]) + (red[k][2] + red[k][3])
                              : nan_max(nan_max(red[k][0], red[k][1]), nan_max(red[k][2], red[k][3]));
  }
}

static_assert(EP_THREADS == 256, "the workgroup's statistics are combined as (w0, w1), (w2, w3)");

struct EpArgs {
  const double* y;
  const double* m;          // the prior mean at the points (nullptr: zero)
  const double* mu;
  const double* sigma2;
  const double* tau;        // (tau_out / nu_out may be the same memory: a thread reads its point before it writes it)
  const double* nu;
  const double* nodes;
  const double* weights;
  double* tau_out;
  double* nu_out;
  double* lz;
  double* mu_hat;
  double* s2_hat;
  double* partials;         // [6][gridDim.x]
  double damping;
  int64_t n;
  int H, moments_only;
};

// one workgroup's points of ONE model: the body of both ep_sites_kernel and ep_sites_batched_kernel (p: that model's operands)
template <int KIND>
__device__ __forceinline__ void ep_sites_body(const EpArgs& p) {
  __shared__ double rule[2][EP_MAX_H];
  const int tid = threadIdx.x;
  if (KIND == GPN_LIK_LOGIT) {
    if (tid < p.H) {
      rule[0][tid] = p.nodes[tid];
      rule[1][tid] = p.weights[tid];
    }
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * EP_THREADS + tid;
  double st[EP_NSTATS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < p.n) {
    const double t = 2.0 * p.y[i] - 1.0, mi = p.m ? p.m[i] : 0.0;
    const double prec = 1.0 / p.sigma2[i], tau = p.tau[i], nu = p.nu[i];
    const double tau_c = prec - tau, nu_c = p.mu[i] * prec - nu;
    const double v_c = 1.0 / tau_c, mu_c = nu_c * v_c;
    const EpMoments mo = KIND == GPN_LIK_PROBIT ? ep_moments_probit(t, mu_c, v_c) : ep_moments_logit(t, mu_c, v_c, rule[0], rule[1], p.H);
    const double c = mu_c - mi, w = nu - tau * mi;
    const double site = mo.lz + 0.5 * log1p(tau * v_c) + 0.5 * (tau_c * c * (tau * c - 2.0 * w) - w * w) / (tau_c + tau);
    const double dtau = mo.tau_full - tau, dnu = mo.nu_full - nu;
    double tau_n = tau, nu_n = nu;
    if (!p.moments_only) {
      tau_n = fmax(tau + p.damping * dtau, 0.0);
      nu_n = nu + p.damping * dnu;
      p.tau_out[i] = tau_n;
      p.nu_out[i] = nu_n;
    }
    if (p.lz) p.lz[i] = mo.lz;
    if (p.mu_hat) p.mu_hat[i] = mo.mu_hat;
    if (p.s2_hat) p.s2_hat[i] = mo.s2_hat;
    st[0] = mo.lz;
    st[1] = site;
    st[2] = fabs(dtau);
    st[3] = fabs(dnu);
    st[4] = fabs(tau_n);
    st[5] = fabs(nu_n);
  }
  ep_block_stats(st, p.partials + blockIdx.x, gridDim.x);
}

// one model's workgroup slots [6][blocks] -> its six statistics: the body of both stats kernels
__device__ __forceinline__ void ep_stats_body(const double* __restrict__ partials, int64_t blocks, double* __restrict__ stats) {
  double st[EP_NSTATS];
#pragma unroll
  for (int k = 0; k < EP_NSTATS; ++k) {
    double a = 0.0;
    for (int64_t j = threadIdx.x; j < blocks; j += EP_THREADS) a = k < 2 ? a + partials[k * blocks + j] : nan_max(a, partials[k * blocks + j]);
    st[k] = a;
  }
  ep_block_stats(st, stats, 1);
}

template <int KIND>
__global__ __launch_bounds__(EP_THREADS) void ep_sites_kernel(EpArgs p) {
  ep_sites_body<KIND>(p);
}

__global__ __launch_bounds__(EP_THREADS) void ep_stats_kernel(const double* __restrict__ partials, int64_t blocks, double* __restrict__ stats) {
  ep_stats_body(partials, blocks, stats);
}

// ... for `batch` equal-length models, blockIdx.y the model: p holds model 0's operands, every stacked operand of model b lies
// b * n further on (y: b * sy, sy = 0 shared), its slots b * 6 * gridDim.x, its damping at dampings[b]
template <int KIND>
__global__ __launch_bounds__(EP_THREADS) void ep_sites_batched_kernel(EpArgs p, const double* __restrict__ dampings, int64_t sy) {
  const int64_t b = blockIdx.y, at = b * p.n;
  p.y += b * sy;
  if (p.m) p.m += at;
  p.mu += at, p.sigma2 += at, p.tau += at, p.nu += at;
  if (!p.moments_only) p.tau_out += at, p.nu_out += at;
  if (p.lz) p.lz += at;
  if (p.mu_hat) p.mu_hat += at;
  if (p.s2_hat) p.s2_hat += at;
  p.partials += b * EP_NSTATS * (int64_t)gridDim.x;
  p.damping = dampings[b];
  ep_sites_body<KIND>(p);
}

__global__ __launch_bounds__(EP_THREADS) void ep_stats_batched_kernel(const double* __restrict__ partials, int64_t blocks, double* __restrict__ stats) {
  const int64_t b = blockIdx.y;
  ep_stats_body(partials + b * EP_NSTATS * blocks, blocks, stats + b * EP_NSTATS);
}

}  // namespace gpn

using namespace gpn;

extern "C" int64_t gpn_ep_sites_work_bytes(int64_t n) {
  if (n <= 0) return 0;
  return EP_NSTATS * ((n + EP_THREADS - 1) / EP_THREADS) * (int64_t)sizeof(double);
}

extern "C" int gpn_ep_sites(void* stream, int kind, int64_t n, const double* y, const double* m, const double* mu, const double* sigma2,
                            const double* tau, const double* nu, double damping, const double* nodes, const double* weights, int H,
                            int moments_only, double* work, int64_t work_bytes, double* tau_out, double* nu_out, double* lz,
                            double* mu_hat, double* s2_hat, double* stats) {
  if (kind < GPN_LIK_PROBIT || kind > GPN_LIK_STUDENT_T) return -2;
  if (kind != GPN_LIK_PROBIT && kind != GPN_LIK_LOGIT) return GPN_E_UNSUPPORTED;
  if (n <= 0) return -3;
  if (!y) return -4;
  if (!mu) return -6;
  if (!sigma2) return -7;
  if (!tau) return -8;
  if (!nu) return -9;
  if (!(damping > 0.0 && damping <= 1.0)) return -10;
  if (kind == GPN_LIK_LOGIT) {
    if (!nodes) return -11;
    if (!weights) return -12;
    if (H < 2 || H > EP_MAX_H) return -13;      // (one node has no second moment)
  }
  if (!work) return -15;
  const int64_t blocks = (n + EP_THREADS - 1) / EP_THREADS;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  if (work_bytes < gpn_ep_sites_work_bytes(n)) return -16;
  if (!moments_only && !tau_out) return -17;
  if (!moments_only && !nu_out) return -18;
  if (!stats) return -22;
  hipStream_t s = static_cast<hipStream_t>(stream);
  EpArgs p;
  p.y = y, p.m = m, p.mu = mu, p.sigma2 = sigma2, p.tau = tau, p.nu = nu, p.nodes = nodes, p.weights = weights;
  p.tau_out = tau_out, p.nu_out = nu_out, p.lz = lz, p.mu_hat = mu_hat, p.s2_hat = s2_hat, p.partials = work;
  p.damping = damping, p.n = n, p.H = H, p.moments_only = moments_only;
  if (kind == GPN_LIK_PROBIT) hipLaunchKernelGGL(ep_sites_kernel<GPN_LIK_PROBIT>, dim3((unsigned)blocks), dim3(EP_THREADS), 0, s, p);
  else hipLaunchKernelGGL(ep_sites_kernel<GPN_LIK_LOGIT>, dim3((unsigned)blocks), dim3(EP_THREADS), 0, s, p);
  GPN_LAUNCH_CHECK();
  hipLaunchKernelGGL(ep_stats_kernel, dim3(1), dim3(EP_THREADS), 0, s, work, blocks, stats);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}

extern "C" int64_t gpn_ep_sites_batched_work_bytes(int64_t n, int batch) {
  if (batch <= 0) return 0;
  return batch * gpn_ep_sites_work_bytes(n);
}

extern "C" int gpn_ep_sites_batched(void* stream, int kind, int batch, int64_t n, const double* y, int64_t sy, const double* m,
                                    const double* mu, const double* sigma2, const double* tau, const double* nu, const double* dampings,
                                    const double* nodes, const double* weights, int H, int moments_only, double* work, int64_t work_bytes,
                                    double* tau_out, double* nu_out, double* lz, double* mu_hat, double* s2_hat, double* stats) {
  if (kind < GPN_LIK_PROBIT || kind > GPN_LIK_STUDENT_T) return -2;
  if (kind != GPN_LIK_PROBIT && kind != GPN_LIK_LOGIT) return GPN_E_UNSUPPORTED;
  if (batch <= 0) return -3;
  if (batch > 65535) return GPN_E_UNSUPPORTED;      // (a grid dimension)
  if (n <= 0) return -4;
  if (!y) return -5;
  if (sy != 0 && sy != n) return -6;
  if (!mu) return -8;
  if (!sigma2) return -9;
  if (!tau) return -10;
  if (!nu) return -11;
  if (!dampings) return -12;                        // (their values live on the device: the caller's to keep in (0, 1])
  if (kind == GPN_LIK_LOGIT) {
    if (!nodes) return -13;
    if (!weights) return -14;
    if (H < 2 || H > EP_MAX_H) return -15;
  }
  if (!work) return -17;
  const int64_t blocks = (n + EP_THREADS - 1) / EP_THREADS;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  if (work_bytes < gpn_ep_sites_batched_work_bytes(n, batch)) return -18;
  if (!moments_only && !tau_out) return -19;
  if (!moments_only && !nu_out) return -20;
  if (!stats) return -24;
  hipStream_t s = static_cast<hipStream_t>(stream);
  EpArgs p;
  p.y = y, p.m = m, p.mu = mu, p.sigma2 = sigma2, p.tau = tau, p.nu = nu, p.nodes = nodes, p.weights = weights;
  p.tau_out = tau_out, p.nu_out = nu_out, p.lz = lz, p.mu_hat = mu_hat, p.s2_hat = s2_hat, p.partials = work;
  p.damping = 0.0, p.n = n, p.H = H, p.moments_only = moments_only;
  const dim3 grid((unsigned)blocks, (unsigned)batch);
  if (kind == GPN_LIK_PROBIT) hipLaunchKernelGGL(ep_sites_batched_kernel<GPN_LIK_PROBIT>, grid, dim3(EP_THREADS), 0, s, p, dampings, sy);
  else hipLaunchKernelGGL(ep_sites_batched_kernel<GPN_LIK_LOGIT>, grid, dim3(EP_THREADS), 0, s, p, dampings, sy);
  GPN_LAUNCH_CHECK();
  hipLaunchKernelGGL(ep_stats_batched_kernel, dim3(1, (unsigned)batch), dim3(EP_THREADS), 0, s, work, blocks, stats);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}
