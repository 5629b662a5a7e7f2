// LaplaceGP (gptorch_amd/models/laplace.py): the kernels of the Newton mode search and of the evidence gradient that are not
// the factorisation pipeline's own.  (The reference's Likelihood leaves the non-conjugate case as a TODO, likelihoods.py:47-78:
// nothing here restates reference code.)
//
//   lik_derivs_kernel     lp, d1 = dlp/df, W = -d2lp/df2, d3 = d3lp/df3 per point, sum lp per workgroup (then one workgroup adds
//                         the workgroups' sums): the point function of lik.hip, so both tails are stable.
//   lap_rows_kernel       one workgroup per lower 64 x 64 tile (kmat.hip's enumeration, staging and order of the sum over the
//                         coordinates: k_ij has the assembly's bits).  MODE 0: K v.  MODE 1: sum_j K_ij s_j Binv_ij, the row-dot
//                         form of diag((K^-1 + W)^-1) s.  Entry (i, j), j < i, is evaluated once and used twice: times vec_j it
//                         goes to row i, times vec_i (the mirror K_ji) to row j.  A tile leaves 64 row sums in slot [I][J] of the
//                         workspace and, off the diagonal, 64 mirror sums in slot [J][I]: every slot of the T x T grid is written
//                         exactly once.  lap_gather_kernel adds a row's T slots in ascending order.
//   lap_grad_kernel       the sweep of gpn_lml_grad (grad.hip, chunked form: any input dimension) with
//                         G_ij = 1/2 a_i a_j - 1/2 s_i s_j Binv_ij + 1/2 (u_i d1_j + d1_i u_j) formed in the tile epilogue from the
//                         four vectors (staged in LDS) and the lower triangle of Binv (read once, 16-byte loads).
// One kernel per operation: every kernel takes `batch` equal-shape models in one launch, the model index on blockIdx.y and model
// b's operands at a stride (lap_model; sf, sy).  The lock-step entry points (gpn_*_batched; models/_laplace_lockstep.py) launch
// gridDim.y = batch; a single entry point is its lock-step twin at batch = 1 with every stride 0, so a model's arithmetic and the
// order of its sums cannot depend on the entry point.
// HBM traffic: MODE 1 and the gradient sweep read Binv's lower triangle once (4 n^2 bytes); MODE 0 reads the points only and is
// bound by the fp64 exponentials.  Sums: a thread's own in a fixed order, then LDS in a fixed order, then the workspace in a
// fixed order -- no atomics, the same call twice gives the same bits.
#include "kernel_fn.h"
#include "lik_point.h"
#include "rowkernels.h"

namespace gpn {

typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int LT = 64;            // tile edge (kmat.hip KT)
constexpr int LDC = 16;           // coordinates staged per pass (kmat.hip DC)
constexpr int LD_THREADS = 256;   // points of a workgroup of lik_derivs_kernel, one per thread

// ---- pointwise derivatives -------------------------------------------------------------------------------------------------
// (the kernels' bodies are device functions of ONE model: the kernel moves the operands to model blockIdx.y, then runs the body)
template <int KIND>
__device__ __forceinline__ void lik_derivs_body(const double* __restrict__ f, const double* __restrict__ y, int64_t n,
                                                double* __restrict__ partials, double* __restrict__ d1,
                                                double* __restrict__ w, double* __restrict__ d3) {
  __shared__ double red[LD_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * LD_THREADS + tid;
  double lp = 0.0;
  if (i < n) {
    const double fi = f[i], yi = y[i];
    double g1, g2, g3;
    if (KIND == GPN_LIK_POISSON) {
      // log link: lp = y f - e^f - lgamma(y + 1)
      const double m = exp(fi);
      lp = yi * fi - m - lgamma(yi + 1.0);
      g1 = yi - m;
      g2 = m;
      g3 = -m;
    } else {
      const LikConst none = {0.0, 0.0, 0.0};
      double dlp, dpar;
      lik_point<KIND>(none, fi, 0.0, yi, lp, dlp, dpar);
      const double t = 2.0 * yi - 1.0;
      g1 = dlp;
      if (KIND == GPN_LIK_PROBIT) {
        const double z = t * fi, r = t * dlp;               // the hazard phi(z) / Phi(z) (t = +-1: exact)
        const double zr = z + r;
        g2 = r * zr;
        g3 = t * r * (zr * (zr + r) - 1.0);
      } else {
        // W = sigma(f) sigma(-f) = e / (1 + e)^2 and d3 = W tanh(f / 2) = W sign(f) (1 - e) / (1 + e), e = exp(-|f|):
        // independent of y; 1 - e through expm1 (no cancellation at small |f|)
        const double e = exp(-fabs(fi)), q = 1.0 + e;
        g2 = e / (q * q);
        g3 = g2 * (copysign(1.0, fi) * -expm1(-fabs(fi)) / q);
      }
    }
    if (d1) d1[i] = g1;
    if (w) w[i] = g2;
    if (d3) d3[i] = g3;
  }
  lp = wave_sum(lp);
  if (lane == 0) red[wave] = lp;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// model blockIdx.y: f + b sf, y + b sy (0: shared), its workgroups' sums at partials + b gridDim.x, outputs [batch, n]
template <int KIND>
__global__ __launch_bounds__(LD_THREADS) void lik_derivs_kernel(const double* __restrict__ f, int64_t sf, const double* __restrict__ y,
                                                                int64_t sy, int64_t n, double* __restrict__ partials,
                                                                double* __restrict__ d1, double* __restrict__ w,
                                                                double* __restrict__ d3) {
  const int64_t b = blockIdx.y;
  lik_derivs_body<KIND>(f + b * sf, y + b * sy, n, partials + b * gridDim.x, d1 ? d1 + b * n : nullptr, w ? w + b * n : nullptr,
                        d3 ? d3 + b * n : nullptr);
}

// (workgroup b adds model b's `count` sums into value[b])
__global__ __launch_bounds__(256) void lik_derivs_sum_kernel(const double* __restrict__ partials, int64_t count, double* __restrict__ value) {
  partials += (int64_t)blockIdx.x * count;
  value += blockIdx.x;
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) a += partials[i];
  a = wave_sum(a);
  if (lane == 0) red[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) value[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

static_assert(LD_THREADS == 256, "the workgroup's sums are combined as (w0 + w1) + (w2 + w3)");

// ---- what the tile kernels share ---------------------------------------------------------------------------------------------
struct LapArgs {
  const double* X;
  const double* variance;
  const double* ls;
  const double* s;        // sqrt(W): MODE 1, gradient sweep
  const double* Binv;     // lower triangle read: MODE 1, gradient sweep
  int64_t ldb;
  const double* v;        // MODE 0: the vector
  const double* a;        // gradient sweep: a, u, d1
  const double* u;
  const double* d1;
  double* work;
  int n, d, nls, tiles, nout;
};

// a lock-step launch: what separates model b's operands from model 0's, in doubles (X: 0 = shared points; the hyper-parameters
// are consecutive: variance[b], ls + b nls)
struct LapStrides {
  int64_t X, vec, Binv, work;      // vec: every [n] vector (s, v, a, u, d1)
};

// (what every tile kernel reads; a kernel moves its own vectors and Binv itself, so nothing asks which pointers are null and the
//  address arithmetic is straight-line.  Model 0 -- every workgroup of a single call -- skips it: its operands are where the
//  arguments point, and its instruction path is the one a kernel without strides would run)
__device__ __forceinline__ void lap_model(LapArgs& p, const LapStrides& st, int64_t b) {
  p.X += b * st.X;
  p.variance += b;
  p.ls += b * p.nls;
  p.work += b * st.work;
}

// tile q of the row-major enumeration of the lower triangle (kmat.hip)
__device__ __forceinline__ void lower_tile(int q, int& ti, int& tj) {
  ti = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > q) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
  tj = q - ti * (ti + 1) / 2;
}

struct LapStage {
  double xs[LDC][LT];     // row points, [coordinate][point], pre-multiplied by 1 / ell
  double ys[LDC][LT];     // column points
  double inv_ell[LDC];
};

// coordinates c0 .. c0 + 15 of both point blocks (the scaling and the layout of kmat.hip)
__device__ __forceinline__ void lap_stage(LapStage& S, const LapArgs& p, int i0, int j0, int c0) {
  const int tid = threadIdx.x;
  __syncthreads();                                   // the previous chunk is consumed
  if (tid < LDC) S.inv_ell[tid] = c0 + tid < p.d ? 1.0 / p.ls[p.nls == 1 ? 0 : c0 + tid] : 0.0;
  __syncthreads();
  for (int idx = tid; idx < LDC * LT; idx += 256) {
    const int dd = idx / LT, pt = idx - dd * LT;     // pt fastest: conflict-free LDS writes
    double vx = 0.0, vy = 0.0;
    if (c0 + dd < p.d) {
      const double ie = S.inv_ell[dd];
      if (i0 + pt < p.n) vx = p.X[(int64_t)(i0 + pt) * p.d + c0 + dd] * ie;
      if (j0 + pt < p.n) vy = p.X[(int64_t)(j0 + pt) * p.d + c0 + dd] * ie;
    }
    S.xs[dd][pt] = vx;
    S.ys[dd][pt] = vy;
  }
  __syncthreads();
}

// the 4 x 4 micro-tile of thread (tx, ty): rows ty * 4 + a, columns {2 tx, 2 tx + 1, 32 + 2 tx, 33 + 2 tx}
__device__ __forceinline__ void lap_fragments(const LapStage& S, int dd, int tx, int ty, double (&xr)[4], double (&yc)[4]) {
  const d2 xa = *reinterpret_cast<const d2*>(&S.xs[dd][ty * 4]);
  const d2 xb = *reinterpret_cast<const d2*>(&S.xs[dd][ty * 4 + 2]);
  const d2 ya = *reinterpret_cast<const d2*>(&S.ys[dd][tx * 2]);
  const d2 yb = *reinterpret_cast<const d2*>(&S.ys[dd][32 + tx * 2]);
  xr[0] = xa.x; xr[1] = xa.y; xr[2] = xb.x; xr[3] = xb.y;
  yc[0] = ya.x; yc[1] = ya.y; yc[2] = yb.x; yc[3] = yb.y;
}

// scaled squared distances of the micro-tile, the coordinates in ascending order (kmat.hip's sum, bit for bit)
__device__ __forceinline__ void lap_sqdist(LapStage& S, const LapArgs& p, int i0, int j0, int tx, int ty, double (&r2)[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
  for (int c0 = 0; c0 < p.d; c0 += LDC) {
    lap_stage(S, p, i0, j0, c0);
    const int lim = min(LDC, p.d - c0);
    for (int dd = 0; dd < lim; ++dd) {
      double xr[4], yc[4];
      lap_fragments(S, dd, tx, ty, xr, yc);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = xr[a] - yc[b];
          r2[a][b] = fma(df, df, r2[a][b]);
        }
    }
  }
}

// the lower triangle of Binv at the micro-tile: one 16-byte load per column pair where the layout allows it; zero above the
// diagonal and outside the matrix
__device__ __forceinline__ void lap_load_binv(const LapArgs& p, int i0, int j0, int tx, int ty, d2 (&gk)[4][2]) {
  const bool vec = ((p.ldb & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.Binv) & 15) == 0);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = i0 + ty * 4 + a;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int col = j0 + h * 32 + tx * 2;
      gk[a][h] = d2{0.0, 0.0};
      if (row < p.n && col <= row) {
        const double* src = p.Binv + (int64_t)row * p.ldb + col;
        if (vec && col + 1 <= row) gk[a][h] = *reinterpret_cast<const d2*>(src);
        else { gk[a][h].x = src[0]; if (col + 1 <= row) gk[a][h].y = src[1]; }
      }
    }
  }
}

// ---- K v and diag((K^-1 + W)^-1) s ----------------------------------------------------------------------------------------------
template <int KIND, int MODE>
__device__ __forceinline__ void lap_rows_body(const LapArgs& p) {
  __shared__ __attribute__((aligned(16))) LapStage S;
  __shared__ double vrow[LT], vcol[LT];
  __shared__ double rpart[16][LT + 1], cpart[16][LT + 1];
  __shared__ double fin[2][LT];
  int ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = ti * LT, j0 = tj * LT;

  d2 gk[4][2];
  if (MODE == 1) lap_load_binv(p, i0, j0, tx, ty, gk);      // requested here: the round trip runs under the distance pass
  const double* vec = MODE == 0 ? p.v : p.s;
  if (tid < 2 * LT) {
    const int pt = tid & (LT - 1), idx = (tid < LT ? i0 : j0) + pt;
    (tid < LT ? vrow : vcol)[pt] = idx < p.n ? vec[idx] : 0.0;
  }
  double r2[4][4];
  lap_sqdist(S, p, i0, j0, tx, ty, r2);                     // (its barriers also publish vrow / vcol)

  const double var = p.variance[0];
  double racc[4] = {0.0, 0.0, 0.0, 0.0}, cacc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int rl = ty * 4 + a, row = i0 + rl;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int cl = (b >> 1) * 32 + tx * 2 + (b & 1), col = j0 + cl;
      if (row < p.n && col <= row) {
        double t = kernel_of_r2<KIND>(r2[a][b], var);
        if (MODE == 1) t *= (b & 1) ? gk[a][b >> 1].y : gk[a][b >> 1].x;
        racc[a] = fma(t, vcol[cl], racc[a]);
        if (col < row) cacc[b] = fma(t, vrow[rl], cacc[b]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) rpart[tx][ty * 4 + a] = racc[a];
#pragma unroll
  for (int b = 0; b < 4; ++b) cpart[ty][(b >> 1) * 32 + tx * 2 + (b & 1)] = cacc[b];
  __syncthreads();
  if (tid < 2 * LT) {
    const int pt = tid & (LT - 1);
    double sum = 0.0;
    if (tid < LT) { for (int k = 0; k < 16; ++k) sum += rpart[k][pt]; }
    else { for (int k = 0; k < 16; ++k) sum += cpart[k][pt]; }
    fin[tid >> 6][pt] = sum;
  }
  __syncthreads();
  if (tid < LT) {
    double* slot = p.work + ((int64_t)ti * p.tiles + tj) * LT;
    if (ti == tj) {
      slot[tid] = fin[0][tid] + fin[1][tid];
    } else {
      slot[tid] = fin[0][tid];
      p.work[((int64_t)tj * p.tiles + ti) * LT + tid] = fin[1][tid];
    }
  }
}

template <int KIND, int MODE>
__global__ __launch_bounds__(256) void lap_rows_kernel(LapArgs p, LapStrides st) {
  const int64_t b = blockIdx.y;
  if (b != 0) {
    lap_model(p, st, b);
    if (MODE == 0) {
      p.v += b * st.vec;
    } else {
      p.s += b * st.vec;
      p.Binv += b * st.Binv;
    }
  }
  lap_rows_body<KIND, MODE>(p);
}

// out_i = sum_J slot[I][J][i - 64 I], J ascending (divide != nullptr: ... / divide_i); model blockIdx.y of a lock-step launch has
// its slots at work + b s_work, its divisors at divide + b s_div and its row of out at out + b n
__global__ __launch_bounds__(256) void lap_gather_kernel(const double* __restrict__ work, int tiles, int64_t n, const double* __restrict__ divide,
                                                         double* __restrict__ out, int64_t s_work, int64_t s_div) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  work += blockIdx.y * s_work;
  if (divide) divide += blockIdx.y * s_div;
  out += blockIdx.y * n;
  const double* src = work + (i / LT) * (int64_t)tiles * LT + (i % LT);
  double sum = 0.0;
  for (int j = 0; j < tiles; ++j) sum += src[(int64_t)j * LT];
  out[i] = divide ? sum / divide[i] : sum;
}

// ---- the evidence gradient ------------------------------------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ void lap_grad_body(const LapArgs& p) {
  __shared__ __attribute__((aligned(16))) LapStage S;
  __shared__ double rows4[4][LT], cols4[4][LT];             // a, u, d1, s at the tile's rows and columns
  __shared__ double red[256];
  int ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = ti * LT, j0 = tj * LT;

  d2 gk[4][2];
  lap_load_binv(p, i0, j0, tx, ty, gk);
  if (tid < 2 * LT) {
    const int pt = tid & (LT - 1), idx = (tid < LT ? i0 : j0) + pt;
    double (*dst)[LT] = tid < LT ? rows4 : cols4;
    const bool in = idx < p.n;
    dst[0][pt] = in ? p.a[idx] : 0.0;
    dst[1][pt] = in ? p.u[idx] : 0.0;
    dst[2][pt] = in ? p.d1[idx] : 0.0;
    dst[3][pt] = in ? p.s[idx] : 0.0;
  }
  double r2[4][4];
  lap_sqdist(S, p, i0, j0, tx, ty, r2);

  const double var = p.variance[0];
  double gb[4][4];
  double s_var = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int rl = ty * 4 + a, row = i0 + rl;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int cl = (b >> 1) * 32 + tx * 2 + (b & 1), col = j0 + cl;
      double g = 0.0;
      if (row < p.n && col <= row) {
        const double binv = (b & 1) ? gk[a][b >> 1].y : gk[a][b >> 1].x;
        const double cross = fma(rows4[1][rl], cols4[2][cl], rows4[2][rl] * cols4[1][cl]);     // u_i d1_j + d1_i u_j
        g = 0.5 * (fma(rows4[0][rl], cols4[0][cl], cross) - (rows4[3][rl] * cols4[3][cl]) * binv);
        if (col != row) g *= 2.0;                            // the symmetric partner (col, row)
      }
      double K, B;
      k_and_base<KIND>(r2[a][b], var, K, B);
      s_var = fma(g, K, s_var);
      gb[a][b] = g * B;
    }
  }

  auto block_sum = [&](double v) -> double {
    red[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) red[tid] += red[tid + w];
      __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
  };
  double* out = p.work + (int64_t)blockIdx.x * p.nout;
  const double tv = block_sum(s_var);
  if (tid == 0) out[0] = tv / var;                          // dK/dvar = K / var

  // per-dimension sums S_d = sum G'_ij ((x_id - x_jd) / ell_d)^2, chunk by chunk
  double s_iso = 0.0;
  for (int c0 = 0; c0 < p.d; c0 += LDC) {
    lap_stage(S, p, i0, j0, c0);
    const int lim = min(LDC, p.d - c0);
    for (int dd = 0; dd < lim; ++dd) {                      // uniform
      double xr[4], yc[4];
      lap_fragments(S, dd, tx, ty, xr, yc);
      double sacc = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = xr[a] - yc[b];
          sacc = fma(gb[a][b], df * df, sacc);
        }
      if (p.nls == 1) {
        s_iso += sacc;
      } else {
        const double t = block_sum(sacc);
        if (tid == 0) out[1 + c0 + dd] = t / p.ls[c0 + dd];
      }
    }
  }
  if (p.nls == 1) {
    const double t = block_sum(s_iso);
    if (tid == 0) out[1] = t / p.ls[0];
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void lap_grad_kernel(LapArgs p, LapStrides st) {
  const int64_t b = blockIdx.y;
  if (b != 0) {
    lap_model(p, st, b);
    p.s += b * st.vec;
    p.a += b * st.vec;
    p.u += b * st.vec;
    p.d1 += b * st.vec;
    p.Binv += b * st.Binv;
  }
  lap_grad_body<KIND>(p);
}

// out[k] = sum over the tiles' partials, in a fixed order (model blockIdx.y of a lock-step launch: its nblocks x nout partials and
// its row of out)
__global__ __launch_bounds__(256) void lap_grad_reduce_kernel(const double* __restrict__ partial, int64_t nblocks, int nout, double* __restrict__ out) {
  __shared__ double red[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  partial += (int64_t)blockIdx.y * nblocks * nout;
  out += (int64_t)blockIdx.y * nout;
  double s = 0.0;
  for (int64_t b = tid; b < nblocks; b += 256) s += partial[b * nout + k];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[k] = red[0];
}

static int64_t lap_tiles(int64_t n) { return (n + LT - 1) / LT; }

constexpr int LAP_MAX_BATCH = 65535;      // the model index is a grid's y (z) dimension

// what every tile entry point checks, in the order of its leading arguments: kind, X, n .. nls are arguments 2, 3, 4 .. 8 of a
// single entry point (which passes batch = 1, sX = 0) and, with batch and sX in between, 2, 4, 6 .. 10 of a lock-step one
static int lap_check(bool lockstep, int kind, int batch, const double* X, int64_t sX, int64_t n, int d, const double* variance,
                     const double* length_scales, int nls) {
  const int at_X = lockstep ? 4 : 3, at_n = lockstep ? 6 : 4;
  if (!kind_is_covariance(kind)) return -2;
  if (batch < 1) return -3;
  if (!X) return -at_X;
  if (sX < 0) return -5;
  if (n < 0 || n > 0x7fffffff) return -at_n;
  if (d <= 0) return -(at_n + 1);
  if (!variance) return -(at_n + 2);
  if (!length_scales) return -(at_n + 3);
  if (nls != 1 && nls != d) return -(at_n + 4);
  return GPN_OK;
}

// the operands every tile kernel takes (s, Binv, ldb: MODE 1 and the gradient sweep); the caller adds its own vectors
static LapArgs lap_args(const double* X, int64_t n, int d, const double* variance, const double* length_scales, int nls, const double* s,
                        const double* Binv, int64_t ldb, double* work) {
  LapArgs p = {};
  p.X = X; p.variance = variance; p.ls = length_scales; p.s = s; p.Binv = Binv; p.ldb = ldb; p.work = work;
  p.n = (int)n; p.d = d; p.nls = nls; p.tiles = (int)lap_tiles(n);
  return p;
}

// the pointwise derivatives of `batch` models and, value != nullptr, their sums (blocks: workgroups per model)
static int lik_derivs_launch(hipStream_t s, int kind, int batch, const double* f, int64_t sf, const double* y, int64_t sy, int64_t n,
                             int64_t blocks, double* work, double* value, double* d1, double* w, double* d3) {
  const dim3 grid((unsigned)blocks, (unsigned)batch), block(LD_THREADS);
  switch (kind) {
    case GPN_LIK_PROBIT: hipLaunchKernelGGL(lik_derivs_kernel<GPN_LIK_PROBIT>, grid, block, 0, s, f, sf, y, sy, n, work, d1, w, d3); break;
    case GPN_LIK_LOGIT: hipLaunchKernelGGL(lik_derivs_kernel<GPN_LIK_LOGIT>, grid, block, 0, s, f, sf, y, sy, n, work, d1, w, d3); break;
    default: hipLaunchKernelGGL(lik_derivs_kernel<GPN_LIK_POISSON>, grid, block, 0, s, f, sf, y, sy, n, work, d1, w, d3); break;
  }
  GPN_LAUNCH_CHECK();
  if (value) {
    hipLaunchKernelGGL(lik_derivs_sum_kernel, dim3((unsigned)batch), dim3(256), 0, s, work, blocks, value);
    GPN_LAUNCH_CHECK();
  }
  return GPN_OK;
}

// the tile sweep of `batch` models and the gather of their rows (n > 0)
template <int MODE>
static int lap_rows_launch(hipStream_t s, int kind, int batch, const LapArgs& p, const LapStrides& st, const double* divide, double* out) {
  const int64_t t = p.tiles;
  if (t * (t + 1) / 2 > 0x7fffffff || batch > LAP_MAX_BATCH) return GPN_E_UNSUPPORTED;
  const dim3 grid((unsigned)(t * (t + 1) / 2), (unsigned)batch);
  const int rc = with_kind(kind, [&](auto k) -> int {
    hipLaunchKernelGGL((lap_rows_kernel<decltype(k)::value, MODE>), grid, dim3(256), 0, s, p, st);
    GPN_LAUNCH_CHECK();
    return GPN_OK;
  });
  if (rc != GPN_OK) return rc;
  hipLaunchKernelGGL(lap_gather_kernel, dim3((unsigned)((p.n + 255) / 256), (unsigned)batch), dim3(256), 0, s, p.work, p.tiles, (int64_t)p.n,
                     divide, out, st.work, st.vec);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}

// the gradient sweep of `batch` models (p.a, p.u, p.d1 set; model b's partials st.work after model 0's) and its reduce into
// out [batch, 1 + nls] (kind: one that lap_check let through)
static int lap_grad_launch(hipStream_t s, int kind, int batch, LapArgs p, const LapStrides& st, double* out) {
  p.nout = 1 + p.nls;
  if (p.n == 0) {
    GPN_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)batch * p.nout * sizeof(double), s));
    return GPN_OK;
  }
  const int64_t t = p.tiles, nblocks = t * (t + 1) / 2;
  if (nblocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  const dim3 grid((unsigned)nblocks, (unsigned)batch);
  const double n = p.n;
  const int rc = with_kind(kind, [&](auto k) -> int {
    int rec = -1;
    if (profile_on()) rec = profile_begin(s, batch * 8.0 * (0.5 * n * (n + 1.0) + n * p.d), PROF_GRAD);
    hipLaunchKernelGGL(lap_grad_kernel<decltype(k)::value>, grid, dim3(256), 0, s, p, st);
    if (rec >= 0) profile_end(s, rec);
    GPN_LAUNCH_CHECK();
    return GPN_OK;
  });
  if (rc != GPN_OK) return rc;
  hipLaunchKernelGGL(lap_grad_reduce_kernel, dim3((unsigned)p.nout, (unsigned)batch), dim3(256), 0, s, p.work, nblocks, p.nout, out);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}

}  // namespace gpn

using namespace gpn;

extern "C" int64_t gpn_lik_derivs_work_bytes(int64_t n) {
  if (n <= 0) return 0;
  return (n + LD_THREADS - 1) / LD_THREADS * (int64_t)sizeof(double);
}

extern "C" int gpn_lik_derivs(void* stream, int kind, const double* f, const double* y, int64_t n, double* work, int64_t work_bytes,
                              double* value, double* d1, double* w, double* d3) {
  if (kind < GPN_LIK_PROBIT || kind > GPN_LIK_STUDENT_T) return -2;
  if (kind == GPN_LIK_STUDENT_T) return GPN_E_UNSUPPORTED;      // not log-concave: W may be negative, B indefinite
  if (!f) return -3;
  if (!y) return -4;
  if (n <= 0) return -5;
  if (!work) return -6;
  const int64_t blocks = (n + LD_THREADS - 1) / LD_THREADS;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  if (work_bytes < 8 * blocks) return -7;
  return lik_derivs_launch(static_cast<hipStream_t>(stream), kind, 1, f, 0, y, 0, n, blocks, work, value, d1, w, d3);
}

extern "C" int gpn_laplace_system(void* stream, int kind, const double* X, int64_t n, int d,
                                  const double* variance, const double* length_scales, int nls, const double* sc, double* A, int64_t lda) {
  const int rc = lap_check(false, kind, 1, X, 0, n, d, variance, length_scales, nls);
  if (rc != GPN_OK) return rc;
  if (!sc) return -9;
  if (!A) return -10;
  if (lda < n) return -11;
  if (n == 0) return GPN_OK;
  return assemble_laplace_system_batched(static_cast<hipStream_t>(stream), kind, 1, X, 0, n, d, variance, length_scales, nls, sc, 0, A, lda, 0);
}

extern "C" int64_t gpn_laplace_rows_work_bytes(int64_t n) {
  if (n <= 0) return 0;
  const int64_t t = lap_tiles(n);
  return t * t * LT * (int64_t)sizeof(double);
}

extern "C" int gpn_laplace_matvec(void* stream, int kind, const double* X, int64_t n, int d,
                                  const double* variance, const double* length_scales, int nls, const double* v, double* work, double* out) {
  const int rc = lap_check(false, kind, 1, X, 0, n, d, variance, length_scales, nls);
  if (rc != GPN_OK) return rc;
  if (!v) return -9;
  if (!work) return -10;
  if (!out) return -11;
  if (n == 0) return GPN_OK;
  LapArgs p = lap_args(X, n, d, variance, length_scales, nls, nullptr, nullptr, 0, work);
  p.v = v;
  return lap_rows_launch<0>(static_cast<hipStream_t>(stream), kind, 1, p, LapStrides{}, nullptr, out);
}

extern "C" int gpn_laplace_diag(void* stream, int kind, const double* X, int64_t n, int d,
                                const double* variance, const double* length_scales, int nls, const double* sc,
                                const double* Binv, int64_t ldb, double* work, double* sigma) {
  const int rc = lap_check(false, kind, 1, X, 0, n, d, variance, length_scales, nls);
  if (rc != GPN_OK) return rc;
  if (!sc) return -9;
  if (!Binv) return -10;
  if (ldb < n) return -11;
  if (!work) return -12;
  if (!sigma) return -13;
  if (n == 0) return GPN_OK;
  const LapArgs p = lap_args(X, n, d, variance, length_scales, nls, sc, Binv, ldb, work);
  return lap_rows_launch<1>(static_cast<hipStream_t>(stream), kind, 1, p, LapStrides{}, sc, sigma);
}

extern "C" int64_t gpn_laplace_grad_work_bytes(int64_t n, int nls) {
  if (n <= 0 || nls <= 0) return 0;
  const int64_t t = lap_tiles(n);
  return t * (t + 1) / 2 * (1 + nls) * (int64_t)sizeof(double);
}

extern "C" int gpn_laplace_grad(void* stream, int kind, const double* X, int64_t n, int d,
                                const double* variance, const double* length_scales, int nls, const double* sc,
                                const double* Binv, int64_t ldb, const double* a, const double* u, const double* d1,
                                double* work, double* out) {
  const int rc = lap_check(false, kind, 1, X, 0, n, d, variance, length_scales, nls);
  if (rc != GPN_OK) return rc;
  if (!sc) return -9;
  if (!Binv) return -10;
  if (ldb < n) return -11;
  if (!a) return -12;
  if (!u) return -13;
  if (!d1) return -14;
  if (!work) return -15;
  if (!out) return -16;
  LapArgs p = lap_args(X, n, d, variance, length_scales, nls, sc, Binv, ldb, work);
  p.a = a; p.u = u; p.d1 = d1;
  return lap_grad_launch(static_cast<hipStream_t>(stream), kind, 1, p, LapStrides{}, out);
}

// ---- the lock-step forms (models/_laplace_lockstep.py): the same launches with gridDim.y = batch and the operands' strides --------
extern "C" int64_t gpn_lik_derivs_batched_work_bytes(int64_t n, int batch) {
  if (batch <= 0) return 0;
  return batch * gpn_lik_derivs_work_bytes(n);
}

extern "C" int gpn_lik_derivs_batched(void* stream, int kind, int batch, const double* f, int64_t sf, const double* y, int64_t sy, int64_t n,
                                      double* work, int64_t work_bytes, double* value, double* d1, double* w, double* d3) {
  if (kind < GPN_LIK_PROBIT || kind > GPN_LIK_STUDENT_T) return -2;
  if (kind == GPN_LIK_STUDENT_T) return GPN_E_UNSUPPORTED;
  if (batch < 1) return -3;
  if (!f) return -4;
  if (sf < 0) return -5;
  if (!y) return -6;
  if (sy < 0) return -7;
  if (n <= 0) return -8;
  if (!work) return -9;
  const int64_t blocks = (n + LD_THREADS - 1) / LD_THREADS;
  if (blocks > 0x7fffffff || batch > LAP_MAX_BATCH) return GPN_E_UNSUPPORTED;
  if (work_bytes < 8 * blocks * batch) return -10;
  return lik_derivs_launch(static_cast<hipStream_t>(stream), kind, batch, f, sf, y, sy, n, blocks, work, value, d1, w, d3);
}

extern "C" int gpn_laplace_system_batched(void* stream, int kind, int batch, const double* X, int64_t sX, int64_t n, int d,
                                          const double* variance, const double* length_scales, int nls, const double* sc, int64_t ss,
                                          double* A, int64_t lda, int64_t sA) {
  const int rc = lap_check(true, kind, batch, X, sX, n, d, variance, length_scales, nls);
  if (rc != GPN_OK) return rc;
  if (!sc) return -11;
  if (ss < 0) return -12;
  if (!A) return -13;
  if (lda < n) return -14;
  if (batch > 1 && sA < (n - 1) * lda + n) return -15;
  if (batch > LAP_MAX_BATCH) return GPN_E_UNSUPPORTED;
  if (n == 0) return GPN_OK;
  return assemble_laplace_system_batched(static_cast<hipStream_t>(stream), kind, batch, X, sX, n, d, variance, length_scales, nls, sc, ss, A,
                                         lda, sA);
}

extern "C" int64_t gpn_laplace_rows_batched_work_bytes(int64_t n, int batch) {
  if (batch <= 0) return 0;
  return batch * gpn_laplace_rows_work_bytes(n);
}

extern "C" int gpn_laplace_matvec_batched(void* stream, int kind, int batch, const double* X, int64_t sX, int64_t n, int d,
                                          const double* variance, const double* length_scales, int nls, const double* v, int64_t sv,
                                          double* work, double* out) {
  const int rc = lap_check(true, kind, batch, X, sX, n, d, variance, length_scales, nls);
  if (rc != GPN_OK) return rc;
  if (!v) return -11;
  if (sv < 0) return -12;
  if (!work) return -13;
  if (!out) return -14;
  if (n == 0) return GPN_OK;
  LapArgs p = lap_args(X, n, d, variance, length_scales, nls, nullptr, nullptr, 0, work);
  p.v = v;
  const LapStrides st = {sX, sv, 0, gpn_laplace_rows_work_bytes(n) / (int64_t)sizeof(double)};
  return lap_rows_launch<0>(static_cast<hipStream_t>(stream), kind, batch, p, st, nullptr, out);
}

extern "C" int gpn_laplace_diag_batched(void* stream, int kind, int batch, const double* X, int64_t sX, int64_t n, int d,
                                        const double* variance, const double* length_scales, int nls, const double* sc, int64_t ss,
                                        const double* Binv, int64_t ldb, int64_t sB, double* work, double* sigma) {
  const int rc = lap_check(true, kind, batch, X, sX, n, d, variance, length_scales, nls);
  if (rc != GPN_OK) return rc;
  if (!sc) return -11;
  if (ss < 0) return -12;
  if (!Binv) return -13;
  if (ldb < n) return -14;
  if (sB < 0) return -15;
  if (!work) return -16;
  if (!sigma) return -17;
  if (n == 0) return GPN_OK;
  const LapArgs p = lap_args(X, n, d, variance, length_scales, nls, sc, Binv, ldb, work);
  const LapStrides st = {sX, ss, sB, gpn_laplace_rows_work_bytes(n) / (int64_t)sizeof(double)};
  return lap_rows_launch<1>(static_cast<hipStream_t>(stream), kind, batch, p, st, sc, sigma);
}

extern "C" int64_t gpn_laplace_grad_batched_work_bytes(int64_t n, int nls, int batch) {
  if (batch <= 0) return 0;
  return batch * gpn_laplace_grad_work_bytes(n, nls);
}

extern "C" int gpn_laplace_grad_batched(void* stream, int kind, int batch, const double* X, int64_t sX, int64_t n, int d,
                                        const double* variance, const double* length_scales, int nls, const double* sc,
                                        const double* Binv, int64_t ldb, int64_t sB, const double* a, const double* u, const double* d1,
                                        int64_t sv, double* work, double* out) {
  const int rc = lap_check(true, kind, batch, X, sX, n, d, variance, length_scales, nls);
  if (rc != GPN_OK) return rc;
  if (!sc) return -11;
  if (!Binv) return -12;
  if (ldb < n) return -13;
  if (sB < 0) return -14;
  if (!a) return -15;
  if (!u) return -16;
  if (!d1) return -17;
  if (sv < 0) return -18;
  if (!work) return -19;
  if (!out) return -20;
  if (batch > LAP_MAX_BATCH) return GPN_E_UNSUPPORTED;
  LapArgs p = lap_args(X, n, d, variance, length_scales, nls, sc, Binv, ldb, work);
  p.a = a; p.u = u; p.d1 = d1;
  const LapStrides st = {sX, sv, sB, gpn_laplace_grad_work_bytes(n, nls) / (int64_t)sizeof(double)};
  return lap_grad_launch(static_cast<hipStream_t>(stream), kind, batch, p, st, out);
}
