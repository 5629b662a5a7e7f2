// Leave-one-out cross-validation of the exact GP (GPR(objective="loo"); Rasmussen & Williams 5.4.2, eqs. 5.10-5.13): what the
// closed form needs beyond the factorisation pipeline.  (The reference has no cross-validation objective: nothing here restates
// reference code.)  With P = Kyy^-1 (lower triangle, from U U^T), a = P r and p_i = P_ii:
//
//   loo_terms_kernel    one point per thread: q_ic = a_ic / p_i (the held-out residual y_i - mu_i), 1 / p_i (the held-out variance
//                       of the OBSERVATION), sqrt(d_i) with d_i = dy / (2 p_i) + sum_c a_ic^2 / (2 p_i^2), and the point's term
//                       1/2 dy log p_i - 1/2 sum_c a_ic q_ic of L_LOO, summed per workgroup; loo_sum_kernel (one workgroup) adds
//                       the workgroups' sums and the constant -1/2 n dy log 2 pi.  A p_i that is not a positive finite number
//                       makes every output of that point, and the value, NaN: nothing is clamped.
//   loo_scale_kernel    one workgroup per lower 64 x 64 tile of P: S_ij = P_ij sqrt(d_j), the FULL square.  The tile is read once
//                       (16-byte loads), kept in LDS ([64][65]: the column walk of the mirror is conflict-free), written as it
//                       stands (times the column's sqrt(d)) and, transposed, as its mirror (times the row's); a diagonal tile
//                       is completed in LDS and written once.  Nothing outside [n, n] is written.
//                       Q = P diag(d) P = S S^T is then ONE lower contraction (gpn_gemm_nt, unchanged).
//   loo_grad_kernel     the sweep of gpn_lml_grad / gpn_laplace_grad (chunked form: any input dimension) over the lower tiles with
//                       G_ij = -Q_ij + 1/2 sum_c (a_ic w_jc + w_ic a_jc), w = P q, formed in the tile epilogue: Q from its lower
//                       triangle (16-byte loads, once), a^T and w^T staged in LDS four right-hand sides at a time.
//                       Per tile: sum G dK/dvariance, sum G dK/dell_d, tr G; loo_grad_reduce_kernel adds the tiles' partials.
// HBM traffic: loo_scale reads 4 n^2 bytes and writes 8 n^2; loo_grad reads 4 n^2 and is otherwise bound by the fp64
// exponentials.  Sums: a thread's own in a fixed order, then the wavefront's shuffle tree / LDS in a fixed order, then the
// workspace in a fixed order -- no atomics, the same call twice gives the same bits.  Nothing synchronises.
// One kernel per operation: every kernel takes `batch` equal-shape models in one launch, the model index on blockIdx.y and model
// b's operands at pointer + b * stride (strides in doubles; sX = 0: shared points).  The lock-step entry points (gpn_loo_*_batched;
// _ops.BatchedGPRLooLik) launch gridDim.y = batch; a single entry point is its lock-step twin at batch = 1, so a model's
// arithmetic and the order of its sums cannot depend on the entry point.
#include "kernel_fn.h"
#include "rowkernels.h"

namespace gpn {

typedef double loo_d2 __attribute__((ext_vector_type(2)));

constexpr int OT = 64;             // tile edge (kmat.hip KT)
constexpr int ODC = 16;            // coordinates staged per pass (kmat.hip DC)
constexpr int ORHS = 4;            // right-hand sides of a^T / w^T staged per pass
constexpr int OT_THREADS = 256;    // points of a workgroup of loo_terms_kernel, one per thread

// ---- per-point terms -----------------------------------------------------------------------------------------------------------
// model blockIdx.y: Kinv + b sK, at + b sAt, qt + b sQt, its workgroups' sums at partials + b gridDim.x, var / rootd [batch, n]
struct LooTermStrides { int64_t sK, sAt, sQt; };

__global__ __launch_bounds__(OT_THREADS) void loo_terms_kernel(const double* __restrict__ Kinv, int64_t ldk, const double* __restrict__ at,
                                                               int64_t ldat, int64_t n, int dy, double* __restrict__ partials,
                                                               double* __restrict__ qt, int64_t ldqt, double* __restrict__ var,
                                                               double* __restrict__ rootd, LooTermStrides st) {
  __shared__ double red[OT_THREADS / 64];
  if (const int64_t b = blockIdx.y) {
    Kinv += b * st.sK;
    at += b * st.sAt;
    partials += b * gridDim.x;
    if (qt) qt += b * st.sQt;
    if (var) var += b * n;
    if (rootd) rootd += b * n;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * OT_THREADS + tid;
  double term = 0.0;
  if (i < n) {
    double p = Kinv[i * ldk + i];
    if (!(p > 0.0) || !(p < INFINITY)) p = NAN;              // not a precision: every output of the point says so
    const double v = 1.0 / p;
    double aq = 0.0, a2 = 0.0;
    for (int c = 0; c < dy; ++c) {
      const double a = at[(int64_t)c * ldat + i];
      const double q = a / p;
      if (qt) qt[(int64_t)c * ldqt + i] = q;
      aq = fma(a, q, aq);
      a2 = fma(a, a, a2);
    }
    term = 0.5 * ((double)dy * log(p) - aq);
    if (var) var[i] = v;
    if (rootd) rootd[i] = sqrt(0.5 * v * ((double)dy + a2 * v));
  }
  term = wave_sum(term);
  if (lane == 0) red[wave] = term;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

static_assert(OT_THREADS == 256, "the workgroup's sums are combined as (w0 + w1) + (w2 + w3)");

// value[0] = offset + the `count` workgroup sums, in a fixed strided order and the same tree (model blockIdx.y: its `count` sums
// and value[b])
__global__ __launch_bounds__(256) void loo_sum_kernel(const double* __restrict__ partials, int64_t count, double offset, double* __restrict__ value) {
  __shared__ double red[4];
  partials += (int64_t)blockIdx.y * count;
  value += blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) a += partials[i];
  a = wave_sum(a);
  if (lane == 0) red[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) value[0] = ((red[0] + red[1]) + (red[2] + red[3])) + offset;
}

// ---- what the tile kernels share -----------------------------------------------------------------------------------------------
// tile q of the row-major enumeration of the lower triangle (kmat.hip)
__device__ __forceinline__ void loo_lower_tile(int q, int& ti, int& tj) {
  ti = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > q) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
  tj = q - ti * (ti + 1) / 2;
}

// the lower triangle of a symmetric matrix at the 4 x 4 micro-tile of thread (tx, ty) -- rows ty * 4 + a, columns
// {2 tx, 2 tx + 1, 32 + 2 tx, 33 + 2 tx} --: one 16-byte load per column pair where the layout allows it; zero above the diagonal
// and outside the matrix
__device__ __forceinline__ void loo_load_lower(const double* __restrict__ M, int64_t ldm, int n, int i0, int j0, int tx, int ty,
                                               loo_d2 (&gk)[4][2]) {
  const bool vec = ((ldm & 1) == 0) && ((reinterpret_cast<uintptr_t>(M) & 15) == 0);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = i0 + ty * 4 + a;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int col = j0 + h * 32 + tx * 2;
      gk[a][h] = loo_d2{0.0, 0.0};
      if (row < n && col <= row) {
        const double* src = M + (int64_t)row * ldm + col;
        if (vec && col + 1 <= row) gk[a][h] = *reinterpret_cast<const loo_d2*>(src);
        else { gk[a][h].x = src[0]; if (col + 1 <= row) gk[a][h].y = src[1]; }
      }
    }
  }
}

// ---- S = P diag(sqrt d), both triangles ----------------------------------------------------------------------------------------
// (model blockIdx.y: Kinv + b sK, rootd + b n, S + b sS)
__global__ __launch_bounds__(256) void loo_scale_kernel(const double* __restrict__ Kinv, int64_t ldk, const double* __restrict__ rootd, int n,
                                                        double* __restrict__ S, int64_t lds, int64_t sK, int64_t sS) {
  __shared__ double T[OT][OT + 1];
  __shared__ double rrow[OT], rcol[OT];
  if (const int64_t b = blockIdx.y) {
    Kinv += b * sK;
    rootd += b * n;
    S += b * sS;
  }
  int ti, tj;
  loo_lower_tile(blockIdx.x, ti, tj);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = ti * OT, j0 = tj * OT;

  loo_d2 gk[4][2];
  loo_load_lower(Kinv, ldk, n, i0, j0, tx, ty, gk);
  if (tid < 2 * OT) {
    const int pt = tid & (OT - 1), idx = (tid < OT ? i0 : j0) + pt;
    (tid < OT ? rrow : rcol)[pt] = idx < n ? rootd[idx] : 0.0;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      T[ty * 4 + a][h * 32 + tx * 2] = gk[a][h].x;
      T[ty * 4 + a][h * 32 + tx * 2 + 1] = gk[a][h].y;
    }
  __syncthreads();
  if (ti == tj) {
    // the tile holds its own mirror: completed from LDS, written once
    for (int idx = tid; idx < OT * OT; idx += 256) {
      const int r = idx >> 6, c = idx & (OT - 1);
      if (i0 + r < n && j0 + c < n) S[(int64_t)(i0 + r) * lds + j0 + c] = (c <= r ? T[r][c] : T[c][r]) * rcol[c];
    }
    return;
  }
  for (int idx = tid; idx < OT * OT; idx += 256) {           // the tile as it stands: S_ij = P_ij sqrt(d_j)  (j0 + c < i0 <= n)
    const int r = idx >> 6, c = idx & (OT - 1);
    if (i0 + r < n) S[(int64_t)(i0 + r) * lds + j0 + c] = T[r][c] * rcol[c];
  }
  for (int idx = tid; idx < OT * OT; idx += 256) {           // its mirror: S_ji = P_ij sqrt(d_i), r fastest (coalesced stores)
    const int c = idx >> 6, r = idx & (OT - 1);
    if (i0 + r < n) S[(int64_t)(j0 + c) * lds + i0 + r] = T[r][c] * rrow[r];
  }
}

// ---- the gradient sweep ----------------------------------------------------------------------------------------------------------
struct LooGradArgs {
  const double* X;
  const double* variance;
  const double* ls;
  const double* Q;        // lower triangle read
  int64_t ldq;
  const double* at;       // a^T, w^T [dy, n]
  int64_t ldat;
  const double* wt;
  int64_t ldwt;
  double* work;
  int n, d, nls, dy, nout;
};

// model b of a lock-step launch: its operands b strides on (sX = 0: shared points), its own variance and length scales, its tiles'
// partials after those of the models before it
struct LooGradStrides { int64_t sX, sQ, sAt, sWt; };

__device__ __forceinline__ void loo_model(LooGradArgs& p, const LooGradStrides& st, int64_t b) {
  p.X += b * st.sX;
  p.variance += b;
  p.ls += b * p.nls;
  p.Q += b * st.sQ;
  p.at += b * st.sAt;
  p.wt += b * st.sWt;
  p.work += b * (int64_t)gridDim.x * p.nout;
}

struct LooStage {
  double xs[ODC][OT];     // row points, [coordinate][point], pre-multiplied by 1 / ell
  double ys[ODC][OT];     // column points
  double inv_ell[ODC];
};

// coordinates c0 .. c0 + 15 of both point blocks (the scaling and the layout of kmat.hip)
__device__ __forceinline__ void loo_stage(LooStage& S, const LooGradArgs& p, int i0, int j0, int c0) {
  const int tid = threadIdx.x;
  __syncthreads();                                   // the previous chunk is consumed
  if (tid < ODC) S.inv_ell[tid] = c0 + tid < p.d ? 1.0 / p.ls[p.nls == 1 ? 0 : c0 + tid] : 0.0;
  __syncthreads();
  for (int idx = tid; idx < ODC * OT; idx += 256) {
    const int dd = idx / OT, pt = idx - dd * OT;     // pt fastest: conflict-free LDS writes
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

__device__ __forceinline__ void loo_fragments(const LooStage& S, int dd, int tx, int ty, double (&xr)[4], double (&yc)[4]) {
  const loo_d2 xa = *reinterpret_cast<const loo_d2*>(&S.xs[dd][ty * 4]);
  const loo_d2 xb = *reinterpret_cast<const loo_d2*>(&S.xs[dd][ty * 4 + 2]);
  const loo_d2 ya = *reinterpret_cast<const loo_d2*>(&S.ys[dd][tx * 2]);
  const loo_d2 yb = *reinterpret_cast<const loo_d2*>(&S.ys[dd][32 + tx * 2]);
  xr[0] = xa.x; xr[1] = xa.y; xr[2] = xb.x; xr[3] = xb.y;
  yc[0] = ya.x; yc[1] = ya.y; yc[2] = yb.x; yc[3] = yb.y;
}

template <int KIND>
__global__ __launch_bounds__(256) void loo_grad_kernel(LooGradArgs p, LooGradStrides st) {
  if (const int64_t b = blockIdx.y) loo_model(p, st, b);
  __shared__ __attribute__((aligned(16))) LooStage S;
  __shared__ double arow[ORHS][OT], acol[ORHS][OT], wrow[ORHS][OT], wcol[ORHS][OT];
  __shared__ double red[256];
  int ti, tj;
  loo_lower_tile(blockIdx.x, ti, tj);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = ti * OT, j0 = tj * OT;

  loo_d2 gk[4][2];
  loo_load_lower(p.Q, p.ldq, p.n, i0, j0, tx, ty, gk);       // requested here: the round trip runs under the distance pass

  // scaled squared distances, the coordinates in ascending order (kmat.hip's sum)
  double r2[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
  for (int c0 = 0; c0 < p.d; c0 += ODC) {
    loo_stage(S, p, i0, j0, c0);
    const int lim = min(ODC, p.d - c0);
    for (int dd = 0; dd < lim; ++dd) {
      double xr[4], yc[4];
      loo_fragments(S, dd, tx, ty, xr, yc);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = xr[a] - yc[b];
          r2[a][b] = fma(df, df, r2[a][b]);
        }
    }
  }

  // the rank terms sum_c (a_ic w_jc + w_ic a_jc), four right-hand sides at a time, c ascending
  double cross[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) cross[a][b] = 0.0;
  for (int c0 = 0; c0 < p.dy; c0 += ORHS) {
    const int lim = min(ORHS, p.dy - c0);
    __syncthreads();                                         // the previous four are consumed
    for (int idx = tid; idx < 2 * ORHS * OT; idx += 256) {
      const int side = idx / (ORHS * OT), rem = idx - side * (ORHS * OT), cc = rem / OT, pt = rem - cc * OT;
      const int g = (side == 0 ? i0 : j0) + pt;
      const bool in = cc < lim && g < p.n;
      const double av = in ? p.at[(int64_t)(c0 + cc) * p.ldat + g] : 0.0;
      const double wv = in ? p.wt[(int64_t)(c0 + cc) * p.ldwt + g] : 0.0;
      (side == 0 ? arow : acol)[cc][pt] = av;
      (side == 0 ? wrow : wcol)[cc][pt] = wv;
    }
    __syncthreads();
    for (int cc = 0; cc < lim; ++cc) {                       // uniform
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int rl = ty * 4 + a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int cl = (b >> 1) * 32 + tx * 2 + (b & 1);
          cross[a][b] = fma(arow[cc][rl], wcol[cc][cl], fma(wrow[cc][rl], acol[cc][cl], cross[a][b]));
        }
      }
    }
  }

  const double var = p.variance[0];
  double gb[4][4];
  double s_var = 0.0, s_tr = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = i0 + ty * 4 + a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = j0 + (b >> 1) * 32 + tx * 2 + (b & 1);
      double g = 0.0;
      if (row < p.n && col <= row) {
        const double q = (b & 1) ? gk[a][b >> 1].y : gk[a][b >> 1].x;
        g = 0.5 * cross[a][b] - q;
        if (col == row) s_tr += g;
        else g *= 2.0;                                       // the symmetric partner (col, row)
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
  for (int c0 = 0; c0 < p.d; c0 += ODC) {
    loo_stage(S, p, i0, j0, c0);
    const int lim = min(ODC, p.d - c0);
    for (int dd = 0; dd < lim; ++dd) {                      // uniform
      double xr[4], yc[4];
      loo_fragments(S, dd, tx, ty, xr, yc);
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
  const double tt = block_sum(s_tr);
  if (tid == 0) out[1 + p.nls] = tt;
}

// out[k] = sum over the tiles' partials, in a fixed order (model blockIdx.y of a lock-step launch: its nblocks x nout partials and
// its row of out)
__global__ __launch_bounds__(256) void loo_grad_reduce_kernel(const double* __restrict__ partial, int64_t nblocks, int nout, double* __restrict__ out) {
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

static int64_t loo_tiles(int64_t n) { return (n + OT - 1) / OT; }

constexpr int LOO_MAX_BATCH = 65535;      // the model index is a grid's y dimension: larger batches go out in several launches

// the extent of a [rows, n] row-major block with leading dimension ld, in doubles: the least stride between two models' blocks
static int64_t loo_extent(int64_t rows, int64_t n, int64_t ld) { return rows <= 0 || n <= 0 ? 0 : (rows - 1) * ld + n; }

// ---- the launches: `batch` models per call (validated by the entry points; n > 0) ------------------------------------------------
static int loo_terms_launch(hipStream_t s, int batch, int64_t n, int dy, const double* Kinv, int64_t ldk, int64_t sK, const double* at,
                            int64_t ldat, int64_t sAt, double* work, double* qt, int64_t ldqt, int64_t sQt, double* var, double* rootd,
                            double* value) {
  const int64_t blocks = (n + OT_THREADS - 1) / OT_THREADS;
  const double offset = -0.5 * (double)n * (double)dy * 1.83787706640934548356;      // log(2 pi)
  const LooTermStrides st = {sK, sAt, sQt};
  for (int64_t z0 = 0; z0 < batch; z0 += LOO_MAX_BATCH) {
    const unsigned nb = (unsigned)std::min<int64_t>(LOO_MAX_BATCH, batch - z0);
    double* wz = work + z0 * blocks;
    hipLaunchKernelGGL(loo_terms_kernel, dim3((unsigned)blocks, nb), dim3(OT_THREADS), 0, s, Kinv + z0 * sK, ldk, at + z0 * sAt, ldat, n, dy, wz,
                       qt ? qt + z0 * sQt : nullptr, ldqt, var ? var + z0 * n : nullptr, rootd ? rootd + z0 * n : nullptr, st);
    GPN_LAUNCH_CHECK();
    if (value) {
      hipLaunchKernelGGL(loo_sum_kernel, dim3(1, nb), dim3(256), 0, s, wz, blocks, offset, value + z0);
      GPN_LAUNCH_CHECK();
    }
  }
  return GPN_OK;
}

static int loo_scale_launch(hipStream_t s, int batch, int64_t n, const double* Kinv, int64_t ldk, int64_t sK, const double* rootd, double* S,
                            int64_t lds, int64_t sS) {
  const int64_t t = loo_tiles(n), nblocks = t * (t + 1) / 2;
  if (nblocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  for (int64_t z0 = 0; z0 < batch; z0 += LOO_MAX_BATCH) {
    const unsigned nb = (unsigned)std::min<int64_t>(LOO_MAX_BATCH, batch - z0);
    hipLaunchKernelGGL(loo_scale_kernel, dim3((unsigned)nblocks, nb), dim3(256), 0, s, Kinv + z0 * sK, ldk, rootd + z0 * n, (int)n, S + z0 * sS, lds,
                       sK, sS);
    GPN_LAUNCH_CHECK();
  }
  return GPN_OK;
}

// p: model 0's operands; work holds batch x tiles x nout partials, out [batch, nout]
static int loo_grad_launch(hipStream_t s, int kind, int batch, LooGradArgs p, const LooGradStrides& st, double* out) {
  const int64_t n = p.n, t = loo_tiles(n), nblocks = t * (t + 1) / 2;
  if (nblocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  const double nn = (double)n;
  for (int64_t z0 = 0; z0 < batch; z0 += LOO_MAX_BATCH) {
    const unsigned nb = (unsigned)std::min<int64_t>(LOO_MAX_BATCH, batch - z0);
    LooGradArgs q = p;
    q.X += z0 * st.sX; q.variance += z0; q.ls += z0 * p.nls; q.Q += z0 * st.sQ; q.at += z0 * st.sAt; q.wt += z0 * st.sWt;
    q.work += z0 * nblocks * p.nout;
    const dim3 grid((unsigned)nblocks, nb);
    const int rc = with_kind<true>(kind, [&](auto k) -> int {
      int rec = -1;
      if (profile_on()) rec = profile_begin(s, 8.0 * (double)nb * (0.5 * nn * (nn + 1.0) + nn * p.d), PROF_GRAD);
      hipLaunchKernelGGL(loo_grad_kernel<decltype(k)::value>, grid, dim3(256), 0, s, q, st);
      if (rec >= 0) profile_end(s, rec);
      GPN_LAUNCH_CHECK();
      return GPN_OK;
    });
    if (rc != GPN_OK) return rc;
    hipLaunchKernelGGL(loo_grad_reduce_kernel, dim3((unsigned)p.nout, nb), dim3(256), 0, s, q.work, nblocks, p.nout, out + z0 * p.nout);
    GPN_LAUNCH_CHECK();
  }
  return GPN_OK;
}

}  // namespace gpn

using namespace gpn;

extern "C" int64_t gpn_loo_terms_work_bytes(int64_t n) {
  if (n <= 0) return 0;
  return (n + OT_THREADS - 1) / OT_THREADS * (int64_t)sizeof(double);
}

extern "C" int gpn_loo_terms(void* stream, int64_t n, int dy, const double* Kinv, int64_t ldk, const double* at, int64_t ldat,
                             double* work, int64_t work_bytes, double* qt, int64_t ldqt, double* var, double* rootd, double* value) {
  if (n < 0) return -2;
  if (dy < 1) return -3;
  if (!Kinv) return -4;
  if (ldk < n) return -5;
  if (!at) return -6;
  if (ldat < n) return -7;
  if (n > 0 && !work) return -8;
  const int64_t blocks = (n + OT_THREADS - 1) / OT_THREADS;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  if (work_bytes < 8 * blocks) return -9;
  if (qt && ldqt < n) return -11;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (value) GPN_HIP_CHECK(hipMemsetAsync(value, 0, sizeof(double), s));
    return GPN_OK;
  }
  return loo_terms_launch(s, 1, n, dy, Kinv, ldk, 0, at, ldat, 0, work, qt, ldqt, 0, var, rootd, value);
}

extern "C" int64_t gpn_loo_terms_batched_work_bytes(int64_t n, int batch) {
  if (batch < 1) return 0;
  return (int64_t)batch * gpn_loo_terms_work_bytes(n);
}

extern "C" int gpn_loo_terms_batched(void* stream, int batch, int64_t n, int dy, const double* Kinv, int64_t ldk, int64_t sK,
                                     const double* at, int64_t ldat, int64_t sAt, double* work, int64_t work_bytes, double* qt,
                                     int64_t ldqt, int64_t sQt, double* var, double* rootd, double* value) {
  if (batch < 1) return -2;
  if (n < 0) return -3;
  if (dy < 1) return -4;
  if (!Kinv) return -5;
  if (ldk < n) return -6;
  if (batch > 1 && sK < loo_extent(n, n, ldk)) return -7;
  if (!at) return -8;
  if (ldat < n) return -9;
  if (batch > 1 && sAt < loo_extent(dy, n, ldat)) return -10;
  if (n > 0 && !work) return -11;
  const int64_t blocks = (n + OT_THREADS - 1) / OT_THREADS;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  if (work_bytes < gpn_loo_terms_batched_work_bytes(n, batch)) return -12;
  if (qt && ldqt < n) return -14;
  if (qt && batch > 1 && sQt < loo_extent(dy, n, ldqt)) return -15;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (value) GPN_HIP_CHECK(hipMemsetAsync(value, 0, (size_t)batch * sizeof(double), s));
    return GPN_OK;
  }
  return loo_terms_launch(s, batch, n, dy, Kinv, ldk, sK, at, ldat, sAt, work, qt, ldqt, sQt, var, rootd, value);
}

extern "C" int gpn_loo_scale(void* stream, int64_t n, const double* Kinv, int64_t ldk, const double* rootd, double* S, int64_t lds) {
  if (n < 0 || n > 0x7fffffff) return -2;
  if (!Kinv) return -3;
  if (ldk < n) return -4;
  if (!rootd) return -5;
  if (!S) return -6;
  if (lds < n) return -7;
  if (n == 0) return GPN_OK;
  return loo_scale_launch(static_cast<hipStream_t>(stream), 1, n, Kinv, ldk, 0, rootd, S, lds, 0);
}

extern "C" int gpn_loo_scale_batched(void* stream, int batch, int64_t n, const double* Kinv, int64_t ldk, int64_t sK, const double* rootd,
                                     double* S, int64_t lds, int64_t sS) {
  if (batch < 1) return -2;
  if (n < 0 || n > 0x7fffffff) return -3;
  if (!Kinv) return -4;
  if (ldk < n) return -5;
  if (batch > 1 && sK < loo_extent(n, n, ldk)) return -6;
  if (!rootd) return -7;
  if (!S) return -8;
  if (lds < n) return -9;
  if (batch > 1 && sS < loo_extent(n, n, lds)) return -10;
  if (n == 0) return GPN_OK;
  return loo_scale_launch(static_cast<hipStream_t>(stream), batch, n, Kinv, ldk, sK, rootd, S, lds, sS);
}

extern "C" int64_t gpn_loo_grad_work_bytes(int64_t n, int nls) {
  if (n <= 0 || nls <= 0) return 0;
  const int64_t t = loo_tiles(n);
  return t * (t + 1) / 2 * (2 + nls) * (int64_t)sizeof(double);
}

extern "C" int gpn_loo_grad(void* stream, int kind, const double* X, int64_t n, int d, const double* variance, const double* length_scales,
                            int nls, const double* Q, int64_t ldq, const double* at, int64_t ldat, const double* wt, int64_t ldwt, int dy,
                            double* work, int64_t work_bytes, double* out) {
  if (kind < GPN_RBF || kind > GPN_PERIODIC) return -2;
  if (!X) return -3;
  if (n < 0 || n > 0x7fffffff) return -4;
  if (d <= 0) return -5;
  if (!variance) return -6;
  if (!length_scales) return -7;
  if (nls != 1 && nls != d) return -8;
  if (!Q) return -9;
  if (ldq < n) return -10;
  if (!at) return -11;
  if (ldat < n) return -12;
  if (!wt) return -13;
  if (ldwt < n) return -14;
  if (dy < 1) return -15;
  if (n > 0 && !work) return -16;
  if (work_bytes < gpn_loo_grad_work_bytes(n, nls)) return -17;
  if (!out) return -18;
  hipStream_t s = static_cast<hipStream_t>(stream);
  LooGradArgs p = {};
  p.X = X; p.variance = variance; p.ls = length_scales; p.Q = Q; p.ldq = ldq; p.at = at; p.ldat = ldat; p.wt = wt; p.ldwt = ldwt;
  p.work = work; p.n = (int)n; p.d = d; p.nls = nls; p.dy = dy; p.nout = 2 + nls;
  if (n == 0) {
    GPN_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)p.nout * sizeof(double), s));
    return GPN_OK;
  }
  return loo_grad_launch(s, kind, 1, p, LooGradStrides{0, 0, 0, 0}, out);
}

extern "C" int64_t gpn_loo_grad_batched_work_bytes(int64_t n, int nls, int batch) {
  if (batch < 1) return 0;
  return (int64_t)batch * gpn_loo_grad_work_bytes(n, nls);
}

extern "C" int gpn_loo_grad_batched(void* stream, int kind, int batch, const double* X, int64_t sX, int64_t n, int d, const double* variance,
                                    const double* length_scales, int nls, const double* Q, int64_t ldq, int64_t sQ, const double* at,
                                    int64_t ldat, int64_t sAt, const double* wt, int64_t ldwt, int64_t sWt, int dy, double* work,
                                    int64_t work_bytes, double* out) {
  if (kind < GPN_RBF || kind > GPN_PERIODIC) return -2;
  if (batch < 1) return -3;
  if (!X) return -4;
  if (n < 0 || n > 0x7fffffff) return -6;
  if (d <= 0) return -7;
  if (sX != 0 && sX < n * d) return -5;
  if (!variance) return -8;
  if (!length_scales) return -9;
  if (nls != 1 && nls != d) return -10;
  if (!Q) return -11;
  if (ldq < n) return -12;
  if (batch > 1 && sQ < loo_extent(n, n, ldq)) return -13;
  if (!at) return -14;
  if (ldat < n) return -15;
  if (dy < 1) return -20;
  if (batch > 1 && sAt < loo_extent(dy, n, ldat)) return -16;
  if (!wt) return -17;
  if (ldwt < n) return -18;
  if (batch > 1 && sWt < loo_extent(dy, n, ldwt)) return -19;
  if (n > 0 && !work) return -21;
  if (work_bytes < gpn_loo_grad_batched_work_bytes(n, nls, batch)) return -22;
  if (!out) return -23;
  hipStream_t s = static_cast<hipStream_t>(stream);
  LooGradArgs p = {};
  p.X = X; p.variance = variance; p.ls = length_scales; p.Q = Q; p.ldq = ldq; p.at = at; p.ldat = ldat; p.wt = wt; p.ldwt = ldwt;
  p.work = work; p.n = (int)n; p.d = d; p.nls = nls; p.dy = dy; p.nout = 2 + nls;
  if (n == 0) {
    GPN_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)batch * p.nout * sizeof(double), s));
    return GPN_OK;
  }
  return loo_grad_launch(s, kind, batch, p, LooGradStrides{sX, sQ, sAt, sWt}, out);
}
