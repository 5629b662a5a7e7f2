// k-fold cross-validation of the exact GP in closed form (GPR(objective="kfold")): what the held-out folds need beyond the
// factorisation pipeline and loo.hip.  (The reference has no cross-validation objective: nothing here restates reference code.)
// With P = Kyy^-1 (lower triangle, from U U^T), a = P r, a fold with index set I of m_f points and P_f = P[I, I] = L_f L_f^T,
// U_f = L_f^-T, beta_f = L_f^-1 a_I:
//   y_I - mu_I = q_I = P_f^-1 a_I = U_f beta_f,  Sigma_f = P_f^-1 = U_f U_f^T,
//   L_kfold = sum_f (dy sum log L_f,ii - 1/2 ||beta_f||^2) - 1/2 n dy log 2 pi,
//   D = blockdiag_f 1/2 (dy Sigma_f + q_I q_I^T) = blockdiag_f W_f W_f^T,  W_f = [sqrt(dy/2) U_f | sqrt(1/2) q_I],
//   Q = P D P = S S^T,  S = P blockdiag(W_f),  G = -Q + 1/2 (a w^T + w a^T),  w = P q  (the sweep: loo.hip gpn_loo_grad).
// The k folds are padded to ONE shape m_max (identity on the padding diagonal: log 1 = 0, the padding decoupled, so the padded
// problems are exact) and go through gpn_potrf_lower_batched / gpn_lml_reduce_batched / gpn_trtri_upper_batched as equal-shape
// factor buffers; the products are gpn_gemm_nt_batched / gpn_gemm_nt.  New here, the fold on blockIdx.y, one launch each:
//   kfold_gather_kernel     P[I, I] (entry (i, j) read as P[max, min]), identity padding and a_I^T (the extra rows) into the k
//                           factor buffers: a pure copy.
//   kfold_columns_kernel    P[:, I_f] as full columns into [k, n_pad, m_pad], zero padded.  One workgroup per 64 x 64 tile: the
//                           entries on or below the diagonal are read along the row of P (thread index along the fold's columns),
//                           the mirrored ones along the row of P that holds them (thread index along the tile's ROWS: coalesced
//                           for every index list), both into LDS ([64][65]: the column walk is conflict-free), and the tile is
//                           stored once, rows of 64 consecutive doubles.
//   kfold_terms_kernel      one wavefront per held-out point: q_ic = sum_j U_f,ij beta_f,jc and the held-out variance
//                           sum_j U_f,ij^2 over j >= i in a fixed order, scattered to data order; sqrt(1/2) q into the last rows of W_f^T.
//   kfold_weights_kernel    W_f^T = sqrt(dy/2) U_f^T, 64 x 64 tiles transposed through LDS: the B operand of S_f = P[:, I_f] W_f.
//   kfold_value_kernel      one workgroup: the folds' sums in a fixed strided order; NaN when any fold's info != 0.
// No atomics, nothing synchronises, the same call twice gives the same bits.  An index outside [0, n) or a fold longer than m_max
// (the table is device memory: the host cannot see it) is never followed: such an entry reads nothing and writes nothing.
#include "kernel_fn.h"
#include "rowkernels.h"

namespace gpn {

constexpr int FT = 64;             // tile edge
constexpr int FROWS = 64;          // held-out points per workgroup of kfold_terms_kernel (16 per wavefront)

// fold f of the table: its first entry in idx and its length, clipped to m_max
__device__ __forceinline__ void kfold_range(const int32_t* __restrict__ off, int f, int m_max, int n, int& start, int& len) {
  const int a = off[f], b = off[f + 1];
  start = a;
  len = b - a;
  if (a < 0 || b > n || len < 0) len = 0;
  if (len > m_max) len = m_max;
}

// ---- P[I, I], the identity padding and a_I^T into the fold's factor buffer -----------------------------------------------------
// grid: (tiles over [m_max + dy rows] x [m_max columns], folds); thread index along the columns
__global__ __launch_bounds__(256) void kfold_gather_kernel(const double* __restrict__ Kinv, int64_t ldk, const double* __restrict__ at,
                                                           int64_t ldat, int n, int dy, const int32_t* __restrict__ off,
                                                           const int32_t* __restrict__ idx, int m_max, double* __restrict__ A, int64_t lda,
                                                           int64_t sA) {
  __shared__ int ri[FT], ci[FT];
  const int f = blockIdx.y;
  int start, len;
  kfold_range(off, f, m_max, n, start, len);
  const int tcols = (m_max + FT - 1) / FT;
  const int ti = blockIdx.x / tcols, tj = blockIdx.x - ti * tcols;
  const int i0 = ti * FT, j0 = tj * FT, tid = threadIdx.x;
  if (tid < 2 * FT) {
    const int loc = (tid < FT ? i0 : j0) + (tid & (FT - 1));
    int g = -1;
    if (loc < len) {
      g = idx[start + loc];
      if (g < 0 || g >= n) g = -1;
    }
    (tid < FT ? ri : ci)[tid & (FT - 1)] = g;
  }
  __syncthreads();
  A += (int64_t)f * sA;
  const int jj = tid & (FT - 1), j = j0 + jj;
  if (j >= m_max) return;
  const int gj = ci[jj];
  for (int ii = tid >> 6; ii < FT; ii += 4) {
    const int i = i0 + ii;
    if (i >= m_max + dy) break;
    double v;
    if (i < m_max) {
      const int gi = ri[ii];
      if (i < len && j < len) {
        if (gi < 0 || gj < 0) continue;                      // a bad table entry: not followed
        v = gi >= gj ? Kinv[(int64_t)gi * ldk + gj] : Kinv[(int64_t)gj * ldk + gi];
      } else {
        v = i == j ? 1.0 : 0.0;
      }
    } else {
      v = 0.0;
      if (j < len) {
        if (gj < 0) continue;
        v = at[(int64_t)(i - m_max) * ldat + gj];
      }
    }
    A[(int64_t)i * lda + j] = v;
  }
}

// ---- P[:, I_f] as full columns ---------------------------------------------------------------------------------------------------
// grid: (tiles over [n_pad rows] x [m_pad columns], folds); C_f = C + f sC, [n_pad, ldc]
__global__ __launch_bounds__(256) void kfold_columns_kernel(const double* __restrict__ Kinv, int64_t ldk, int n, const int32_t* __restrict__ off,
                                                            const int32_t* __restrict__ idx, int m_max, int n_pad, int m_pad,
                                                            double* __restrict__ C, int64_t ldc, int64_t sC) {
  __shared__ double T[FT][FT + 1];
  __shared__ int ci[FT];
  const int f = blockIdx.y;
  int start, len;
  kfold_range(off, f, m_max, n, start, len);
  const int tcols = (m_pad + FT - 1) / FT;
  const int ti = blockIdx.x / tcols, tj = blockIdx.x - ti * tcols;
  const int r0 = ti * FT, j0 = tj * FT, tid = threadIdx.x;
  if (tid < FT) {
    int g = -1;
    if (j0 + tid < len) {
      g = idx[start + j0 + tid];
      if (g < 0 || g >= n) g = -1;
    }
    ci[tid] = g;
  }
  __syncthreads();
  {
    // on or below the diagonal of P (and the zeros): thread index along the fold's columns
    const int jj = tid & (FT - 1), c = ci[jj];
    for (int rr = tid >> 6; rr < FT; rr += 4) {
      const int r = r0 + rr;
      if (c >= 0 && r < n) {
        if (r >= c) T[rr][jj] = Kinv[(int64_t)r * ldk + c];
      } else {
        T[rr][jj] = 0.0;
      }
    }
  }
  {
    // above it: the mirror P[c, r], thread index along the tile's rows (consecutive addresses of row c of P)
    const int rr = tid & (FT - 1), r = r0 + rr;
    for (int jj = tid >> 6; jj < FT; jj += 4) {
      const int c = ci[jj];
      if (c >= 0 && r < n && r < c) T[rr][jj] = Kinv[(int64_t)c * ldk + r];
    }
  }
  __syncthreads();
  C += (int64_t)f * sC;
  const int jj = tid & (FT - 1), j = j0 + jj;
  if (j >= m_pad) return;
  for (int rr = tid >> 6; rr < FT; rr += 4) {
    const int r = r0 + rr;
    if (r < n_pad) C[(int64_t)r * ldc + j] = T[rr][jj];
  }
}

// ---- q, the held-out variances, sqrt(1/2) q^T into W^T -----------------------------------------------------------------------------
// grid: (blocks of FROWS fold rows, folds).  U_f = U + f sU [.., ldu] (upper triangular), beta_f^T = the extra rows of the fold's
// factor buffer A + f sA (rows m_max .. m_max + dy - 1, lda).  Outputs in DATA order: qt [dy, n] (ldqt), var [n]; Wt_f = Wt + f sW
// ([.., ldw]): row m_max + c, column i <- sqrt(1/2) q_ic.
struct KFoldTermArgs {
  const double* U; int64_t ldu, sU;
  const double* A; int64_t lda, sA;
  const int32_t* off; const int32_t* idx;
  double* qt; int64_t ldqt;
  double* var;
  double* Wt; int64_t ldw, sW;
  int n, dy, m_max;
};

__global__ __launch_bounds__(256) void kfold_terms_kernel(KFoldTermArgs p) {
  const int f = blockIdx.y;
  int start, len;
  kfold_range(p.off, f, p.m_max, p.n, start, len);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* U = p.U + (int64_t)f * p.sU;
  const double* beta = p.A + (int64_t)f * p.sA + (int64_t)p.m_max * p.lda;
  double* Wt = p.Wt ? p.Wt + (int64_t)f * p.sW : nullptr;
  const int base = blockIdx.x * FROWS + wave * (FROWS / 4);
  for (int k = 0; k < FROWS / 4; ++k) {                      // uniform per wavefront
    const int i = base + k;
    if (i >= len) break;
    const int g = p.idx[start + i];
    if (g < 0 || g >= p.n) continue;
    const double* row = U + (int64_t)i * p.ldu;
    const int jb = i & ~63;
    if (p.var) {
      double s = 0.0;
      for (int j = jb + lane; j < len; j += 64) {
        const double u = j >= i ? row[j] : 0.0;
        s = fma(u, u, s);
      }
      s = wave_sum(s);
      if (lane == 0) p.var[g] = s;
    }
    for (int c = 0; c < p.dy; ++c) {
      const double* bc = beta + (int64_t)c * p.lda;
      double s = 0.0;
      for (int j = jb + lane; j < len; j += 64) {
        const double u = j >= i ? row[j] : 0.0;
        s = fma(u, bc[j], s);
      }
      s = wave_sum(s);
      if (lane == 0) {
        if (p.qt) p.qt[(int64_t)c * p.ldqt + g] = s;
        if (Wt) Wt[(int64_t)(p.m_max + c) * p.ldw + i] = 0.70710678118654752440 * s;
      }
    }
  }
}

// ---- W_f^T = scale U_f^T (rows and columns below the fold's length only) --------------------------------------------------------
// grid: (lower tiles (tj <= ti of W^T: U^T is lower triangular) over m_max, folds)
__global__ __launch_bounds__(256) void kfold_weights_kernel(const double* __restrict__ U, int64_t ldu, int64_t sU, const int32_t* __restrict__ off,
                                                            int n, int m_max, double scale, double* __restrict__ Wt, int64_t ldw, int64_t sW) {
  __shared__ double T[FT][FT + 1];
  const int f = blockIdx.y;
  int start, len;
  kfold_range(off, f, m_max, n, start, len);
  int ti = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > (int)blockIdx.x) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
  const int tj = blockIdx.x - ti * (ti + 1) / 2;
  // tile (ti, tj) of W^T = the transpose of tile (tj, ti) of U
  const int i0 = ti * FT, j0 = tj * FT, tid = threadIdx.x;
  if (i0 >= len) return;                                     // uniform
  U += (int64_t)f * sU;
  Wt += (int64_t)f * sW;
  const int cc = tid & (FT - 1);
  for (int rr = tid >> 6; rr < FT; rr += 4) {                // U[j0 + rr][i0 + cc], along the row of U
    const int ur = j0 + rr, uc = i0 + cc;
    T[rr][cc] = (ur < len && uc < len && uc >= ur) ? U[(int64_t)ur * ldu + uc] : 0.0;
  }
  __syncthreads();
  for (int rr = tid >> 6; rr < FT; rr += 4) {                // W^T[i0 + rr][j0 + cc] = scale U[j0 + cc][i0 + rr]
    const int wr = i0 + rr, wc = j0 + cc;
    if (wr < len && wc < len) Wt[(int64_t)wr * ldw + wc] = scale * T[cc][rr];
  }
}

// ---- the value ----------------------------------------------------------------------------------------------------------------------
// out3 [k, 3] of gpn_lml_reduce_batched over the folds' factor buffers: [3 f] = sum log L_f,ii, [3 f + 1] = ||beta_f||^2
__global__ __launch_bounds__(256) void kfold_value_kernel(const double* __restrict__ out3, const int32_t* __restrict__ info, int k, int dy,
                                                          double offset, double* __restrict__ value) {
  __shared__ double red[4];
  __shared__ int bad[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a = 0.0;
  int b = 0;
  for (int f = threadIdx.x; f < k; f += 256) {
    a += (double)dy * out3[3 * f] - 0.5 * out3[3 * f + 1];
    if (info && info[f] != 0) b = 1;
  }
  a = wave_sum(a);
  b = __any(b);
  if (lane == 0) { red[wave] = a; bad[wave] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double v = ((red[0] + red[1]) + (red[2] + red[3])) + offset;
    value[0] = (bad[0] | bad[1] | bad[2] | bad[3]) ? NAN : v;
  }
}

constexpr int KFOLD_MAX_FOLDS = 65535;    // the fold is a grid's y dimension

static int64_t kfold_tiles(int64_t x) { return (x + FT - 1) / FT; }

}  // namespace gpn

using namespace gpn;

extern "C" int gpn_kfold_gather(void* stream, int64_t n, int dy, const double* Kinv, int64_t ldk, const double* at, int64_t ldat,
                                int k, const int32_t* fold_off, const int32_t* fold_idx, int64_t m_max, double* A, int64_t lda,
                                int64_t sA) {
  if (n < 1 || n > 0x7fffffff) return -2;
  if (dy < 1) return -3;
  if (!Kinv) return -4;
  if (ldk < n) return -5;
  if (!at) return -6;
  if (ldat < n) return -7;
  if (k < 1) return -8;
  if (k > KFOLD_MAX_FOLDS) return GPN_E_UNSUPPORTED;
  if (!fold_off) return -9;
  if (!fold_idx) return -10;
  if (m_max < 1 || m_max > n) return -11;
  if (!A) return -12;
  if (lda < gpn_factor_ld(m_max, dy)) return -13;
  if (k > 1 && sA < gpn_factor_rows(m_max, dy) * lda) return -14;
  const int64_t blocks = kfold_tiles(m_max + dy) * kfold_tiles(m_max);
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kfold_gather_kernel, dim3((unsigned)blocks, (unsigned)k), dim3(256), 0, s, Kinv, ldk, at, ldat, (int)n, dy, fold_off, fold_idx,
                     (int)m_max, A, lda, sA);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}

extern "C" int gpn_kfold_columns(void* stream, int64_t n, const double* Kinv, int64_t ldk, int k, const int32_t* fold_off,
                                 const int32_t* fold_idx, int64_t m_max, double* C, int64_t ldc, int64_t sC) {
  if (n < 1 || n > 0x7fffffff) return -2;
  if (!Kinv) return -3;
  if (ldk < n) return -4;
  if (k < 1) return -5;
  if (k > KFOLD_MAX_FOLDS) return GPN_E_UNSUPPORTED;
  if (!fold_off) return -6;
  if (!fold_idx) return -7;
  if (m_max < 1 || m_max > n) return -8;
  if (!C) return -9;
  const int64_t n_pad = round_up(n, 16), m_pad = round_up(m_max, 16);
  if (ldc < m_pad) return -10;
  if (k > 1 && sC < n_pad * ldc) return -11;
  if ((ldc & 1) || (sC & 1) || (reinterpret_cast<uintptr_t>(C) & 15)) return GPN_E_ALIGN;
  const int64_t blocks = kfold_tiles(n_pad) * kfold_tiles(m_pad);
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kfold_columns_kernel, dim3((unsigned)blocks, (unsigned)k), dim3(256), 0, s, Kinv, ldk, (int)n, fold_off, fold_idx, (int)m_max,
                     (int)n_pad, (int)m_pad, C, ldc, sC);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}

extern "C" int gpn_kfold_terms(void* stream, int64_t n, int dy, int k, const int32_t* fold_off, const int32_t* fold_idx, int64_t m_max,
                               const double* U, int64_t ldu, int64_t sU, const double* A, int64_t lda, int64_t sA, const double* out3,
                               const int32_t* info, double* qt, int64_t ldqt, double* var, double* Wt, int64_t ldw, int64_t sW,
                               double* value) {
  if (n < 1 || n > 0x7fffffff) return -2;
  if (dy < 1) return -3;
  if (k < 1) return -4;
  if (k > KFOLD_MAX_FOLDS) return GPN_E_UNSUPPORTED;
  if (!fold_off) return -5;
  if (!fold_idx) return -6;
  if (m_max < 1 || m_max > n) return -7;
  if (!U) return -8;
  if (ldu < m_max) return -9;
  if (k > 1 && sU < m_max * ldu) return -10;
  if (!A) return -11;
  if (lda < gpn_factor_ld(m_max, dy)) return -12;
  if (k > 1 && sA < gpn_factor_rows(m_max, dy) * lda) return -13;
  if (value && !out3) return -14;
  if (qt && ldqt < n) return -17;
  if (Wt && ldw < round_up(m_max, 16)) return -20;
  if (Wt && k > 1 && sW < round_up(m_max + dy, 16) * ldw) return -21;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (qt || var || Wt) {
    KFoldTermArgs p = {U, ldu, sU, A, lda, sA, fold_off, fold_idx, qt, ldqt, var, Wt, ldw, sW, (int)n, dy, (int)m_max};
    hipLaunchKernelGGL(kfold_terms_kernel, dim3((unsigned)((m_max + FROWS - 1) / FROWS), (unsigned)k), dim3(256), 0, s, p);
    GPN_LAUNCH_CHECK();
  }
  if (Wt) {
    const int64_t t = kfold_tiles(m_max), blocks = t * (t + 1) / 2;
    if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
    hipLaunchKernelGGL(kfold_weights_kernel, dim3((unsigned)blocks, (unsigned)k), dim3(256), 0, s, U, ldu, sU, fold_off, (int)n, (int)m_max,
                       sqrt(0.5 * (double)dy), Wt, ldw, sW);
    GPN_LAUNCH_CHECK();
  }
  if (value) {
    const double offset = -0.5 * (double)n * (double)dy * 1.83787706640934548356;      // log(2 pi)
    hipLaunchKernelGGL(kfold_value_kernel, dim3(1), dim3(256), 0, s, out3, info, k, dy, offset, value);
    GPN_LAUNCH_CHECK();
  }
  return GPN_OK;
}

// bytes of the column buffer of gpn_kfold_columns ([k, round_up(n, 16), round_up(m_max, 16)]) and of W^T of gpn_kfold_terms
// ([k, round_up(m_max + dy, 16), round_up(m_max, 16)])
extern "C" int64_t gpn_kfold_columns_work_bytes(int64_t n, int k, int64_t m_max) {
  if (n < 1 || k < 1 || m_max < 1) return 0;
  return (int64_t)k * round_up(n, 16) * round_up(m_max, 16) * (int64_t)sizeof(double);
}

extern "C" int64_t gpn_kfold_weights_work_bytes(int k, int64_t m_max, int dy) {
  if (k < 1 || m_max < 1 || dy < 1) return 0;
  return (int64_t)k * round_up(m_max + dy, 16) * round_up(m_max, 16) * (int64_t)sizeof(double);
}
