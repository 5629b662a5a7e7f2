// The row kernels of the SVGP bound (gptorch/models/sparse_gpr.py:263-308, 337-381) around the contractions: with
// alpha = K(x_b, Z) L^-T [rows, m], T = alpha Q [rows, m] (Q = beta beta^T - I) and w = L^-1 m_u [m, dy],
//   marginals:      f_var_i = kdiag_i + sum_j alpha_ij T_ij,   f_mean0_i = alpha_i w           (sparse_gpr.py:367-377)
//   backward rows:  T <- G_alpha = 2 g_var_i T_i + g_mean_i w^T  (in place), and the transposed operands alpha^T and
//                   (diag(g_var) alpha)^T [m, rows] of the weighted SYRK alpha^T diag(g_var) alpha and of alpha^T g_mean.
// Both are one pass over HBM.  Every sum has a fixed order (lane-strided partial sums, then a shuffle tree): the same
// inputs give the same bits, whatever the scheduling; nothing is accumulated with atomics.
#include "gpn_common.h"

namespace gpn {

constexpr int SV_WAVES = 4;       // wavefronts per workgroup (marginals)
constexpr int SV_RW = 4;          // rows per wavefront
constexpr int SV_JT = 1024;       // columns of w staged in LDS at a time
constexpr int SV_DYB = 4;         // output columns per pass over a row

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;                        // lane 0 holds the sum
}

// One wavefront per SV_RW rows; lane l owns the column pairs 2l, 2l + 128, ... (16-byte loads).  w is staged in LDS in tiles
// of SV_JT columns x SV_DYB outputs; output columns beyond SV_DYB take further passes over the (cache-resident) rows.
__global__ __launch_bounds__(SV_WAVES * 64) void svgp_marginals_kernel(const double* __restrict__ alpha, int64_t lda,
                                                                       const double* __restrict__ T, int64_t ldt, int64_t rows,
                                                                       int64_t m, const double* __restrict__ w, int64_t ldw, int dy,
                                                                       const double* __restrict__ kdiag, int64_t kds,
                                                                       double* __restrict__ f_mean, double* __restrict__ f_var) {
  __shared__ double ws[SV_JT * SV_DYB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = ((int64_t)blockIdx.x * SV_WAVES + wave) * SV_RW;
  for (int c0 = 0; c0 < dy; c0 += SV_DYB) {
    const int nc = dy - c0 < SV_DYB ? dy - c0 : SV_DYB;
    double q[SV_RW], mu[SV_RW][SV_DYB];
#pragma unroll
    for (int r = 0; r < SV_RW; ++r) {
      q[r] = 0.0;
#pragma unroll
      for (int c = 0; c < SV_DYB; ++c) mu[r][c] = 0.0;
    }
    for (int64_t j0 = 0; j0 < m; j0 += SV_JT) {
      const int jt = (int)(m - j0 < SV_JT ? m - j0 : SV_JT);
      __syncthreads();
      for (int k = threadIdx.x; k < SV_JT * SV_DYB; k += SV_WAVES * 64) {
        const int j = k / SV_DYB, c = k - j * SV_DYB;
        ws[k] = (j < jt && c < nc) ? w[(j0 + j) * ldw + c0 + c] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < SV_RW; ++r) {
        const int64_t row = r0 + r;
        if (row >= rows) continue;                       // wave-uniform
        const double* ar = alpha + row * lda + j0;
        const double* tr = T + row * ldt + j0;
        for (int j = 2 * lane; j < jt; j += 128) {
          double2 a = *reinterpret_cast<const double2*>(ar + j);
          if (j + 1 >= jt) a.y = 0.0;                    // odd tail: the neighbour is padding
          if (c0 == 0) {
            double2 t = *reinterpret_cast<const double2*>(tr + j);
            if (j + 1 >= jt) t.y = 0.0;
            q[r] = fma(a.x, t.x, q[r]);
            q[r] = fma(a.y, t.y, q[r]);
          }
#pragma unroll
          for (int c = 0; c < SV_DYB; ++c) {
            mu[r][c] = fma(a.x, ws[j * SV_DYB + c], mu[r][c]);
            mu[r][c] = fma(a.y, ws[(j + 1) * SV_DYB + c], mu[r][c]);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < SV_RW; ++r) {
      const int64_t row = r0 + r;
      if (row >= rows) continue;
      if (c0 == 0) {
        const double s = wave_sum(q[r]);
        if (lane == 0) f_var[row] = kdiag[row * kds] + s;
      }
#pragma unroll
      for (int c = 0; c < SV_DYB; ++c) {
        const double s = wave_sum(mu[r][c]);
        if (lane == 0 && c < nc) f_mean[row * dy + c0 + c] = s;
      }
    }
  }
}

constexpr int SV_TR = 32;         // rows of a transposed tile
constexpr int SV_TC = 64;         // columns of a transposed tile
constexpr int SV_GB = 8;          // output columns of g_mean / w staged at a time

// Tile (32 rows x 64 columns) per workgroup of 256 threads.  Read side: thread (tx, ty) reads the column pair 2 tx of the
// rows ty, ty + 8, ... (16-byte loads, coalesced along the row); write side: the tile goes out transposed from LDS, row
// pairs as 16-byte stores (coalesced along the rows of alpha^T).  Rows rows .. round_up(rows, 16) - 1 (the K padding of the
// contractions that read the transposed operands) are written as exact zeros.
__global__ __launch_bounds__(256) void svgp_backward_rows_kernel(const double* __restrict__ alpha, int64_t lda, double* __restrict__ T,
                                                                 int64_t ldt, int64_t rows, int64_t m, const double* __restrict__ w,
                                                                 int64_t ldw, int dy, const double* __restrict__ g_var,
                                                                 const double* __restrict__ g_mean, double* __restrict__ alphaT,
                                                                 double* __restrict__ galphaT, int64_t ldo) {
  __shared__ double ta[SV_TR][SV_TC + 1];
  __shared__ double gv[SV_TR];
  __shared__ double gm[SV_TR][SV_GB];
  __shared__ double wt[SV_TC][SV_GB];
  const int64_t r0 = (int64_t)blockIdx.y * SV_TR, c0 = (int64_t)blockIdx.x * SV_TC;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  if (tid < SV_TR) gv[tid] = (r0 + tid < rows) ? g_var[r0 + tid] : 0.0;
  const int64_t cc = c0 + 2 * tx;
  double2 acc[SV_TR / 8];
#pragma unroll
  for (int k = 0; k < SV_TR / 8; ++k) acc[k] = make_double2(0.0, 0.0);
  for (int k0 = 0; k0 < dy; k0 += SV_GB) {                 // sum_k g_mean[r, k] w[c, k]
    __syncthreads();
    {
      const int r = tid / SV_GB, k = tid - r * SV_GB;     // 32 x 8
      gm[r][k] = (r0 + r < rows && k0 + k < dy) ? g_mean[(r0 + r) * dy + k0 + k] : 0.0;
    }
    for (int e = tid; e < SV_TC * SV_GB; e += 256) {
      const int c = e / SV_GB, k = e - c * SV_GB;
      wt[c][k] = (c0 + c < m && k0 + k < dy) ? w[(c0 + c) * ldw + k0 + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SV_TR / 8; ++kk) {
      const int r = ty + 8 * kk;
#pragma unroll
      for (int k = 0; k < SV_GB; ++k) {
        acc[kk].x = fma(gm[r][k], wt[2 * tx][k], acc[kk].x);
        acc[kk].y = fma(gm[r][k], wt[2 * tx + 1][k], acc[kk].y);
      }
    }
  }
  __syncthreads();                                         // gv visible (dy == 0 never happens: validated)
#pragma unroll
  for (int kk = 0; kk < SV_TR / 8; ++kk) {
    const int r = ty + 8 * kk;
    const int64_t row = r0 + r;
    double2 a = make_double2(0.0, 0.0);
    if (row < rows && cc < m) {
      a = *reinterpret_cast<const double2*>(alpha + row * lda + cc);
      double2 t = *reinterpret_cast<const double2*>(T + row * ldt + cc);
      const double g2 = 2.0 * gv[r];
      t.x = fma(g2, t.x, acc[kk].x);
      if (cc + 1 < m) {
        t.y = fma(g2, t.y, acc[kk].y);
        *reinterpret_cast<double2*>(T + row * ldt + cc) = t;
      } else {
        a.y = 0.0;
        T[row * ldt + cc] = t.x;
      }
    }
    ta[r][2 * tx] = a.x;
    ta[r][2 * tx + 1] = a.y;
  }
  __syncthreads();
  // write side: 16 lanes cover the 32 rows of the tile as pairs, 16 columns of the tile per pass
  const int px = tid & 15, py = tid >> 4;
  const int64_t rr = r0 + 2 * px;                          // column index of the transposed operands
  const int64_t rpad = (rows + 15) / 16 * 16;
  if (rr < rpad) {                                         // rpad is even: rr + 1 < rpad as well
#pragma unroll
    for (int pass = 0; pass < SV_TC / 16; ++pass) {
      const int c = py + 16 * pass;
      if (c0 + c < m) {
        const double2 a = make_double2(ta[2 * px][c], ta[2 * px + 1][c]);
        const double2 g = make_double2(gv[2 * px] * a.x, gv[2 * px + 1] * a.y);
        *reinterpret_cast<double2*>(alphaT + (c0 + c) * ldo + rr) = a;
        *reinterpret_cast<double2*>(galphaT + (c0 + c) * ldo + rr) = g;
      }
    }
  }
}

static bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace gpn

using namespace gpn;

extern "C" int gpn_svgp_marginals(void* stream, const double* alpha, int64_t lda, const double* T, int64_t ldt, int64_t rows,
                                  int64_t m, const double* w, int64_t ldw, int dy, const double* kdiag, int64_t kdiag_stride,
                                  double* f_mean, double* f_var) {
  if (!alpha) return -2;
  if (lda < m) return -3;
  if (!T) return -4;
  if (ldt < m) return -5;
  if (rows <= 0) return -6;
  if (m <= 0) return -7;
  if (!w) return -8;
  if (dy <= 0) return -10;
  if (ldw < dy) return -9;
  if (!kdiag) return -11;
  if (kdiag_stride < 0) return -12;
  if (!f_mean) return -13;
  if (!f_var) return -14;
  if ((lda & 1) || (ldt & 1) || misaligned(alpha) || misaligned(T)) return GPN_E_ALIGN;
  const int64_t per_block = (int64_t)SV_WAVES * SV_RW;
  const int64_t blocks = (rows + per_block - 1) / per_block;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  hipLaunchKernelGGL(svgp_marginals_kernel, dim3((unsigned)blocks), dim3(SV_WAVES * 64), 0, static_cast<hipStream_t>(stream), alpha,
                     lda, T, ldt, rows, m, w, ldw, dy, kdiag, kdiag_stride, f_mean, f_var);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}

extern "C" int gpn_svgp_backward_rows(void* stream, const double* alpha, int64_t lda, double* T, int64_t ldt, int64_t rows,
                                      int64_t m, const double* w, int64_t ldw, int dy, const double* g_var, const double* g_mean,
                                      double* alphaT, double* galphaT, int64_t ldo) {
  if (!alpha) return -2;
  if (lda < m) return -3;
  if (!T) return -4;
  if (ldt < m) return -5;
  if (rows <= 0) return -6;
  if (m <= 0) return -7;
  if (!w) return -8;
  if (dy <= 0) return -10;
  if (ldw < dy) return -9;
  if (!g_var) return -11;
  if (!g_mean) return -12;
  if (!alphaT) return -13;
  if (!galphaT) return -14;
  if (ldo < (rows + 15) / 16 * 16) return -15;
  if ((lda & 1) || (ldt & 1) || (ldo & 1) || misaligned(alpha) || misaligned(T) || misaligned(alphaT) || misaligned(galphaT))
    return GPN_E_ALIGN;
  const int64_t rpad = (rows + 15) / 16 * 16;
  const int64_t gy = (rpad + SV_TR - 1) / SV_TR, gx = (m + SV_TC - 1) / SV_TC;
  if (gy > 65535) return GPN_E_UNSUPPORTED;
  hipLaunchKernelGGL(svgp_backward_rows_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, static_cast<hipStream_t>(stream), alpha,
                     lda, T, ldt, rows, m, w, ldw, dy, g_var, g_mean, alphaT, galphaT, ldo);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}
