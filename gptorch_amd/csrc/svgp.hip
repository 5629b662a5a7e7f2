// The row kernels of the SVGP bound (gptorch/models/sparse_gpr.py:263-308, 337-381) around the contractions: with
// alpha = K(x_b, Z) L^-T [rows, m], T = alpha Q [rows, m] (Q = beta beta^T - I) and w = L^-1 m_u [m, dy],
//   marginals:      f_var_i = kdiag_i + sum_j alpha_ij T_ij,   f_mean0_i = alpha_i w           (sparse_gpr.py:367-377)
//   backward rows:  T <- G_alpha = 2 g_var_i T_i + g_mean_i w^T  (in place), and the transposed operands alpha^T and
//                   (diag(g_var) alpha)^T [m, rows] of the weighted SYRK alpha^T diag(g_var) alpha and of alpha^T g_mean.
// Both are one pass over HBM.  Every sum has a fixed order (lane-strided partial sums, then a shuffle tree): the same
// inputs give the same bits, whatever the scheduling; nothing is accumulated with atomics.
#include "rowkernels.h"

namespace gpn {

constexpr int SV_WAVES = 4;       // wavefronts per workgroup (marginals)
constexpr int SV_RW = 4;          // rows per wavefront
constexpr int SV_JT = 1024;       // columns of w staged in LDS at a time
constexpr int SV_DYB = 4;         // output columns per pass over a row

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

// Tile (RK_TR rows x RK_TC columns, rowkernels.h) per workgroup of 256 threads: the rank-dy term g_mean w^T, the update of T in
// place, and the tile of alpha out transposed.  Rows rows .. round_up(rows, 16) - 1 (the K padding of the contractions that
// read the transposed operands) are written as exact zeros.
__global__ __launch_bounds__(256) void svgp_backward_rows_kernel(const double* __restrict__ alpha, int64_t lda, double* __restrict__ T,
                                                                 int64_t ldt, int64_t rows, int64_t m, const double* __restrict__ w,
                                                                 int64_t ldw, int dy, const double* __restrict__ g_var,
                                                                 const double* __restrict__ g_mean, double* __restrict__ alphaT,
                                                                 double* __restrict__ galphaT, int64_t ldo) {
  __shared__ RowTile s;
  __shared__ double gv[RK_TR];
  const int64_t r0 = (int64_t)blockIdx.y * RK_TR, c0 = (int64_t)blockIdx.x * RK_TC;
  const int tid = threadIdx.x;
  if (tid < RK_TR) gv[tid] = (r0 + tid < rows) ? g_var[r0 + tid] : 0.0;
  double2 acc[RK_TR / 8];
  tile_rank_term(s, acc, [=](int, int64_t row, int k) { return g_mean[row * dy + k]; }, w, ldw, r0, rows, c0, m, dy);
  __syncthreads();                                         // gv visible (dy == 0 never happens: validated)
  tile_update(s, acc, alpha, lda, T, ldt, r0, rows, c0, m, [&](int r, double2 t, double2, double2 ac) {
    const double g2 = 2.0 * gv[r];
    return make_double2(fma(g2, t.x, ac.x), fma(g2, t.y, ac.y));
  });
  __syncthreads();
  tile_write_transposed(s, gv, alphaT, galphaT, ldo, r0, rows, c0, m);
}

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
  const int64_t gy = (rpad + RK_TR - 1) / RK_TR, gx = (m + RK_TC - 1) / RK_TC;
  if (gy > 65535) return GPN_E_UNSUPPORTED;
  hipLaunchKernelGGL(svgp_backward_rows_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, static_cast<hipStream_t>(stream), alpha,
                     lda, T, ldt, rows, m, w, ldw, dy, g_var, g_mean, alphaT, galphaT, ldo);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}
