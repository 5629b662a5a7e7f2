// The row kernels of the FITC marginal likelihood (Snelson & Ghahramani 2006; models/_fitc.py) around the contractions: with
// a_i = row i of A_c^T = K(x_c, Z) L^-T [rows, m] and lambda_i = kdiag_i - |a_i|^2 + noise,
//   forward rows:   lambda_i; a_i <- a_i / sqrt(lambda_i) in place; (err_i / sqrt(lambda_i))^T into the K-padded operand of
//                   the A err contraction; the chunk's sum log lambda_i and sum |err_i|^2 / lambda_i
//   backward rows:  with T = alpha [B^-1 | beta] (one dense contraction: alpha B^-1 in columns 0 .. m - 1, alpha beta from
//                   column round_up(m, 16) on), r_i = (err_i - alpha_i beta) / lambda_i, h_i = alpha_i . T_i,
//                   g_i = |r_i|^2 - dy (1 / lambda_i - h_i / lambda_i^2);  T_i <- r_i beta^T - (dy / lambda_i) T_i - g_i alpha_i
//                   (the rows of dF/dA^T, in place), and the transposed operands alpha^T and (diag(g) alpha)^T of the weighted
//                   accumulation A diag(g) A^T (g has both signs: a two-operand NT product, as in svgp.hip).
// Every sum has a fixed order (lane-strided partial sums, a shuffle tree, per-workgroup partials combined by a second
// kernel in a fixed order): the same inputs give the same bits; nothing is accumulated with atomics.
#include "rowkernels.h"

namespace gpn {

constexpr int FT_WAVES = 4;       // wavefronts per workgroup (forward rows)
constexpr int FT_RW = 4;          // rows per wavefront, one after the other

// One wavefront per row; lane l owns the column pairs 2l, 2l + 128, ... (16-byte accesses).  The first NP pairs of a lane
// stay in registers between the sum of squares and the scaling (NP = 8: m <= 1024, NP = 32: m <= 4096 -- one pass over HBM);
// pairs beyond them are read again (cache-resident: the wavefront has just read them).
template <int NP>
__global__ __launch_bounds__(FT_WAVES * 64) void fitc_forward_rows_kernel(double* __restrict__ At, int64_t lda, int64_t rows, int64_t m,
                                                                          const double* __restrict__ err, int dy,
                                                                          const double* __restrict__ kdiag, int64_t kds, double noise,
                                                                          double* __restrict__ errT, int64_t ldo,
                                                                          double* __restrict__ lambda, double* __restrict__ partials) {
  __shared__ double red[FT_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rpad = (rows + 15) / 16 * 16;
  double slog = 0.0, squad = 0.0;                        // (lane 0's are the wavefront's)
  const int mi = (int)m;                                 // (m < 2^31: validated)
#pragma unroll 1
  for (int q = 0; q < FT_RW; ++q) {
    const int64_t row = ((int64_t)blockIdx.x * FT_WAVES + wave) * FT_RW + q;   // wave-uniform
    if (row >= rpad) break;
    double* ar = At + row * lda;
    if (row >= rows) {                                   // K padding of the contractions that read the chunk: exact zeros
      for (int64_t j = 2 * lane; j < m; j += 128) *reinterpret_cast<double2*>(ar + j) = make_double2(0.0, 0.0);
      for (int k = lane; k < dy; k += 64) errT[(int64_t)k * ldo + row] = 0.0;
      continue;
    }
    double2 v[NP];
    double ss = 0.0;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int j = 2 * lane + 128 * t;
      const double2 a = *reinterpret_cast<const double2*>(ar + (j < mi ? j : 0));  // always a valid address: no branch per load
      v[t].x = j < mi ? a.x : 0.0;
      v[t].y = j + 1 < mi ? a.y : 0.0;                   // odd tail: the neighbour is padding
      ss = fma(v[t].x, v[t].x, ss);
      ss = fma(v[t].y, v[t].y, ss);
    }
    for (int64_t j = 2 * lane + 128 * NP; j < m; j += 128) {
      double2 a = *reinterpret_cast<const double2*>(ar + j);
      if (j + 1 >= m) a.y = 0.0;
      ss = fma(a.x, a.x, ss);
      ss = fma(a.y, a.y, ss);
    }
    ss = wave_sum_all(ss);
    const double lam = (kdiag[row * kds] - ss) + noise;
    const double sc = 1.0 / sqrt(lam);
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int j = 2 * lane + 128 * t;
      if (j + 1 < mi) *reinterpret_cast<double2*>(ar + j) = make_double2(v[t].x * sc, v[t].y * sc);
      else if (j < mi) ar[j] = v[t].x * sc;
    }
    for (int64_t j = 2 * lane + 128 * NP; j < m; j += 128) {
      const double2 a = *reinterpret_cast<const double2*>(ar + j);
      if (j + 1 < m) *reinterpret_cast<double2*>(ar + j) = make_double2(a.x * sc, a.y * sc);
      else ar[j] = a.x * sc;
    }
    double qd = 0.0;
    for (int k = lane; k < dy; k += 64) {
      const double e = err[row * dy + k] * sc;
      errT[(int64_t)k * ldo + row] = e;
      qd = fma(e, e, qd);
    }
    qd = wave_sum(qd);
    if (lane == 0) {
      lambda[row] = lam;
      slog += log(lam);
      squad += qd;
    }
  }
  if (lane == 0) {
    red[wave][0] = slog;
    red[wave][1] = squad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < FT_WAVES; ++w) {
      a += red[w][0];
      b += red[w][1];
    }
    partials[2 * (int64_t)blockIdx.x] = a;
    partials[2 * (int64_t)blockIdx.x + 1] = b;
  }
}

// second stage: out2 = the sums of the workgroups' partial pairs, in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void fitc_sum_partials_kernel(const double* __restrict__ partials, int64_t count, double* __restrict__ out2) {
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
    out2[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    out2[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
  }
}

__device__ inline double fitc_resid(const double* __restrict__ err, const double* T, int64_t ldt, int64_t mp, int dy, int64_t row, int k,
                                    double inv) {
  return (err[row * dy + k] - T[row * ldt + mp + k]) * inv;   // r_ik = (err_ik - alpha_i beta_k) / lambda_i
}

// A workgroup of 256 threads owns RK_TR rows over all columns.  Pass 1: one wavefront per row (8 rows each) forms h_i, r_i and
// g_i (16-byte loads, lane-strided sums, a shuffle tree).  Pass 2 walks the rows again in tiles of RK_TC columns with the tile
// pass of rowkernels.h (the one svgp_backward_rows_kernel runs once per workgroup): the rank-dy term r beta^T with the tile of
// beta and the rows' r staged in LDS, the update of T in place, and the tile of alpha out transposed, row pairs as 16-byte
// stores.  Columns rows .. round_up(rows, 16) - 1 of the transposed operands (the contractions' K padding) are exact zeros.
__global__ __launch_bounds__(256) void fitc_backward_rows_kernel(const double* __restrict__ alpha, int64_t lda, double* T, int64_t ldt,
                                                                 int64_t rows, int64_t m, int64_t mp, const double* __restrict__ beta,
                                                                 int64_t ldb, int dy, const double* __restrict__ err,
                                                                 const double* __restrict__ lambda, double* __restrict__ r_out,
                                                                 double* __restrict__ g_out, double* __restrict__ alphaT,
                                                                 double* __restrict__ galphaT, int64_t ldo) {
  __shared__ RowTile s;
  __shared__ double gs[RK_TR], ps[RK_TR], il[RK_TR];       // g_i, dy / lambda_i, 1 / lambda_i
  const int64_t r0 = (int64_t)blockIdx.x * RK_TR;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int q = 0; q < RK_TR / 4; ++q) {
    const int r = wave * (RK_TR / 4) + q;
    const int64_t row = r0 + r;                            // wave-uniform
    if (row < rows) {
      const double* ar = alpha + row * lda;
      const double* tr = T + row * ldt;
      double h = 0.0;
      for (int64_t j = 2 * lane; j < m; j += 128) {
        const double2 a = *reinterpret_cast<const double2*>(ar + j);
        const double2 t = *reinterpret_cast<const double2*>(tr + j);
        h = fma(a.x, t.x, h);
        if (j + 1 < m) h = fma(a.y, t.y, h);               // odd tail: the neighbour is padding
      }
      h = wave_sum(h);
      const double inv = 1.0 / lambda[row];
      double rr = 0.0;
      for (int k = lane; k < dy; k += 64) {
        const double rv = fitc_resid(err, T, ldt, mp, dy, row, k, inv);
        r_out[row * dy + k] = rv;
        rr = fma(rv, rv, rr);
      }
      rr = wave_sum(rr);
      if (lane == 0) {
        const double g = rr - dy * (inv - h * inv * inv);
        gs[r] = g;
        ps[r] = dy * inv;
        il[r] = inv;
        g_out[row] = g;
      }
    } else if (lane == 0) {
      gs[r] = 0.0;
      ps[r] = 0.0;
      il[r] = 0.0;
    }
  }
  __syncthreads();
  for (int64_t c0 = 0; c0 < m; c0 += RK_TC) {
    double2 acc[RK_TR / 8];
    tile_rank_term(s, acc, [&](int r, int64_t row, int k) { return fitc_resid(err, T, ldt, mp, dy, row, k, il[r]); }, beta, ldb, r0, rows,
                   c0, m, dy);
    tile_update(s, acc, alpha, lda, T, ldt, r0, rows, c0, m,
                [&](int r, double2 t, double2 a, double2 ac) {
                  const double pl = ps[r], g = gs[r];
                  return make_double2(ac.x - pl * t.x - g * a.x, ac.y - pl * t.y - g * a.y);
                });
    __syncthreads();
    tile_write_transposed(s, gs, alphaT, galphaT, ldo, r0, rows, c0, m);
  }
}

static int64_t fitc_forward_blocks(int64_t rows) {
  const int64_t per_block = (int64_t)FT_WAVES * FT_RW;
  return (round_up(rows, 16) + per_block - 1) / per_block;
}

}  // namespace gpn

using namespace gpn;

extern "C" int64_t gpn_fitc_forward_work_bytes(int64_t rows) { return rows <= 0 ? 0 : 2 * 8 * fitc_forward_blocks(rows); }

extern "C" int gpn_fitc_forward_rows(void* stream, double* At, int64_t lda, int64_t rows, int64_t m, const double* err, int dy,
                                     const double* kdiag, int64_t kdiag_stride, double noise, double* errT, int64_t ldo,
                                     double* lambda, double* work, double* out2) {
  if (!At) return -2;
  if (lda < m || lda < 2) return -3;
  if (rows <= 0) return -4;
  if (m <= 0 || m > 0x7ffffffe) return -5;
  if (!err) return -6;
  if (dy <= 0) return -7;
  if (!kdiag) return -8;
  if (kdiag_stride < 0) return -9;
  if (!(noise >= 0.0)) return -10;
  if (!errT) return -11;
  if (ldo < round_up(rows, 16)) return -12;
  if (!lambda) return -13;
  if (!work) return -14;
  if (!out2) return -15;
  if ((lda & 1) || misaligned(At)) return GPN_E_ALIGN;
  const int64_t blocks = fitc_forward_blocks(rows);
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (m <= 1024)
    hipLaunchKernelGGL(fitc_forward_rows_kernel<8>, dim3((unsigned)blocks), dim3(FT_WAVES * 64), 0, s, At, lda, rows, m, err, dy, kdiag,
                       kdiag_stride, noise, errT, ldo, lambda, work);
  else
    hipLaunchKernelGGL(fitc_forward_rows_kernel<32>, dim3((unsigned)blocks), dim3(FT_WAVES * 64), 0, s, At, lda, rows, m, err, dy, kdiag,
                       kdiag_stride, noise, errT, ldo, lambda, work);
  GPN_LAUNCH_CHECK();
  hipLaunchKernelGGL(fitc_sum_partials_kernel, dim3(1), dim3(256), 0, s, work, blocks, out2);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}

extern "C" int gpn_fitc_backward_rows(void* stream, const double* alpha, int64_t lda, double* T, int64_t ldt, int64_t rows, int64_t m,
                                      const double* beta, int64_t ldb, int dy, const double* err, const double* lambda, double* r_out,
                                      double* g_out, double* alphaT, double* galphaT, int64_t ldo) {
  if (!alpha) return -2;
  if (lda < m) return -3;
  if (!T) return -4;
  if (rows <= 0) return -6;
  if (m <= 0) return -7;
  if (!beta) return -8;
  if (dy <= 0) return -10;
  if (ldt < round_up(m, 16) + dy) return -5;
  if (ldb < dy) return -9;
  if (!err) return -11;
  if (!lambda) return -12;
  if (!r_out) return -13;
  if (!g_out) return -14;
  if (!alphaT) return -15;
  if (!galphaT) return -16;
  if (ldo < round_up(rows, 16)) return -17;
  if ((lda & 1) || (ldt & 1) || (ldo & 1) || misaligned(alpha) || misaligned(T) || misaligned(alphaT) || misaligned(galphaT))
    return GPN_E_ALIGN;
  const int64_t blocks = (round_up(rows, 16) + RK_TR - 1) / RK_TR;
  if (blocks > 0x7fffffff) return GPN_E_UNSUPPORTED;
  hipLaunchKernelGGL(fitc_backward_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), alpha, lda, T,
                     ldt, rows, m, round_up(m, 16), beta, ldb, dy, err, lambda, r_out, g_out, alphaT, galphaT, ldo);
  GPN_LAUNCH_CHECK();
  return GPN_OK;
}
