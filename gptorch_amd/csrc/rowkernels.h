// What the row kernels around the sparse models' contractions share (svgp.hip, fitc.hip).
#pragma once
#include "gpn_common.h"

namespace gpn {

// wavefront sum in a fixed order (shuffle tree); lane 0 holds the result
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// ... and every lane holds it
__device__ inline double wave_sum_all(double v) { return __shfl(wave_sum(v), 0, 64); }

// the row kernels read and write column pairs as 16-byte accesses
static inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// ---- the tile pass that the backward row kernels share ----------------------------------------------------------------------
// A workgroup of 256 threads works on a tile of RK_TR rows x RK_TC columns of alpha / T [rows, m].  Read side: thread (tx, ty)
// owns the column pair 2 tx of the rows ty, ty + 8, ... (16-byte accesses, coalesced along the row).  Write side: the tile of
// alpha goes out transposed from LDS, row pairs as 16-byte stores (coalesced along the rows of alpha^T).
constexpr int RK_TR = 32;         // rows of a tile
constexpr int RK_TC = 64;         // columns of a tile
constexpr int RK_GB = 8;          // columns of the rank-dy operands staged at a time

struct RowTile {
  double ta[RK_TR][RK_TC + 1];    // the tile of alpha
  double rv[RK_TR][RK_GB];        // [rows, dy] operand of the rank-dy term, RK_GB columns at a time
  double cv[RK_TC][RK_GB];        // [m, dy] operand likewise
};

// acc (rows ty + 8 kk, column pair 2 tx) = sum_k rowval(r, row, k) colmat[c, k]: the rank-dy term of the tile, both operands
// staged in LDS.  rowval(r, row, k): entry (row, k) of the [rows, dy] operand (r = row - r0); colmat [m, dy] (ldc).
template <class RowVal>
__device__ inline void tile_rank_term(RowTile& s, double2 (&acc)[RK_TR / 8], RowVal rowval, const double* __restrict__ colmat,
                                      int64_t ldc, int64_t r0, int64_t rows, int64_t c0, int64_t m, int dy) {
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
#pragma unroll
  for (int k = 0; k < RK_TR / 8; ++k) acc[k] = make_double2(0.0, 0.0);
  for (int k0 = 0; k0 < dy; k0 += RK_GB) {
    __syncthreads();
    {
      const int r = tid / RK_GB, k = tid - r * RK_GB;     // 32 x 8
      s.rv[r][k] = (r0 + r < rows && k0 + k < dy) ? rowval(r, r0 + r, k0 + k) : 0.0;
    }
    for (int e = tid; e < RK_TC * RK_GB; e += 256) {
      const int c = e / RK_GB, k = e - c * RK_GB;
      s.cv[c][k] = (c0 + c < m && k0 + k < dy) ? colmat[(c0 + c) * ldc + k0 + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < RK_TR / 8; ++kk) {
      const int r = ty + 8 * kk;
#pragma unroll
      for (int k = 0; k < RK_GB; ++k) {
        acc[kk].x = fma(s.rv[r][k], s.cv[2 * tx][k], acc[kk].x);
        acc[kk].y = fma(s.rv[r][k], s.cv[2 * tx + 1][k], acc[kk].y);
      }
    }
  }
}

// T[row, c] <- upd(r, T[row, c], alpha[row, c], acc) over the tile, a column pair (double2) at a time (in place), and the tile of alpha into s.ta (zeros outside
// rows x m).  The caller synchronises before tile_write_transposed.
template <class Upd>
__device__ inline void tile_update(RowTile& s, const double2 (&acc)[RK_TR / 8], const double* __restrict__ alpha, int64_t lda, double* T,
                                   int64_t ldt, int64_t r0, int64_t rows, int64_t c0, int64_t m, Upd upd) {
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int64_t cc = c0 + 2 * tx;
#pragma unroll
  for (int kk = 0; kk < RK_TR / 8; ++kk) {
    const int r = ty + 8 * kk;
    const int64_t row = r0 + r;
    double2 a = make_double2(0.0, 0.0);
    if (row < rows && cc < m) {
      a = *reinterpret_cast<const double2*>(alpha + row * lda + cc);
      double2 t = *reinterpret_cast<const double2*>(T + row * ldt + cc);
      t = upd(r, t, a, acc[kk]);
      if (cc + 1 < m) {
        *reinterpret_cast<double2*>(T + row * ldt + cc) = t;
      } else {
        a.y = 0.0;                                         // odd tail: the neighbour is padding
        T[row * ldt + cc] = t.x;
      }
    }
    s.ta[r][2 * tx] = a.x;
    s.ta[r][2 * tx + 1] = a.y;
  }
}

// alphaT [m, ldo] <- the tile of alpha transposed, galphaT <- (diag(wgt) alpha)^T (wgt [RK_TR]: the rows' weights, in LDS): 16
// lanes cover the 32 rows of the tile as pairs, 16 columns of the tile per pass.  Columns rows .. round_up(rows, 16) - 1 (the K
// padding of the contractions that read the transposed operands) come out as exact zeros: s.ta and wgt are zero there.
__device__ inline void tile_write_transposed(const RowTile& s, const double* wgt, double* __restrict__ alphaT, double* __restrict__ galphaT,
                                             int64_t ldo, int64_t r0, int64_t rows, int64_t c0, int64_t m) {
  const int tid = threadIdx.x, px = tid & 15, py = tid >> 4;
  const int64_t rr = r0 + 2 * px;                          // column index of the transposed operands
  const int64_t rpad = (rows + 15) / 16 * 16;
  if (rr < rpad) {                                         // rpad is even: rr + 1 < rpad as well
#pragma unroll
    for (int pass = 0; pass < RK_TC / 16; ++pass) {
      const int c = py + 16 * pass;
      if (c0 + c < m) {
        const double2 a = make_double2(s.ta[2 * px][c], s.ta[2 * px + 1][c]);
        const double2 g = make_double2(wgt[2 * px] * a.x, wgt[2 * px + 1] * a.y);
        *reinterpret_cast<double2*>(alphaT + (c0 + c) * ldo + rr) = a;
        *reinterpret_cast<double2*>(galphaT + (c0 + c) * ldo + rr) = g;
      }
    }
  }
}

}  // namespace gpn
