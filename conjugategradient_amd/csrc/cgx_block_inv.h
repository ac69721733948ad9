// cgx_block_inv.h — block-Jacobi setup shared by the single solve
// (cgx_kernels.hip: k_block_inv, k_block_check) and the many-systems solve
// (cgx_many.hip: k_many_block_inv, k_many_block_check): the verdict on a
// diagonal or a pivot, one diagonal block's inverse, and a caller's row of W.
// tests/bj_model.py is the model of all three.
#pragma once

#include <hip/hip_runtime.h>

#include <limits>

namespace cgx {

// k_diag_inv's verdict on a diagonal, a pivot or a caller's m: positive and finite
template <typename T> __device__ __forceinline__ bool pc_ok(T d) {
  return d > T(0) && d <= std::numeric_limits<T>::max();  // false for NaN
}

// W_b = (the diagonal block of A at rows [b0, b0 + m))^-1 by LDL^T without
// pivoting, statement for statement tests/bj_model.py block_inverse and
// csr_blocks. Row i of the block takes the entries of CSR row b0 + i with
// b0 <= col <= b0 + i (the lower triangle decides; duplicates summed from 0 in
// entry order; rows may be unsorted); W = M^T D^-1 M with M = L^-1, the lower
// triangle computed and mirrored; the columns past a partial last block
// (m < BS) are +0.0. out is the matrix's W, n x BS row-major. Returns whether
// every pivot is positive and finite (pc_ok); where one is not, the block's W
// holds whatever the statements give. Idx is the caller's index type, so that
// its address arithmetic neither widens nor narrows.
template <int BS, typename Idx>
__device__ __forceinline__ bool block_inv_one(const int *__restrict__ rowptr,
                                              const int *__restrict__ col,
                                              const double *__restrict__ val,
                                              double *__restrict__ out, Idx b0, int m) {
  double B[BS][BS], L[BS][BS], M[BS][BS], D[BS], E[BS];
#pragma unroll
  for (int i = 0; i < BS; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) B[i][j] = 0.0;
    if (i < m) {
      for (int k = rowptr[b0 + i]; k < rowptr[b0 + i + 1]; ++k) {
        const Idx c = (Idx)col[k] - b0;
        const double v = val[k];
#pragma unroll
        for (int j = 0; j <= i; ++j)
          if (c == j) B[i][j] = B[i][j] + v;
      }
    }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < BS; ++j) {
    if (j < m) {
      double s = B[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - L[j][k] * (L[j][k] * D[k]);
      D[j] = s;
      if (!pc_ok(s)) ok = false;
#pragma unroll
      for (int i = j + 1; i < BS; ++i) {
        if (i < m) {
          double t = B[i][j];
#pragma unroll
          for (int k = 0; k < j; ++k) t = t - L[i][k] * (L[j][k] * D[k]);
          L[i][j] = t / s;
        }
      }
      E[j] = 1.0 / s;
    }
  }
  // M = L^-1 (unit lower triangle): M[i][j] = -(L[i][j] + sum_{j<k<i} L[i][k] M[k][j])
#pragma unroll
  for (int i = 1; i < BS; ++i) {
    if (i < m) {
#pragma unroll
      for (int j = 0; j < i; ++j) {
        double s = L[i][j];
#pragma unroll
        for (int k = j + 1; k < i; ++k) s = s + L[i][k] * M[k][j];
        M[i][j] = -s;
      }
    }
  }
  // W = M^T D^-1 M, the lower triangle computed and mirrored
#pragma unroll
  for (int i = 0; i < BS; ++i) {
    if (i < m) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double s = j == i ? E[i] : M[i][j] * E[i];
#pragma unroll
        for (int k = i + 1; k < BS; ++k)
          if (k < m) s = s + (M[k][i] * E[k]) * (j == i ? M[k][i] : M[k][j]);
        out[(b0 + i) * BS + j] = s;
        out[(b0 + j) * BS + i] = s;
      }
#pragma unroll
      for (int j = 0; j < BS; ++j)
        if (j >= m) out[(b0 + i) * BS + j] = 0.0;
    }
  }
  return ok;
}

// A caller's W, one row: w the row's bs values, d the row's place in its
// block, nc the block's real columns. W_b[i, i] positive and finite (pc_ok),
// every entry of a real column finite.
__device__ __forceinline__ bool block_row_ok(const double *__restrict__ w, int d, int nc) {
  bool ok = pc_ok(w[d]);
  for (int j = 0; j < nc; ++j)
    if (!(fabs(w[j]) <= std::numeric_limits<double>::max())) ok = false;  // NaN, Inf
  return ok;
}

}  // namespace cgx
