// Block triangular solves with the stored supernodal factor for a BLOCK of right-hand sides
// (cxk_solve_block): the level-scheduled forward and back substitution of kernels_tree_level.hip.h with
// kSbW columns per workgroup instead of one.
//
// Layout.  The right-hand sides live in a buffer of this feature's own, permuted and cut into chunks
// of kSbW columns:  X[(chunk * N + p) * kSbW + j]  is row p (permuted order) of column chunk * kSbW + j,
// so the kSbW values of a row are one 256-byte line and lane j of a half wavefront owns column j.  The
// forward-solve contributions  t = off^T b  go to slots as in the single-vector kernels
// (FactorPlan::pubb_dst / fs_ptr / fs_src: a child publishes into slots of its own, the ancestor pulls them
// in list order), kSbW wide:  T[chunk * slot_stride + slot * kSbW + j].  No atomics, no arrival words:
// one launch per level, workgroup (position, chunk) depends on earlier launches only.
//
// One workgroup of 256 threads per supernode and chunk: thread (j = tid & 31, g = tid >> 5).  The factor
// streams through LDS once per chunk in tiles of kSbRT rows x kSbKB columns (any supernode size: the slab
// layout is the same behind every factor route -- diagonal block ns x ns column-major with L in its lower
// triangle, off block ns x s column-major); the rows of X being solved sit in LDS (32 x kSbW) and, during
// the 32 x 32 triangular solve, in the registers of the column's thread.  Every product is a fixed-order
// fma chain, and column j of the result is computed from column j of the input alone.
//
// LDLT contexts (tree_sweep_block_ldlt): the factor is P^T L D L^T P per supernode with unit-lower L and the
// (clamped) pivots on the diagonal; the off block holds D^-1 L^-1 P off.  Forward: transpositions, unit-lower
// solve, publish, then D^-1.  Backward: separator terms, unit-lower-transposed solve, transpositions reversed.
#pragma once
#include "tree_supernode.hip.h"

namespace cxk {

constexpr int kSbW = 32;        // columns per chunk
constexpr int kSbKB = 32;       // columns of L per block step
constexpr int kSbRT = 64;       // rows of L per streamed tile
constexpr int kSbThreads = 256;

struct SolveBlockArgs {
  FactorPlan P;
  const double* slab;
  double* X;              // [chunks][N][kSbW]
  double* T;              // [chunks][slot_stride]
  const int* tr;          // LDLT: transpositions by first permuted index (null otherwise)
  int N;
  long long slot_stride;  // doubles per chunk in T
  int base;               // first position of the level in the level-ordered records
};

// sL[k * kSbRT + i] = src[(i0 + i) + col(k) * ld] for i < rt, k < nc; zero elsewhere
template <typename Col>
__device__ __forceinline__ void SbStageTile(double* __restrict__ sL, const double* __restrict__ src, int ld, int i0,
                                            int rt, int nc, Col col) {
#pragma unroll
  for (int u = 0; u < kSbRT * kSbKB / kSbThreads; u++) {
    const int e = threadIdx.x + u * kSbThreads, i = e & (kSbRT - 1), k = e >> 6;
    sL[e] = (i < rt && k < nc) ? src[(size_t)(i0 + i) + (size_t)col(k) * ld] : 0.0;
  }
}

// sX[i * kSbW + j] = X[(row0 + i) * kSbW + j], i < rt (of `rows` staged rows); zero elsewhere
__device__ __forceinline__ void SbStageRows(double* __restrict__ sX, const double* X, int row0, int rt, int rows) {
  for (int e = threadIdx.x; e < rows * kSbW; e += kSbThreads) {
    const int i = e >> 5;
    sX[e] = i < rt ? X[(size_t)(row0 + i) * kSbW + (e & 31)] : 0.0;
  }
}

// X[row0 + i][j] -= sum_k sL[k][i] sXk[k][j], i < rt: rows g, g + 8, ... of the tile
__device__ __forceinline__ void SbSubtractTile(double* X, int row0, int rt, const double* __restrict__ sL,
                                               const double* __restrict__ sXk, int nk) {
  const int j = threadIdx.x & 31, g = threadIdx.x >> 5;
#pragma unroll
  for (int u = 0; u < kSbRT / 8; u++) {
    const int i = g + 8 * u;
    if (i < rt) {
      double* x = X + (size_t)(row0 + i) * kSbW + j;
      double acc = *x;
      for (int k = 0; k < nk; k++) acc = fma(-sL[k * kSbRT + i], sXk[k * kSbW + j], acc);
      *x = acc;
    }
  }
}

// acc[u] += sum_i sL[c][i] sX[i][j], c = g + 8 u
__device__ __forceinline__ void SbDotTile(double (&acc)[4], int rt, const double* __restrict__ sL,
                                          const double* __restrict__ sX) {
  const int j = threadIdx.x & 31, g = threadIdx.x >> 5;
  for (int i = 0; i < rt; i++) {
    const double xv = sX[i * kSbW + j];
#pragma unroll
    for (int u = 0; u < 4; u++) acc[u] = fma(sL[(g + 8 * u) * kSbRT + i], xv, acc[u]);
  }
}

// the kb x kb diagonal block at (k0, k0): strictly lower part into sL[col * kSbRT + row], reciprocals of the
// diagonal (1.0 for LDLT's unit-lower factor and for padding) into sDinv
template <bool LDLT>
__device__ __forceinline__ void SbStageDiag(double* __restrict__ sL, double* __restrict__ sDinv,
                                            const double* __restrict__ D, int ns, int k0, int kb) {
#pragma unroll
  for (int u = 0; u < kSbRT * kSbKB / kSbThreads; u++) {
    const int e = threadIdx.x + u * kSbThreads, i = e & (kSbRT - 1), k = e >> 6;
    sL[e] = (i < kb && k < i) ? D[(size_t)(k0 + i) + (size_t)(k0 + k) * ns] : 0.0;
  }
  if (threadIdx.x < kSbKB) {
    const int k = threadIdx.x;
    sDinv[k] = (!LDLT && k < kb) ? 1.0 / D[(size_t)(k0 + k) * (size_t)(ns + 1)] : 1.0;
  }
}

// LDLT: the supernode's transpositions applied to the rows of X, forward (k ascending) or reversed
__device__ __forceinline__ void SbTranspositions(double* X, const int* __restrict__ tr, int st, int ns, bool forward) {
  if (threadIdx.x >= kSbW) return;
  const int j = threadIdx.x;
  for (int q = 0; q < ns; q++) {
    const int k = forward ? q : ns - 1 - q, t = tr[st + k];
    if (t != k) {
      double* a = X + (size_t)(st + k) * kSbW + j;
      double* b = X + (size_t)(st + t) * kSbW + j;
      const double v = *a;
      *a = *b;
      *b = v;
    }
  }
}

// B_sn <- L^-1 (B_sn - pulled contributions), publish T = off^T B_sn   (LDLT: see the head of this file)
template <bool LDLT>
__global__ void __launch_bounds__(kSbThreads) solve_block_forward(SolveBlockArgs a) {
  __shared__ double sL[kSbRT * kSbKB], sX[kSbRT * kSbW], sXk[kSbKB * kSbW], sDinv[kSbKB];
  const SnRec R = LoadRec(a.P.rec, a.base + blockIdx.x);
  const int ns = R.ns, s = R.nsep, st = R.start, tid = threadIdx.x, j = tid & 31, g = tid >> 5;
  double* X = a.X + (size_t)blockIdx.y * a.N * kSbW;
  double* T = a.T + (size_t)blockIdx.y * a.slot_stride;
  const double* D = a.slab + R.diag_off;
  const double* B = a.slab + R.offd_off;
  for (int e = tid; e < ns * kSbW; e += kSbThreads) {
    const int row = st + (e >> 5);
    double acc = X[(size_t)row * kSbW + j];
    const int q1 = a.P.fs_ptr[row + 1];
    for (int q = a.P.fs_ptr[row]; q < q1; q++) acc -= T[(size_t)a.P.fs_src[q] * kSbW + j];
    X[(size_t)row * kSbW + j] = acc;
  }
  __syncthreads();
  if constexpr (LDLT) {
    SbTranspositions(X, a.tr, st, ns, true);
    __syncthreads();
  }
  for (int k0 = 0; k0 < ns; k0 += kSbKB) {
    const int kb = min(kSbKB, ns - k0);
    SbStageDiag<LDLT>(sL, sDinv, D, ns, k0, kb);
    SbStageRows(sXk, X, st + k0, kb, kSbKB);
    __syncthreads();
    if (tid < kSbW) {
      double x[kSbKB];
#pragma unroll
      for (int k = 0; k < kSbKB; k++) x[k] = sXk[k * kSbW + j];
#pragma unroll
      for (int k = 0; k < kSbKB; k++)
        if (k < kb) {
          x[k] *= sDinv[k];
#pragma unroll
          for (int i = k + 1; i < kSbKB; i++) x[i] = fma(-sL[k * kSbRT + i], x[k], x[i]);
        }
#pragma unroll
      for (int k = 0; k < kSbKB; k++) {
        sXk[k * kSbW + j] = x[k];
        if (k < kb) X[(size_t)(st + k0 + k) * kSbW + j] = x[k];
      }
    }
    __syncthreads();
    for (int i0 = k0 + kSbKB; i0 < ns; i0 += kSbRT) {
      const int rt = min(kSbRT, ns - i0);
      SbStageTile(sL, D, ns, i0, rt, kb, [&](int k) { return k0 + k; });
      __syncthreads();
      SbSubtractTile(X, st + i0, rt, sL, sXk, kb);
      __syncthreads();
    }
  }
  const int* dst = a.P.pubb_dst + R.updb_off;
  for (int c0 = 0; c0 < s; c0 += kSbKB) {
    const int cb = min(kSbKB, s - c0);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i0 = 0; i0 < ns; i0 += kSbRT) {
      const int rt = min(kSbRT, ns - i0);
      SbStageTile(sL, B, ns, i0, rt, cb, [&](int k) { return c0 + k; });
      SbStageRows(sX, X, st + i0, rt, kSbRT);
      __syncthreads();
      SbDotTile(acc, rt, sL, sX);
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int c = g + 8 * u;
      if (c < cb) T[(size_t)dst[c0 + c] * kSbW + j] = acc[u];
    }
  }
  if constexpr (LDLT) {
    __syncthreads();
    for (int e = tid; e < ns * kSbW; e += kSbThreads) {
      const int i = e >> 5;
      double* x = X + (size_t)(st + i) * kSbW + j;
      *x = (1.0 / D[(size_t)i * (size_t)(ns + 1)]) * *x;
    }
  }
}

// B_sn <- L^-T (B_sn - off X_sep)   (LDLT: see the head of this file)
template <bool LDLT>
__global__ void __launch_bounds__(kSbThreads) solve_block_backward(SolveBlockArgs a) {
  __shared__ double sL[kSbRT * kSbKB], sX[kSbRT * kSbW], sXk[kSbKB * kSbW], sDinv[kSbKB];
  const SnRec R = LoadRec(a.P.rec, a.base + blockIdx.x);
  const int ns = R.ns, st = R.start, tid = threadIdx.x, j = tid & 31, g = tid >> 5;
  double* X = a.X + (size_t)blockIdx.y * a.N * kSbW;
  const double* D = a.slab + R.diag_off;
  const double* B = a.slab + R.offd_off;
  const int cnt = R.bs_end - R.bs_beg;
  for (int q0 = 0; q0 < cnt; q0 += kSbKB) {  // separator terms, in the list's order
    const int qb = min(kSbKB, cnt - q0);
    const int* bc = a.P.bs_c + R.bs_beg + q0;
    const int* br = a.P.bs_row + R.bs_beg + q0;
    for (int e = tid; e < kSbKB * kSbW; e += kSbThreads) {
      const int q = e >> 5;
      sXk[e] = q < qb ? X[(size_t)br[q] * kSbW + j] : 0.0;
    }
    for (int i0 = 0; i0 < ns; i0 += kSbRT) {
      const int rt = min(kSbRT, ns - i0);
      SbStageTile(sL, B, ns, i0, rt, qb, [&](int k) { return bc[k]; });
      __syncthreads();
      SbSubtractTile(X, st + i0, rt, sL, sXk, qb);
      __syncthreads();
    }
  }
  for (int k0 = ((ns - 1) / kSbKB) * kSbKB; ns > 0 && k0 >= 0; k0 -= kSbKB) {
    const int kb = min(kSbKB, ns - k0);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i0 = k0 + kSbKB; i0 < ns; i0 += kSbRT) {  // rows already solved, below the block
      const int rt = min(kSbRT, ns - i0);
      SbStageTile(sL, D, ns, i0, rt, kb, [&](int k) { return k0 + k; });
      SbStageRows(sX, X, st + i0, rt, kSbRT);
      __syncthreads();
      SbDotTile(acc, rt, sL, sX);
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = g + 8 * u;
      sXk[k * kSbW + j] = k < kb ? X[(size_t)(st + k0 + k) * kSbW + j] - acc[u] : 0.0;
    }
    SbStageDiag<LDLT>(sL, sDinv, D, ns, k0, kb);
    __syncthreads();
    if (tid < kSbW) {
      double x[kSbKB];
#pragma unroll
      for (int k = 0; k < kSbKB; k++) x[k] = sXk[k * kSbW + j];
#pragma unroll
      for (int k = kSbKB - 1; k >= 0; k--)
        if (k < kb) {
          x[k] *= sDinv[k];
#pragma unroll
          for (int i = 0; i < k; i++) x[i] = fma(-sL[i * kSbRT + k], x[k], x[i]);  // L[k][i]
        }
#pragma unroll
      for (int k = 0; k < kSbKB; k++)
        if (k < kb) X[(size_t)(st + k0 + k) * kSbW + j] = x[k];
    }
    __syncthreads();
  }
  if constexpr (LDLT) SbTranspositions(X, a.tr, st, ns, false);
}

// X[chunk][p][j] = Y[pinv[p] + (chunk kSbW + j) ld] (zero beyond nrhs) / the way back
__global__ void __launch_bounds__(256) solve_block_gather(int N, int nrhs, int chunks, const int* __restrict__ pinv,
                                                          const double* __restrict__ Y, long long ld,
                                                          double* __restrict__ X) {
  const size_t total = (size_t)chunks * N * kSbW;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(e & 31);
    const size_t row = e >> 5;
    const int p = (int)(row % N);
    const long long col = (long long)(row / N) * kSbW + j;
    X[e] = col < nrhs ? Y[(size_t)pinv[p] + (size_t)col * ld] : 0.0;
  }
}
__global__ void __launch_bounds__(256) solve_block_scatter(int N, int nrhs, int chunks, const int* __restrict__ pinv,
                                                           const double* __restrict__ X, long long ld,
                                                           double* __restrict__ Y) {
  const size_t total = (size_t)chunks * N * kSbW;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(e & 31);
    const size_t row = e >> 5;
    const int p = (int)(row % N);
    const long long col = (long long)(row / N) * kSbW + j;
    if (col < nrhs) Y[(size_t)pinv[p] + (size_t)col * ld] = X[e];
  }
}

}  // namespace cxk
