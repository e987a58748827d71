// Streamed quadratic cones whose inner-product matrix is Q = S + F diag(sigma) F' (cxk_add_quadratic_structured): S an
// n x n matrix held by its nonzeros in CSR (multiplied as given, both triangles stored), F n x rank column-major, sigma
// of either sign.  Q is never formed.  These kernels replace the ONE place where the streamed route reads Q, the pass
// out_r = Q x_r of quad_stream_qmv<R>: they leave the result in split slot 0 of QuadStreamGroup::part with splits = 1,
// so that QuadStreamQx and every kernel of kernels_quad_stream.hip.h read it as they read the dense pass.
//
// A pass is at most two launches:
//   quad_struct_dots<R>     the factor dots F' x_r: grid cone x factor x row segment, each workgroup strides down its
//                           segment of one column of F (coalesced), BlockSum, one partial per segment.  Not launched
//                           when rank = 0.
//   quad_struct_rows<R, L>  grid cone x row tile of 256 rows.  (S x_r)_i is a fixed chain over the row's nonzeros: L
//                           lanes per row (1, 8 or 64), lane l takes entries l, l + L, ..., a fixed butterfly combines
//                           the lanes; x is gathered from global memory through L2 (n has no LDS bound here).  Then
//                           (F t)_i with t = sigma o (F' x_r): t staged in LDS 64 entries at a time, the segment
//                           partials added in segment order while staging, F read coalesced across the tile for each
//                           factor.
// At cxk_finalize quad_struct_sa forms T = S A1 for A_gram = A1' S A1 + (F' A1)' diag(sigma) (F' A1), the products on
// the batched GEMM (cone_quad.hip: QuadStructuredGram); quad_struct_scale_rows makes sigma o (F' A1).
//
// The streamed route's rules hold: no atomics, no workgroup waits for another, every order of summation depends on the
// shape and the launch shape only (same bits every run), no scratch.  Duplicate entries of a row are summed by the
// chain like any two entries (with L = 1 in the order they are stored).
// Bytes per pass: 12 nnz (value and column) + 8 n rank (F, read twice when rank > 0: 16 n rank) + O(n), against 8 n^2.
#pragma once
#include "kernels_quad_stream.hip.h"

namespace cxk {

constexpr int kQuadStructTChunk = 64;  // entries of t staged in LDS at a time
constexpr int kQuadStructColTile = 4;  // columns of A1 one thread of quad_struct_sa carries

struct QuadStructured {
  int n, count, rank, segs, has_s;
  const long long* rowptr;  // count x (n + 1): a member's rows in col / val (absolute: the members' lists are concatenated)
  const int* col;
  const double* val;
  const double* F;      // count x n x rank
  const double* sigma;  // count x rank
  double* tpart;        // count x 2 x rank x segs   segment partials of F' x_0, F' x_1
  double* part;         // count x 2 x n             QuadStreamGroup::part with splits = 1
};

// ---- the factor dots.  Workgroup (cone, factor, segment).
template <int R>
__global__ void __launch_bounds__(kQuadStreamBlock) quad_struct_dots(QuadStructured g, QuadStreamVecs x) {
  __shared__ double scratch[kQuadStreamBlock / 64];
  const int n = g.n, segs = g.segs, rank = g.rank, tid = threadIdx.x;
  const int seg = (int)(blockIdx.x % segs);
  const size_t t = blockIdx.x / segs;
  const int k = (int)(t % rank);
  const size_t mem = t / rank;
  const int per = (n + segs - 1) / segs;
  const int i0 = min(n, seg * per), i1 = min(n, i0 + per);
  const double* f = g.F + (mem * rank + k) * (size_t)n;
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; r++) acc[r] = 0;
  for (int i = i0 + tid; i < i1; i += kQuadStreamBlock) {
    const double e = f[i];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = fma(e, x.p[r][mem * x.stride[r] + i], acc[r]);
  }
#pragma unroll
  for (int r = 0; r < R; r++) {
    const double s = BlockSum(acc[r], scratch);
    if (tid == 0) g.tpart[((mem * 2 + r) * rank + k) * (size_t)segs + seg] = s;
  }
}

// ---- the rows.  Workgroup (cone, row tile); L lanes per row of S, then one row per thread for F t.
template <int R, int L>
__global__ void __launch_bounds__(kQuadStreamBlock) quad_struct_rows(QuadStructured g, QuadStreamVecs x, int tiles) {
  __shared__ double st[R][kQuadStructTChunk];
  __shared__ double srow[L > 1 ? R : 1][L > 1 ? kQuadStreamRowTile : 1];
  const int n = g.n, rank = g.rank, segs = g.segs, tid = threadIdx.x;
  const size_t mem = blockIdx.x / tiles;
  const int row0 = (int)(blockIdx.x % tiles) * kQuadStreamRowTile;
  const int i = row0 + tid;
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; r++) acc[r] = 0;
  if (g.has_s) {
    const long long* rp = g.rowptr + mem * ((size_t)n + 1);
    if (L == 1) {
      if (i < n) {
        for (long long e = rp[i]; e < rp[i + 1]; e++) {
          const double v = g.val[e];
          const int c = g.col[e];
#pragma unroll
          for (int r = 0; r < R; r++) acc[r] = fma(v, x.p[r][mem * x.stride[r] + c], acc[r]);
        }
      }
    } else {
      constexpr int kRows = kQuadStreamRowTile / L;  // rows of one sweep of the workgroup
      const int lane = tid % L, sub = tid / L;
      for (int p = 0; p < L; p++) {
        const int loc = p * kRows + sub, row = row0 + loc;
        long long e0 = 0, e1 = 0;
        if (row < n) {
          e0 = rp[row];
          e1 = rp[row + 1];
        }
        double a[R];
#pragma unroll
        for (int r = 0; r < R; r++) a[r] = 0;
        for (long long e = e0 + lane; e < e1; e += L) {
          const double v = g.val[e];
          const int c = g.col[e];
#pragma unroll
          for (int r = 0; r < R; r++) a[r] = fma(v, x.p[r][mem * x.stride[r] + c], a[r]);
        }
        // (every lane of the wavefront is here: a row's L lanes share e0 and e1, a row past the end has none)
#pragma unroll
        for (int off = L / 2; off >= 1; off >>= 1) {
#pragma unroll
          for (int r = 0; r < R; r++) a[r] += __shfl_xor(a[r], off, L);
        }
        if (lane == 0) {
#pragma unroll
          for (int r = 0; r < R; r++) srow[r][loc] = a[r];
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < R; r++) acc[r] = srow[r][tid];
    }
  }
  for (int k0 = 0; k0 < rank; k0 += kQuadStructTChunk) {
    const int kn = min(kQuadStructTChunk, rank - k0);
    __syncthreads();  // the previous chunk has been read
    if (tid < kn) {
#pragma unroll
      for (int r = 0; r < R; r++) {
        const double* tp = g.tpart + ((mem * 2 + r) * rank + k0 + tid) * (size_t)segs;
        double s = 0;
        for (int q = 0; q < segs; q++) s += tp[q];
        st[r][tid] = g.sigma[mem * rank + k0 + tid] * s;
      }
    }
    __syncthreads();
    if (i < n) {
      const double* f = g.F + (mem * rank + k0) * (size_t)n + i;
#pragma unroll 8
      for (int j = 0; j < kn; j++) {
        const double e = f[(size_t)j * n];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = fma(e, st[r][j], acc[r]);
      }
    }
  }
  if (i < n) {
#pragma unroll
    for (int r = 0; r < R; r++) g.part[(mem * 2 + r) * (size_t)n + i] = acc[r];
  }
}

// ---- once, at cxk_finalize: T = S A1 (n x m per cone, leading dimension n; A1 = A + 1 with leading dimension n + 1).
// Workgroup (cone, row tile, tile of kQuadStructColTile columns): one row per thread, one chain per column.
__global__ void __launch_bounds__(kQuadStreamBlock) quad_struct_sa(QuadStructured g, const double* A, int m, double* T, int tiles,
                                                                   int ctiles) {
  const int n = g.n, len = n + 1;
  const int ct = (int)(blockIdx.x % ctiles);
  const size_t t = blockIdx.x / ctiles;
  const int i = (int)(t % tiles) * kQuadStreamRowTile + threadIdx.x;
  const size_t mem = t / tiles;
  if (i >= n) return;
  const int j0 = ct * kQuadStructColTile, jn = min(kQuadStructColTile, m - j0);
  const long long* rp = g.rowptr + mem * ((size_t)n + 1);
  const double* A1 = A + (mem * m + j0) * (size_t)len + 1;
  double acc[kQuadStructColTile];
#pragma unroll
  for (int j = 0; j < kQuadStructColTile; j++) acc[j] = 0;
  for (long long e = rp[i]; e < rp[i + 1]; e++) {
    const double v = g.val[e];
    const int c = g.col[e];
#pragma unroll
    for (int j = 0; j < kQuadStructColTile; j++)
      if (j < jn) acc[j] = fma(v, A1[(size_t)j * len + c], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < kQuadStructColTile; j++)
    if (j < jn) T[(mem * m + j0 + j) * (size_t)n + i] = acc[j];
}

// ---- once, at cxk_finalize: out = diag(sigma) P for the rank x m matrix P = F' A1 of every cone.
__global__ void __launch_bounds__(kQuadStreamBlock) quad_struct_scale_rows(QuadStructured g, const double* P, int m, double* out) {
  const size_t per = (size_t)g.rank * m, total = per * g.count;
  const size_t idx = (size_t)blockIdx.x * kQuadStreamBlock + threadIdx.x;
  if (idx >= total) return;
  const size_t mem = idx / per;
  const int k = (int)((idx % per) % g.rank);
  out[idx] = g.sigma[mem * g.rank + k] * P[idx];
}

}  // namespace cxk
