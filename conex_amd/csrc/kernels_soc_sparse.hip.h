// Second-order cones on the sparse route (cxk_set_sparse_soc): the cone's (n + 1) x m matrix is held as its nonzeros,
// by rows (CSR, columns ascending) and by columns (CSC, rows ascending), and its dense A never reaches the device.
// With J = diag(-1, 1, .., 1), Q(w) = 2 w w' + det(w) J and Q(w^{1/2})^2 = Q(w) the Schur block is
//   G = 2 A' Q(w) A = 4 u u' + 2 det(w) H,   u = A' w,   H = A' J A,
//   AW = 2 u,   AQc = 2 (2 (w . c) u + det(w) h),   h = A' J c,
//   sc = (2 w . c, 2 (2 (w . c)^2 + det(w) z)),   z = c' J c:
// H, h and z are constants, formed once at cxk_finalize by the kernels below; one assembly is nnz multiply-adds, one
// read of H and one write of G.  No len x m work space, no GEMM, no square root (quad_schur's form for Q = I).
//
// The discipline is the streamed route's: no atomics, no workgroup waits for another, a kernel reads only what an
// earlier launch on the stream wrote, and every sum has an order fixed by the cone's pattern and the launch shape:
// same bits every run.  A row's slack is one fma chain over its nonzeros in ascending column; fma(0, y_j, s) = s, so
// it is soc_stream_slack's chain over j = 0 .. m - 1, bit for bit, and what soc_stream_prepare and
// soc_stream_take_step (reused on a SocStreamGroup view of the group) make of it is the streamed route's.
//
// Members of a group have equal (n, m) but their own patterns: `eptr` gives each member's first nonzero in the
// group's arrays, rowptr / colptr are relative to it.
#pragma once
#include "kernels_soc_stream.hip.h"  // SocStreamGroup: the step kernels serve this route too

namespace cxk {

constexpr int kSocSparseColChunk = 4096;   // doubles of a column of H one workgroup holds in LDS (32 KB)
constexpr int kSocSparseWaveCols = 512;    // widest cone whose columns of H one wavefront each assembles; 256 threads beyond
constexpr int kSocSparseBlock = 256;       // threads of every other kernel here
constexpr int kSocSparseCombineTile = 1024;  // entries of G one workgroup of soc_sparse_combine writes (four per thread)

struct SocSparseGroup {
  SocStreamGroup st;  // v: len = n + 1, m, count, c, W, T1, ids (v.A is null); s and ms (WA, wc, dets, Gf are null)
  const int* eptr;    // count + 1        first nonzero of each member
  const int* rowptr;  // count x (len + 1)
  const int* col;     // by rows, columns ascending within a row
  const double* val;
  const int* colptr;  // count x (m + 1)
  const int* crow;    // by columns, rows ascending within a column
  const double* cval;
  double* H;          // count x (m x m)  A' J A
  double* h;          // count x m        A' J c
  double* z;          // count            c' J c
  double* u;          // count x m        A' w of the last assembly
  double* scal;       // count x 2        det(w), w . c of the last assembly
};

// ---- the constants, once per cxk_finalize.  One workgroup per cone, column j and chunk of CHUNK entries k of that
// column: H[k, j] = sum over the rows r of column j, ascending, of a_rj (J_r a_rk), k running over row r's nonzeros
// (linear_sparse_schur's assembly with the weight -1 for row 0 and +1 for every other row in place of w_r^2).  Each
// wavefront owns a contiguous share of the chunk and walks every row of the column for the entries that fall into it:
// a row's columns are distinct, so lanes never collide, and rows follow one another in the wavefront's program order.
// The chunk leaves LDS coalesced, zeros included.  H[k, j] and H[j, k] see the same products in the same order: the
// square is exactly symmetric.  The first wavefront of chunk 0 also forms h_j = sum a_rj (J_r c_r): a lane's chain
// over every 64th row of the column, then WaveSum.
// CHUNK is kSocSparseColChunk under 256 threads, or kSocSparseWaveCols (the whole column) under one wavefront.
template <int CHUNK>
__global__ void __launch_bounds__(256) soc_sparse_gram(SocSparseGroup g, int chunks) {
  __shared__ double sH[CHUNK];
  const int len = g.st.v.len, m = g.st.v.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int chunk = (int)(blockIdx.x % chunks);
  const size_t cj = blockIdx.x / chunks;
  const int j = (int)(cj % m);
  const size_t mem = cj / m;
  const int k0 = chunk * CHUNK, cw = min(CHUNK, m - k0);
  const int span = (cw + nw - 1) / nw;
  const int lo = min(k0 + cw, k0 + wave * span), hi = min(k0 + cw, lo + span);  // this wavefront's entries of the column
  for (int k = lo + lane; k < hi; k += 64) sH[k - k0] = 0.0;
  WaveSync();
  const size_t base = (size_t)g.eptr[mem];
  const int* rowptr = g.rowptr + mem * ((size_t)len + 1);
  const int* colptr = g.colptr + mem * ((size_t)m + 1);
  const int* col = g.col + base;
  const double* val = g.val + base;
  const int* crow = g.crow + base;
  const double* cval = g.cval + base;
  const double* c = g.st.v.c + mem * len;
  const int e0 = colptr[j], e1 = colptr[j + 1];
  const bool sums = chunk == 0 && wave == 0;
  double hj = 0;
  for (int eb = e0; eb < e1; eb += 64) {
    // 64 rows of the column at a time: each lane fetches one row's entry, sign and extent
    const int e = eb + lane;
    int p0 = 0, p1 = 0;
    double a = 0, sg = 0;
    if (e < e1) {
      const int r = crow[e];
      a = cval[e];
      sg = r == 0 ? -1.0 : 1.0;
      p0 = rowptr[r];
      p1 = rowptr[r + 1];
      if (sums) hj = fma(a, sg * c[r], hj);
    }
    const int nb = min(64, e1 - eb);
    for (int i = 0; i < nb; i++) {
      const double ai = __shfl(a, i), sgi = __shfl(sg, i);
      const int s0 = __shfl(p0, i), s1 = __shfl(p1, i);
      for (int s = s0 + lane; s < s1; s += 64) {
        const int k = col[s];
        if (k >= lo && k < hi) sH[k - k0] = fma(ai, sgi * val[s], sH[k - k0]);
      }
      WaveSync();  // (the next row may touch the same entries from other lanes)
    }
  }
  __syncthreads();
  double* H = g.H + (mem * m + j) * (size_t)m + k0;
  for (int k = threadIdx.x; k < cw; k += blockDim.x) H[k] = sH[k];
  if (sums) {
    hj = WaveSum(hj);
    if (lane == 0) g.h[mem * m + j] = hj;
  }
}

// z = c' J c = sum_{k > 0} c_k^2 - c_0^2.  One workgroup per cone.
__global__ void __launch_bounds__(kSocSparseBlock) soc_sparse_cjc(SocSparseGroup g) {
  __shared__ double scratch[kSocSparseBlock / 64];
  const int len = g.st.v.len, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const double* c = g.st.v.c + mem * len;
  double q = 0;
  for (int k = tid; k < len; k += kSocSparseBlock)
    if (k > 0) q = fma(c[k], c[k], q);
  q = BlockSum(q, scratch);
  if (tid == 0) g.z[mem] = q - c[0] * c[0];
}

// ---- Schur complement, stage 1: det(w) = w_0^2 - |w_1|^2, w . c and the two scalars.  One workgroup per cone.
__global__ void __launch_bounds__(kSocSparseBlock) soc_sparse_vectors(SocSparseGroup g, Arena ar) {
  __shared__ double scratch[kSocSparseBlock / 64];
  const int len = g.st.v.len, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const int id = g.st.v.ids[mem];
  const double* w = g.st.v.W + mem * len;
  const double* c = g.st.v.c + mem * len;
  double t2 = 0, wc = 0;
  for (int k = tid; k < len; k += kSocSparseBlock) {
    const double wk = w[k];
    if (k > 0) t2 = fma(wk, wk, t2);
    wc = fma(wk, c[k], wc);
  }
  t2 = BlockSum(t2, scratch);
  wc = BlockSum(wc, scratch);
  if (tid == 0) {
    const double det = w[0] * w[0] - t2;
    g.scal[2 * mem] = det;
    g.scal[2 * mem + 1] = wc;
    ar.sc[2 * id] = 2 * wc;
    ar.sc[2 * id + 1] = 2 * ((2 * wc) * wc + det * g.z[mem]);
  }
}

// ---- stage 2: one wavefront per column j of a cone (four columns per workgroup): u_j = sum_r a_rj w_r through the
// CSC, each lane a chain over every 64th entry of the column in ascending row, then WaveSum; AW_j = 2 u_j and
// AQc_j = 2 (2 (w . c) u_j + det(w) h_j).
__global__ void __launch_bounds__(kSocSparseBlock) soc_sparse_dots(SocSparseGroup g, Arena ar) {
  const int len = g.st.v.len, m = g.st.v.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t cj = (size_t)blockIdx.x * (kSocSparseBlock / 64) + wave;
  if (cj >= (size_t)g.st.v.count * m) return;  // (whole wavefronts: nothing below waits for another)
  const int j = (int)(cj % m);
  const size_t mem = cj / m;
  const int id = g.st.v.ids[mem];
  const size_t base = (size_t)g.eptr[mem];
  const int* colptr = g.colptr + mem * ((size_t)m + 1);
  const int* crow = g.crow + base;
  const double* cval = g.cval + base;
  const double* w = g.st.v.W + mem * len;
  const int e1 = colptr[j + 1];
  double uj = 0;
  for (int e = colptr[j] + lane; e < e1; e += 64) uj = fma(cval[e], w[crow[e]], uj);
  uj = WaveSum(uj);
  if (lane == 0) {
    const double det = g.scal[2 * mem], wc = g.scal[2 * mem + 1];
    g.u[mem * m + j] = uj;
    ar.AWc[ar.r_off[id] + j] = 2 * uj;
    ar.AQcc[ar.r_off[id] + j] = 2 * ((2 * wc) * uj + det * g.h[mem * m + j]);
  }
}

// ---- stage 3: G[i, j] = fma(4 u_i, u_j, (2 det(w)) H[i, j]) over the full square, kSocSparseCombineTile consecutive
// entries per workgroup (coalesced reads of H and writes of G).  4 u_i u_j is one exact product whichever index comes
// first and H is exactly symmetric: so is G.
__global__ void __launch_bounds__(kSocSparseBlock) soc_sparse_combine(SocSparseGroup g, Arena ar, int tiles) {
  const int m = g.st.v.m, mm = m * m;
  const size_t mem = blockIdx.x / tiles;
  const int t0 = (int)(blockIdx.x % tiles) * kSocSparseCombineTile;
  const int id = g.st.v.ids[mem];
  const double* H = g.H + mem * mm;
  const double* u = g.u + mem * m;
  const double d2 = 2 * g.scal[2 * mem];
  double* G = ar.G + ar.g_off[id];
#pragma unroll
  for (int q = 0; q < kSocSparseCombineTile / kSocSparseBlock; q++) {
    const int idx = t0 + q * kSocSparseBlock + (int)threadIdx.x;
    if (idx < mm) {
      const int j = idx / m, i = idx - j * m;
      G[idx] = fma(4 * u[i], u[j], d2 * H[idx]);
    }
  }
}

// ---- PrepareStep / eigenvalue query, phase 1: ms_k = sum_j a_kj y[perm[j]] - c_k c_weight, one row per thread, the
// row's nonzeros in ascending column (soc_stream_slack's chain without its zero terms; no y staging: no width limit).
// Phase 2 is soc_stream_prepare<MODE>, TakeStep soc_stream_take_step.
__global__ void __launch_bounds__(kSocStreamBlock) soc_sparse_slack(SocSparseGroup g, StepArgs sa, int tiles) {
  sa.c_weight = CWeightOf(sa);  // (the barrier parameter may live on the device: cxk_select_mu_async)
  const int len = g.st.v.len, tid = threadIdx.x;
  const size_t mem = blockIdx.x / tiles;
  const int k = (int)(blockIdx.x % tiles) * kSocStreamRowTile + tid;
  if (k >= len) return;
  const int id = g.st.v.ids[mem];
  const size_t base = (size_t)g.eptr[mem];
  const int* rowptr = g.rowptr + mem * ((size_t)len + 1);
  const int* col = g.col + base;
  const double* val = g.val + base;
  const int* perm = sa.cl_perm + sa.cl_ptr[id];
  double acc = 0;
  const int s1 = rowptr[k + 1];
  for (int s = rowptr[k]; s < s1; s++) acc = fma(val[s], sa.y[perm[col[s]]], acc);
  g.st.ms[mem * len + k] = acc - g.st.v.c[mem * len + k] * sa.c_weight;
}

}  // namespace cxk
