// Linear-inequality blocks on the sparse route (cxk_set_sparse_linear): the block is held as its nonzeros, by rows
// (CSR, columns ascending) and by columns (CSC, rows ascending), and its dense A never reaches the device.  The
// Schur complement costs about sum_r nnz_r^2 multiply-adds plus one write of the m x m square, the slack passes
// nnz multiply-adds, where the dense routes (linear_schur, kernels_linear_tiled.hip.h) spend rows m^2 and rows m.
//
// The discipline is the tiled route's: no atomics, no workgroup waits for another, a kernel reads only what an
// earlier launch on the stream wrote, and every sum has an order fixed by the block's pattern: same bits every run.
// A row's slack is one fma chain over its nonzeros in ascending column; fma(0, y_j, s) = s, so it is the chain of
// the dense routes over j = 0 .. m - 1 and the per-row values, the per-tile partials and what linear_tiled_finish
// makes of them are the tiled route's, bit for bit.
//
// Members of a group have equal rows and m but their own patterns: `eptr` gives each member's first nonzero in the
// group's arrays, rowptr / colptr are relative to it.
#pragma once
#include "kernels_linear_tiled.hip.h"  // LinTiledGroup, LinTiledBlockMax, the finish kernels serve this route too

namespace cxk {

constexpr int kLinSparseColChunk = 4096;  // doubles of a column of G one workgroup holds in LDS (32 KB)
constexpr int kLinSparseWaveCols = 512;   // widest block whose columns one wavefront each assembles; 256 threads beyond

struct LinSparseGroup {
  LinTiledGroup t;    // v: len = rows, m, count, c, W, T1, T2, ids (v.A is null); part: four doubles per row tile
  const int* eptr;    // count + 1        first nonzero of each member
  const int* rowptr;  // count x (rows + 1)
  const int* col;     // by rows, columns ascending within a row
  const double* val;
  const int* colptr;  // count x (m + 1)
  const int* crow;    // by columns, rows ascending within a column
  const double* cval;
};

// ---- Schur complement (the block's two scalars are linear_tiled_scalars').  One workgroup per block, column j and
// chunk of CHUNK entries k of that column: G[k, j] = sum over the rows r of column j, ascending, of
// (w_r a_rj)(w_r a_rk), k running over row r's nonzeros.  Each wavefront owns a contiguous share of the chunk and
// walks every row of the column for the entries that fall into it: a row's columns are distinct, so lanes never
// collide, and rows follow one another in the wavefront's program order.  The chunk leaves LDS coalesced, zeros
// included.  G[k, j] and G[j, k] see the same products in the same order: the square is exactly symmetric.
// The first wavefront of chunk 0 also forms AW_j = sum a_rj w_r and AQc_j = sum (w_r a_rj)(w_r c_r): a lane's chain
// over every 64th row of the column, then WaveSum.
// CHUNK is kLinSparseColChunk under 256 threads, or kLinSparseWaveCols (the whole column, 4 KB: many workgroups per
// compute unit) under one wavefront.
template <int CHUNK>
__global__ void __launch_bounds__(256) linear_sparse_schur(LinSparseGroup g, Arena ar, int chunks) {
  __shared__ double sG[CHUNK];
  const int len = g.t.v.len, m = g.t.v.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int chunk = (int)(blockIdx.x % chunks);
  const size_t cj = blockIdx.x / chunks;
  const int j = (int)(cj % m);
  const size_t mem = cj / m;
  const int id = g.t.v.ids[mem];
  const int k0 = chunk * CHUNK, cw = min(CHUNK, m - k0);
  const int span = (cw + nw - 1) / nw;
  const int lo = min(k0 + cw, k0 + wave * span), hi = min(k0 + cw, lo + span);  // this wavefront's entries of the column
  for (int k = lo + lane; k < hi; k += 64) sG[k - k0] = 0.0;
  WaveSync();
  const size_t base = (size_t)g.eptr[mem];
  const int* rowptr = g.rowptr + mem * ((size_t)len + 1);
  const int* colptr = g.colptr + mem * ((size_t)m + 1);
  const int* col = g.col + base;
  const double* val = g.val + base;
  const int* crow = g.crow + base;
  const double* cval = g.cval + base;
  const double* w = g.t.v.W + mem * len;
  const double* c = g.t.v.c + mem * len;
  const int e0 = colptr[j], e1 = colptr[j + 1];
  const bool sums = chunk == 0 && wave == 0;
  double aw = 0, q = 0;
  for (int eb = e0; eb < e1; eb += 64) {
    // 64 rows of the column at a time: each lane fetches one row's entry, weight and extent
    const int e = eb + lane;
    int p0 = 0, p1 = 0;
    double wr = 0, wa = 0;
    if (e < e1) {
      const int r = crow[e];
      const double a = cval[e];
      wr = w[r];
      wa = wr * a;
      p0 = rowptr[r];
      p1 = rowptr[r + 1];
      if (sums) {
        aw = fma(a, wr, aw);
        q = fma(wa, wr * c[r], q);
      }
    }
    const int nb = min(64, e1 - eb);
    for (int i = 0; i < nb; i++) {
      const double wai = __shfl(wa, i), wri = __shfl(wr, i);
      const int s0 = __shfl(p0, i), s1 = __shfl(p1, i);
      for (int s = s0 + lane; s < s1; s += 64) {
        const int k = col[s];
        if (k >= lo && k < hi) sG[k - k0] = fma(wai, wri * val[s], sG[k - k0]);
      }
      WaveSync();  // (the next row may touch the same entries from other lanes)
    }
  }
  __syncthreads();
  double* G = ar.G + ar.g_off[id] + (size_t)j * m + k0;
  for (int k = threadIdx.x; k < cw; k += blockDim.x) G[k] = sG[k];
  if (sums) {
    aw = WaveSum(aw);
    q = WaveSum(q);
    if (lane == 0) {
      ar.AWc[ar.r_off[id] + j] = aw;
      ar.AQcc[ar.r_off[id] + j] = q;
    }
  }
}

// Row k of a member times NV vectors y_v (gathered through the clique's permutation): one fma chain per vector over
// the row's nonzeros in ascending column.
template <int NV>
__device__ __forceinline__ void LinSparseRowDots(const LinSparseGroup& g, size_t mem, int k, const int* __restrict__ perm,
                                                 const double* __restrict__ y0, const double* __restrict__ y1, double* acc) {
  const size_t base = (size_t)g.eptr[mem];
  const int* rowptr = g.rowptr + mem * ((size_t)g.t.v.len + 1);
  const int* col = g.col + base;
  const double* val = g.val + base;
  double a0 = 0, a1 = 0;
  const int s1 = rowptr[k + 1];
  for (int s = rowptr[k]; s < s1; s++) {
    const int v = perm[col[s]];
    const double a = val[s];
    a0 = fma(a, y0[v], a0);
    if (NV == 2) a1 = fma(a, y1[v], a1);
  }
  acc[0] = a0;
  if (NV == 2) acc[NV - 1] = a1;
}

// ---- PrepareStep (MODE 0) / eigenvalue query (MODE 1), phase 1: linear_tiled_slack<MODE> with the row's dot taken
// from its nonzeros (no y staging: no width limit).  The row operation and the tile's partials are that kernel's,
// line for line; phase 2 is linear_tiled_finish<MODE>.
template <int MODE>
__global__ void __launch_bounds__(kLinTiledBlock) linear_sparse_slack(LinSparseGroup g, StepArgs sa, int tiles) {
  sa.c_weight = CWeightOf(sa);  // (the barrier parameter may live on the device: cxk_select_mu_async)
  __shared__ double scratch[kLinTiledBlock / 64];
  const int len = g.t.v.len, tid = threadIdx.x;
  const size_t mem = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int k = tile * kLinTiledRowTile + tid;
  const int id = g.t.v.ids[mem];
  const bool live = k < len;
  double s = 0;
  if (live) LinSparseRowDots<1>(g, mem, k, sa.cl_perm + sa.cl_ptr[id], sa.y, nullptr, &s);
  const double* c = g.t.v.c + mem * len;
  double* w = g.t.v.W + mem * len;
  const double kc = (MODE == 0 && sa.affine) ? 0.0 : sa.c_weight;
  // rows past the end of the last tile: nothing to the sums, and nothing to min / max
  double mx = MODE == 0 ? 0.0 : -kLinTiledHuge, mn = kLinTiledHuge, s2 = 0, s1 = 0;
  if (live) {
    s -= c[k] * kc;
    if (MODE == 0) {
      if (sa.affine) {  // AffineUpdate: SW = minus_s .* W ; W += W .* SW
        const double sw = s * w[k];
        g.t.v.T1[mem * len + k] = sw;
        w[k] += w[k] * sw;
      } else {
        const double d = s * w[k] + sa.e_weight;
        g.t.v.T2[mem * len + k] = d;
        mx = fmax(0.0, fabs(d));  // (linear_prepare's fmax(mx, |d|) from 0)
        s2 = d * d;
      }
    } else {
      const double ws = w[k] * s;
      mx = ws;
      mn = ws;
      s2 = ws * ws;
      s1 = ws;
    }
  }
  if (MODE == 0 && sa.affine) return;  // (uniform: no barrier follows)
  mx = LinTiledBlockMax(mx, scratch);
  if (MODE == 1) mn = -LinTiledBlockMax(-mn, scratch);
  s2 = BlockSum(s2, scratch);
  if (MODE == 1) s1 = BlockSum(s1, scratch);
  if (tid == 0) {
    double* p = g.t.part + (mem * tiles + tile) * 4;
    if (MODE == 0) {
      p[0] = s2;
      p[1] = mx;
    } else {
      p[0] = mx;
      p[1] = mn;
      p[2] = s2;
      p[3] = s1;
    }
  }
}

// ---- line search: linear_tiled_line_search on the nonzeros; linear_tiled_line_finish reduces its partials.
__global__ void __launch_bounds__(kLinTiledBlock) linear_sparse_line_search(LinSparseGroup g, LineSearchArgs a, int tiles) {
  __shared__ double scratch[kLinTiledBlock / 64];
  const int len = g.t.v.len, tid = threadIdx.x;
  const size_t mem = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int k = tile * kLinTiledRowTile + tid;
  const int id = g.t.v.ids[mem];
  double t[2] = {0, 0};
  if (k < len) LinSparseRowDots<2>(g, mem, k, a.cl_perm + a.cl_ptr[id], a.y0, a.y1, t);
  double ub = kLinTiledHuge, lb = -kLinTiledHuge;
  if (k < len) {
    const double ck = g.t.v.c[mem * len + k], wk = g.t.v.W[mem * len + k];
    const double t0 = t[0] - ck * a.c0_weight;
    const double t1 = t[1] - ck * a.c1_weight;
    const double d0 = t0 * wk + 1, d1 = t1 * wk + 1;
    const double delta = d1 - d0;
    double ubi = (a.dinfmax - d0) / delta, lbi = (-a.dinfmax - d0) / delta;
    if (lbi > ubi) {
      const double x = ubi;
      ubi = lbi;
      lbi = x;
    }
    ub = fmin(ub, ubi);
    lb = fmax(lb, lbi);
  }
  lb = LinTiledBlockMax(lb, scratch);
  ub = -LinTiledBlockMax(-ub, scratch);
  if (tid == 0) {
    double* p = g.t.part + (mem * tiles + tile) * 4;
    p[0] = lb;
    p[1] = ub;
  }
}

}  // namespace cxk
