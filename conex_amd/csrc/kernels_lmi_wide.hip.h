// The two-sided Lanczos run of the large-order LMI route spread over the chip (cxk_set_wide_spectrum): the same
// recurrence and the same outputs as lmi_large_spectrum<MODE> (kernels_lmi_large.hip.h), which keeps seven vectors in
// the LDS of ONE workgroup and so ends at LmiLargeSpectrumMaxOrder().  Here every vector lives in a per-constraint
// work space in HBM, and a run is a sequence of ordinary launches on the context's stream:
//   lmi_wide_traces   64 x 64 tiles of WS: partials of tr(WS WS), tr(WS) and the arg-max of the diagonal
//   lmi_wide_start    the start column (or the HcRandom vector of a Hermitian cone), the run's state words
//   lmi_wide_pass     one pass over a matrix: tile (tr, tc) adds row partials to M x0 and column partials to M' x1
//   lmi_wide_reduce   (orders from kWideReduceMinOrder on) 256 entries per workgroup: sums the partials in tile order
//                     into the two product vectors, and this slice's share of the two inner products they enter
//   lmi_wide_step     per constraint: sums the partials in tile order (or adds the slices' shares), forms alpha and
//                     beta, updates the vectors and sets the "broken" word -- every later launch of the run reads it
//                     and returns at once
//   lmi_wide_finish   TridiagMinMaxWave on alpha / beta, the traces, ClampToSpectrumBound, sa.info
// No atomics and no wait between workgroups: every sum has one fixed order, two runs give the same bits.
#pragma once
#include <climits>
#include <cmath>

#include "kernels_lmi.hip.h"

namespace cxk {

constexpr int kWideTile = 64;     // the matrix tile (rows and columns)
constexpr int kWideTileLd = 65;   // its leading dimension in LDS
constexpr int kWideStepBlock = 1024;
constexpr int kWideReduceBlock = 256;  // entries of the product vectors per workgroup of lmi_wide_reduce
// From this order on the partials are summed by lmi_wide_reduce, a launch of its own over n / 256 workgroups; below,
// by the one workgroup of lmi_wide_step.  Measured (full runs of n / 2 steps): the third launch costs
// 0.4 / 1.1 / 2.6 ms at n = 256 / 512 / 1000, is even at 2000, and saves 28 of 74 ms at 2549, 112 of 225 ms at 4000,
// where one CU reads 2 n^2 / 64 doubles of partials per step.  CXK_WIDE_REDUCE_MIN_ORDER moves it (tests).
constexpr int kWideReduceMinOrder = 2049;

inline __host__ __device__ int LmiWideIters(int n, int herm_d) { return herm_d ? (n / herm_d) / 2 + 1 : n / 2; }
inline __host__ __device__ int LmiWideTiles(int n) { return (n + kWideTile - 1) / kWideTile; }
inline __host__ __device__ int LmiWideSlices(int n) { return (n + kWideReduceBlock - 1) / kWideReduceBlock; }
// doubles of one constraint's work space: state words, alpha, beta, six vectors, the partials of the two products by
// tile row / tile column, the partials of tr(WS WS) by tile, of tr(WS) and the diagonal's arg-max by diagonal tile,
// two inner-product shares per slice of lmi_wide_reduce
inline __host__ __device__ size_t LmiWideDoubles(int n, int herm_d) {
  const size_t nt = LmiWideTiles(n), it1 = (size_t)LmiWideIters(n, herm_d) + 1;
  return 16 + 2 * it1 + 6 * (size_t)n + 2 * nt * n + nt * nt + 3 * nt + 2 * (size_t)LmiWideSlices(n);
}

// state words
enum { kWideBroken = 0, kWideCount = 1, kWideBetaPrev = 2, kWideScaling = 3 };

struct LmiWideView {
  double *st, *alpha, *beta, *V0, *V1, *U0, *U1, *P0, *P1, *part0, *part1, *t2p, *t1p, *dgv, *dgi, *dp;
};
inline __host__ __device__ LmiWideView LmiWideViewOf(double* base, int n, int herm_d) {
  const size_t nt = LmiWideTiles(n), it1 = (size_t)LmiWideIters(n, herm_d) + 1;
  LmiWideView v;
  v.st = base;
  v.alpha = v.st + 16;
  v.beta = v.alpha + it1;
  v.V0 = v.beta + it1;
  v.V1 = v.V0 + n;
  v.U0 = v.V1 + n;
  v.U1 = v.U0 + n;
  v.P0 = v.U1 + n;
  v.P1 = v.P0 + n;
  v.part0 = v.P1 + n;
  v.part1 = v.part0 + nt * n;
  v.t2p = v.part1 + nt * n;
  v.t1p = v.t2p + nt * nt;
  v.dgv = v.t1p + nt;
  v.dgi = v.dgv + nt;
  v.dp = v.dgi + nt;
  return v;
}

// grid (tiles^2, constraints).  Tile (tr, tc) holds sum M[r, c] M[c, r] over its entries; a diagonal tile also the
// sum of its diagonal and that diagonal's first largest entry (lmi_large_spectrum: `>` in ascending order).
__global__ void __launch_bounds__(256) lmi_wide_traces(int n, int herm_d, const double* __restrict__ WS_all,
                                                       double* __restrict__ wide, size_t per) {
  __shared__ double B[kWideTile * kWideTileLd];  // tile (tc, tr): read transposed
  __shared__ double red[4];
  const int nt = LmiWideTiles(n), tr = blockIdx.x % nt, tc = blockIdx.x / nt;
  const double* M = WS_all + (size_t)blockIdx.y * n * n;
  const LmiWideView v = LmiWideViewOf(wide + (size_t)blockIdx.y * per, n, herm_d);
  const int tid = threadIdx.x, lr = tid & 63, lc0 = tid >> 6;
  double a[16];  // this thread's entries of tile (tr, tc)
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int lc = lc0 + 4 * k;
    const int ra = tr * kWideTile + lr, ca = tc * kWideTile + lc;
    a[k] = (ra < n && ca < n) ? M[ra + (size_t)ca * n] : 0.0;
    const int rb = tc * kWideTile + lr, cb = tr * kWideTile + lc;
    B[lr + lc * kWideTileLd] = (rb < n && cb < n) ? M[rb + (size_t)cb * n] : 0.0;
  }
  __syncthreads();
  double s = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) s = fma(a[k], B[lc0 + 4 * k + lr * kWideTileLd], s);
  s = BlockSum(s, red);
  if (tid == 0) v.t2p[blockIdx.x] = s;
  if (tr == tc && tid < 64) {
    const int row = tr * kWideTile + tid;
    const bool has = row < n;
    const double d = has ? M[row + (size_t)row * n] : 0.0;
    const double t1 = WaveSum(d);
    double best = (has && d == d) ? d : -INFINITY;
    int bi = has ? row : INT_MAX;
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > best || (ov == best && oi < bi)) {
        best = ov;
        bi = oi;
      }
    }
    if (tid == 0) {
      v.t1p[tr] = t1;
      v.dgv[tr] = best;
      v.dgi[tr] = (double)bi;
    }
  }
}

// grid = constraints.  V1 = r (mode 0: the column of WS with the largest diagonal entry, mode 1: that column of S;
// Hermitian cones: HcRandom), the state words of a fresh run.  The pass over W that follows forms W r.
template <int MODE>
__global__ void __launch_bounds__(kWideStepBlock)
lmi_wide_start(LmiGroup g, StepArgs sa, const double* __restrict__ WS_all, const double* __restrict__ S_all,
               double* __restrict__ wide, size_t per) {
  __shared__ int s_index;
  const int n = g.n, mem = blockIdx.x, id = g.ids[mem], tid = threadIdx.x;
  const LmiWideView v = LmiWideViewOf(wide + (size_t)mem * per, n, g.herm_d);
  const bool herm = g.herm_d != 0;
  if (tid == 0) {
    const int nt = LmiWideTiles(n);
    int t = 0;
    for (int q = 1; q < nt; q++)
      if (v.dgv[q] > v.dgv[t]) t = q;
    s_index = (int)v.dgi[t];
    v.st[kWideBroken] = 0.0;
    v.st[kWideCount] = 0.0;
    v.st[kWideBetaPrev] = 0.0;
    v.st[kWideScaling] = 0.0;
  }
  __syncthreads();
  const double* r = (MODE == 0 ? WS_all : S_all) + (size_t)mem * n * n + (size_t)s_index * n;
  for (int i = tid; i < n; i += blockDim.x) v.V1[i] = herm ? HcRandom(id, sa.call, i) : r[i];
}

// grid (tiles^2, constraints), 256 threads.  start: the pass over W with x0 = x1 = r (only M x0 is used).
__global__ void __launch_bounds__(256) lmi_wide_pass(int n, int herm_d, const double* __restrict__ M_all,
                                                     double* __restrict__ wide, size_t per, int start) {
  __shared__ double T[kWideTile * kWideTileLd];
  __shared__ double xs0[kWideTile], xs1[kWideTile], red[4][kWideTile];
  const LmiWideView v = LmiWideViewOf(wide + (size_t)blockIdx.y * per, n, herm_d);
  if (!start && v.st[kWideBroken] != 0.0) return;  // (uniform over the grid: the run has ended)
  const int nt = LmiWideTiles(n), tr = blockIdx.x % nt, tc = blockIdx.x / nt;
  const double* M = M_all + (size_t)blockIdx.y * n * n;
  const int tid = threadIdx.x, lr = tid & 63, w = tid >> 6;
  const int r0 = tr * kWideTile, c0 = tc * kWideTile;
  double ld[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int ra = r0 + lr, ca = c0 + w + 4 * k;
    ld[k] = (ra < n && ca < n) ? M[ra + (size_t)ca * n] : 0.0;
  }
  if (tid < 64)
    xs0[tid] = c0 + tid < n ? (start ? v.V1 : v.V0)[c0 + tid] : 0.0;
  else if (tid < 128)
    xs1[tid - 64] = r0 + tid - 64 < n ? v.V1[r0 + tid - 64] : 0.0;
#pragma unroll
  for (int k = 0; k < 16; k++) T[lr + (w + 4 * k) * kWideTileLd] = ld[k];
  __syncthreads();
  double s = 0;
  if (w < 2) {  // row lr, columns of half w
    for (int c = 32 * w; c < 32 * w + 32; c++) s = fma(T[lr + c * kWideTileLd], xs0[c], s);
  } else {  // column lr, rows of half w - 2
    for (int r = 32 * (w - 2); r < 32 * (w - 2) + 32; r++) s = fma(T[r + lr * kWideTileLd], xs1[r], s);
  }
  red[w][lr] = s;
  __syncthreads();
  if (tid < 64) {
    if (r0 + tid < n) v.part0[(size_t)tc * n + r0 + tid] = red[0][tid] + red[1][tid];
  } else if (tid < 128) {
    const int t = tid - 64;
    if (c0 + t < n) v.part1[(size_t)tr * n + c0 + t] = red[2][t] + red[3][t];
  }
}

// grid (slices, constraints).  Entry i of the two products from their partials, tile by tile in ascending order, and
// this slice's share of the inner products the step needs: start (the pass over W): V0 = W r and V0 . V1; else
// U0 = WS V0, U1 = WS' V1, V0 . U1 (alpha) and U0 . U1 (the Hermitian run's scaling at step 0).
__global__ void __launch_bounds__(kWideReduceBlock) lmi_wide_reduce(int n, int herm_d, double* __restrict__ wide, size_t per,
                                                                    int start) {
  __shared__ double red[4];
  const LmiWideView v = LmiWideViewOf(wide + (size_t)blockIdx.y * per, n, herm_d);
  if (!start && v.st[kWideBroken] != 0.0) return;
  const int nt = LmiWideTiles(n), i = blockIdx.x * kWideReduceBlock + threadIdx.x;
  double d1 = 0, d2 = 0;
  if (i < n) {
    double u0 = 0, u1 = 0;
    if (start) {
      for (int t = 0; t < nt; t++) u0 += v.part0[(size_t)t * n + i];
      v.V0[i] = u0;
      d1 = u0 * v.V1[i];
    } else {
      for (int t = 0; t < nt; t++) {  // (both loads of a tile in flight together)
        u0 += v.part0[(size_t)t * n + i];
        u1 += v.part1[(size_t)t * n + i];
      }
      v.U0[i] = u0;
      v.U1[i] = u1;
      d1 = v.V0[i] * u1;
      d2 = u0 * u1;
    }
  }
  d1 = BlockSum(d1, red);
  d2 = BlockSum(d2, red);
  if (threadIdx.x == 0) {
    v.dp[2 * blockIdx.x] = d1;
    v.dp[2 * blockIdx.x + 1] = d2;
  }
}

// grid = constraints.  j = -1: both start vectors normalised.  j >= 0: the tail of Lanczos step j (alpha_j, the
// three-term update) and the head of step j + 1 (beta_j, the break test, the next vectors).  reduced: lmi_wide_reduce
// ran in front; else this kernel sums the partials itself (the same sums in the same order, the inner products as
// one fma chain per thread).  Thread t owns entries t, t + blockDim, ..: it re-reads only what it wrote.
__global__ void __launch_bounds__(kWideStepBlock) lmi_wide_step(int n, int herm_d, double* __restrict__ wide, size_t per,
                                                                int j, int reduced) {
  __shared__ double red[16];
  const LmiWideView v = LmiWideViewOf(wide + (size_t)blockIdx.x * per, n, herm_d);
  if (j >= 0 && v.st[kWideBroken] != 0.0) return;
  const bool herm = herm_d != 0;
  const int ns = LmiWideSlices(n), iters = LmiWideIters(n, herm_d), tid = threadIdx.x;
  const double beta_prev = v.st[kWideBetaPrev];
  double scaling = v.st[kWideScaling];
  double d1 = 0, d2 = 0;
  if (reduced) {
    for (int q = tid; q < ns; q += blockDim.x) {
      d1 += v.dp[2 * q];
      d2 += v.dp[2 * q + 1];
    }
  } else {
    const int nt = LmiWideTiles(n);
    if (j < 0) {
      for (int i = tid; i < n; i += blockDim.x) {
        double u0 = 0;
        for (int t = 0; t < nt; t++) u0 += v.part0[(size_t)t * n + i];
        v.V0[i] = u0;
        d1 = fma(u0, v.V1[i], d1);
      }
    } else {
      for (int i = tid; i < n; i += blockDim.x) {
        double u0 = 0, u1 = 0;
        for (int t = 0; t < nt; t++) {  // (both loads of a tile in flight together)
          u0 += v.part0[(size_t)t * n + i];
          u1 += v.part1[(size_t)t * n + i];
        }
        v.U0[i] = u0;
        v.U1[i] = u1;
        d1 = fma(v.V0[i], u1, d1);
        d2 = fma(u0, u1, d2);
      }
    }
  }
  d1 = BlockSum(d1, red);
  if (j < 0) {
    const double nrm = sqrt(d1);
    const double inrm = 1.0 / nrm;
    for (int i = tid; i < n; i += blockDim.x) {
      const double a = herm ? v.V0[i] * inrm : v.V0[i] / nrm, b = herm ? v.V1[i] * inrm : v.V1[i] / nrm;
      v.V0[i] = a;
      v.V1[i] = b;
      v.P0[i] = a;
      v.P1[i] = b;
    }
    return;
  }
  if (j == 0 && herm) {
    scaling = BlockSum(d2, red);
    if (tid == 0) v.st[kWideScaling] = scaling;
  }
  const double a = d1;
  if (tid == 0) v.alpha[j] = a;
  double b2 = 0;
  for (int i = tid; i < n; i += blockDim.x) {
    double u0 = v.U0[i] - a * v.V0[i], u1 = v.U1[i] - a * v.V1[i];
    if (j > 0) {
      u0 -= beta_prev * v.P0[i];
      u1 -= beta_prev * v.P1[i];
    }
    v.U0[i] = u0;
    v.U1[i] = u1;
    b2 = fma(u0, u1, b2);
  }
  if (j + 1 >= iters) return;
  b2 = BlockSum(b2, red);
  if (herm ? (b2 < 1e-5 * scaling) : (b2 < 1e-6)) {
    if (tid == 0) v.st[kWideBroken] = 1.0;
    return;
  }
  const double bp = sqrt(b2), ib = 1.0 / bp;
  if (tid == 0) {
    v.beta[j] = bp;
    v.st[kWideBetaPrev] = bp;
    v.st[kWideCount] = (double)(j + 1);
  }
  for (int i = tid; i < n; i += blockDim.x) {
    v.P0[i] = v.V0[i];
    v.P1[i] = v.V1[i];
    v.V0[i] = herm ? v.U0[i] * ib : v.U0[i] / bp;
    v.V1[i] = herm ? v.U1[i] * ib : v.U1[i] / bp;
  }
}

// grid = constraints.  The outputs of lmi_large_spectrum<MODE> from alpha, beta (HBM) and the trace partials.
template <int MODE>
__global__ void __launch_bounds__(256) lmi_wide_finish(LmiGroup g, StepArgs sa, double* __restrict__ wide, size_t per) {
  __shared__ double red[4], ext[2];
  const int n = g.n, mem = blockIdx.x, id = g.ids[mem], tid = threadIdx.x;
  const LmiWideView v = LmiWideViewOf(wide + (size_t)mem * per, n, g.herm_d);
  const bool herm = g.herm_d != 0;
  const int nt = LmiWideTiles(n), cnt = (int)v.st[kWideCount];
  if (tid < 64) TridiagMinMaxWave(cnt + 1, v.alpha, v.beta, &ext[0], &ext[1]);
  double t2 = 0, t1 = 0;
  for (int q = tid; q < nt * nt; q += blockDim.x) t2 += v.t2p[q];
  for (int q = tid; q < nt; q += blockDim.x) t1 += v.t1p[q];
  t2 = BlockSum(t2, red);
  t1 = BlockSum(t1, red);
  if (tid == 0) {
    double mn = ext[0], mx = ext[1];
    if (!sa.no_clamp) ClampToSpectrumBound(n, t1, t2, &mn, &mx);
    if (g.herm_d > 1) {
      t2 /= g.herm_d;
      t1 /= g.herm_d;
    }
    const int rank = herm ? n / g.herm_d : n;
    if (MODE == 0) {
      const double l1 = fabs(sa.e_weight + mn), l2 = fabs(sa.e_weight + mx);
      sa.info[2 * id] = t2 + 2 * t1 + rank;
      sa.info[2 * id + 1] = l1 < l2 ? l2 : l1;
    } else {
      sa.info[4 * id] = -mx;
      sa.info[4 * id + 1] = -mn;
      sa.info[4 * id + 2] = t2;
      sa.info[4 * id + 3] = -t1;
    }
  }
}

// The whole run, enqueued on `st`; nobody waits.  A run that breaks at step j still pays its remaining launches,
// each of which reads one word and returns.  reduce: lmi_wide_reduce between every pass and step.
inline hipError_t LmiWideSpectrum(const LmiGroup& g, const StepArgs& sa, const double* WS, const double* S, double* wide,
                                  bool reduce, int mode, hipStream_t st) {
  const int n = g.n, nt = LmiWideTiles(n), iters = LmiWideIters(n, g.herm_d);
  const size_t per = LmiWideDoubles(n, g.herm_d);
  const dim3 tiles(nt * nt, g.count);
  lmi_wide_traces<<<tiles, 256, 0, st>>>(n, g.herm_d, WS, wide, per);
  if (mode == 0)
    lmi_wide_start<0><<<g.count, kWideStepBlock, 0, st>>>(g, sa, WS, S, wide, per);
  else
    lmi_wide_start<1><<<g.count, kWideStepBlock, 0, st>>>(g, sa, WS, S, wide, per);
  const dim3 slices(LmiWideSlices(n), g.count);
  lmi_wide_pass<<<tiles, 256, 0, st>>>(n, g.herm_d, g.W, wide, per, 1);
  if (reduce) lmi_wide_reduce<<<slices, kWideReduceBlock, 0, st>>>(n, g.herm_d, wide, per, 1);
  lmi_wide_step<<<g.count, kWideStepBlock, 0, st>>>(n, g.herm_d, wide, per, -1, reduce);
  for (int j = 0; j < iters; j++) {
    lmi_wide_pass<<<tiles, 256, 0, st>>>(n, g.herm_d, WS, wide, per, 0);
    if (reduce) lmi_wide_reduce<<<slices, kWideReduceBlock, 0, st>>>(n, g.herm_d, wide, per, 0);
    lmi_wide_step<<<g.count, kWideStepBlock, 0, st>>>(n, g.herm_d, wide, per, j, reduce);
  }
  if (mode == 0)
    lmi_wide_finish<0><<<g.count, 256, 0, st>>>(g, sa, wide, per);
  else
    lmi_wide_finish<1><<<g.count, 256, 0, st>>>(g, sa, wide, per);
  return hipGetLastError();
}

}  // namespace cxk
