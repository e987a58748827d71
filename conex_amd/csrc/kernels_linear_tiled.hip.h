// Linear-inequality blocks on the tiled route (cxk_set_tiled_linear): the block's work is spread over the chip
// instead of sitting on the one workgroup of linear_schur / linear_prepare / linear_line_search
// (kernels_linear.hip.h; reference linear_constraint.cc:48-205).  The O(rows m) passes run on a grid of columns
// (assembly) or of row tiles (slack, line search), and the one dense contraction, G = WA^T WA with
// WA = diag(w) A, on the batched fp64 MFMA GEMM (gemm_mfma.hip).  linear_take_step and vec_set_identity are
// grid-wide already and serve both routes.
//
// No atomics, no workgroup waits for another: a kernel reads only what an earlier launch on the stream wrote.
// Every sum is a thread's fma chain followed by BlockSum, or a fixed-order pass over the per-tile partials
// (a thread's chain over its stride of tiles, then BlockSum), so its order depends on the shape only: same
// bits every run.  A row's slack is one fma chain over j = 0 .. m - 1, the order linear_prepare uses: per-row
// values agree with the LDS route's; the sums over rows are associated differently.
//
// Work space per group (LinTiledGroup): WA (rows x m per block), the GEMM's lower triangle Gf (m x m per block),
// four doubles per row tile.
#pragma once
#include "kernels_linear.hip.h"  // (the split rule of the Gram product is the streamed cones': SocStreamSplits, cone_types.h)

namespace cxk {

constexpr int kLinTiledBlock = 256;    // threads of every kernel here
constexpr int kLinTiledRowTile = 256;  // rows of the slack one workgroup forms (one per thread)
constexpr int kLinTiledYChunk = 2048;  // entries of y staged in LDS at a time (16 KB per vector)
constexpr double kLinTiledHuge = 1.7976931348623157e308;

struct LinTiledGroup {
  VecGroup v;    // len = rows, m, count, A, c, W, T1, T2, ids as the LDS route's kernels read them
  double* WA;    // count x (rows x m)       diag(w) a_i, column by column
  double* Gf;    // count x (m x m)          WA^T WA, lower triangle (the GEMM's output)
  double* part;  // count x tiles x 4        per-tile partials of the slack kernels
};

// Block-wide maximum in a fixed order (BlockSum's shape).  `scratch` holds >= blockDim / 64 doubles.
__device__ __forceinline__ double LinTiledBlockMax(double v, double* scratch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = WaveMax(v);
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  double t = scratch[0];
  for (int w = 1; w < kLinTiledBlock / 64; w++) t = fmax(t, scratch[w]);
  return t;
}

// ---- Schur complement, stage 1: the block's two scalars.  One workgroup per block.
__global__ void __launch_bounds__(kLinTiledBlock) linear_tiled_scalars(LinTiledGroup g, Arena ar) {
  __shared__ double scratch[kLinTiledBlock / 64];
  const int len = g.v.len, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const int id = g.v.ids[mem];
  const double* c = g.v.c + mem * len;
  const double* w = g.v.W + mem * len;
  double s1 = 0, s2 = 0;
  for (int k = tid; k < len; k += kLinTiledBlock) {
    const double wc = w[k] * c[k];
    s1 += wc;
    s2 = fma(wc, wc, s2);
  }
  s1 = BlockSum(s1, scratch);
  s2 = BlockSum(s2, scratch);
  if (tid == 0) {
    ar.sc[2 * id] = s1;
    ar.sc[2 * id + 1] = s2;
  }
}

// ---- stage 2: one workgroup per column a_i of a block, striding down the column (coalesced):
// WA_i = w o a_i to the work space, AW_i = sum a_ki w_k, AQc_i = sum (w_k a_ki)(w_k c_k).
__global__ void __launch_bounds__(kLinTiledBlock) linear_tiled_apply(LinTiledGroup g, Arena ar) {
  __shared__ double scratch[kLinTiledBlock / 64];
  const int len = g.v.len, m = g.v.m, tid = threadIdx.x;
  const size_t mem = blockIdx.x / m;
  const int i = (int)(blockIdx.x % m);
  const int id = g.v.ids[mem];
  const double* a = g.v.A + (mem * m + i) * len;
  const double* c = g.v.c + mem * len;
  const double* w = g.v.W + mem * len;
  double* WA = g.WA + (mem * m + i) * len;
  double aw = 0, q = 0;
  for (int k = tid; k < len; k += kLinTiledBlock) {
    const double wk = w[k], ak = a[k];
    const double wa = wk * ak;
    WA[k] = wa;
    aw = fma(ak, wk, aw);
    q = fma(wa, wk * c[k], q);
  }
  aw = BlockSum(aw, scratch);
  q = BlockSum(q, scratch);
  if (tid == 0) {
    ar.AWc[ar.r_off[id] + i] = aw;
    ar.AQcc[ar.r_off[id] + i] = q;
  }
}

// ---- stage 3 is the GEMM (LaunchLinearTiledSchur); this copies its lower triangle to the full square
// linear_schur writes.
__global__ void __launch_bounds__(kLinTiledBlock) linear_tiled_mirror(LinTiledGroup g, Arena ar) {
  const int m = g.v.m;
  const size_t mm = (size_t)m * m, total = mm * g.v.count;
  for (size_t e = blockIdx.x * (size_t)kLinTiledBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kLinTiledBlock) {
    const size_t mem = e / mm;
    const int idx = (int)(e % mm), i = idx % m, j = idx / m;
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    ar.G[ar.g_off[g.v.ids[mem]] + idx] = g.Gf[mem * mm + hi + (size_t)lo * m];
  }
}

// Row k of A times NV vectors y_v (gathered through the clique's permutation), by the whole workgroup: y is
// staged in LDS a chunk at a time, every thread runs one fma chain per vector over j = 0 .. m - 1 across the
// chunks.  Every thread of the workgroup calls this (barriers inside); threads with k >= len stage and idle.
template <int NV>
__device__ __forceinline__ void LinTiledRowDots(const double* __restrict__ A, int len, int m, int k,
                                                const int* __restrict__ perm, const double* __restrict__ y0,
                                                const double* __restrict__ y1, double (*sy)[kLinTiledYChunk],
                                                double* acc) {
  const int tid = threadIdx.x;
  double a0 = 0, a1 = 0;
  for (int j0 = 0; j0 < m; j0 += kLinTiledYChunk) {
    const int jn = min(kLinTiledYChunk, m - j0);
    __syncthreads();  // the previous chunk has been read
    for (int q = tid; q < jn; q += kLinTiledBlock) {
      const int v = perm[j0 + q];
      sy[0][q] = y0[v];
      if (NV == 2) sy[NV - 1][q] = y1[v];
    }
    __syncthreads();
    if (k < len) {
      const double* col = A + k + (size_t)j0 * len;
#pragma unroll 4
      for (int j = 0; j < jn; j++) {
        const double a = col[(size_t)j * len];
        a0 = fma(a, sy[0][j], a0);
        if (NV == 2) a1 = fma(a, sy[NV - 1][j], a1);
      }
    }
  }
  acc[0] = a0;
  if (NV == 2) acc[NV - 1] = a1;
}

// ---- PrepareStep (MODE 0) / eigenvalue query (MODE 1), phase 1: a grid of block x row tiles, one row per
// thread: the slack, then linear_prepare's row operation.  The affine update (MODE 0, sa.affine) ends here;
// otherwise every tile leaves its partials: MODE 0 {sum d^2, max |d|}, MODE 1 {max ws, min ws, sum ws^2, sum ws}.
template <int MODE>
__global__ void __launch_bounds__(kLinTiledBlock) linear_tiled_slack(LinTiledGroup g, StepArgs sa, int tiles) {
  sa.c_weight = CWeightOf(sa);  // (the barrier parameter may live on the device: cxk_select_mu_async)
  __shared__ double sy[1][kLinTiledYChunk];
  __shared__ double scratch[kLinTiledBlock / 64];
  const int len = g.v.len, m = g.v.m, tid = threadIdx.x;
  const size_t mem = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int k = tile * kLinTiledRowTile + tid;
  const int id = g.v.ids[mem];
  const bool live = k < len;
  double s = 0;
  LinTiledRowDots<1>(g.v.A + mem * len * m, len, m, k, sa.cl_perm + sa.cl_ptr[id], sa.y, nullptr, sy, &s);
  const double* c = g.v.c + mem * len;
  double* w = g.v.W + mem * len;
  const double kc = (MODE == 0 && sa.affine) ? 0.0 : sa.c_weight;
  // rows past the end of the last tile: nothing to the sums, and nothing to min / max
  double mx = MODE == 0 ? 0.0 : -kLinTiledHuge, mn = kLinTiledHuge, s2 = 0, s1 = 0;
  if (live) {
    s -= c[k] * kc;
    if (MODE == 0) {
      if (sa.affine) {  // AffineUpdate: SW = minus_s .* W ; W += W .* SW
        const double sw = s * w[k];
        g.v.T1[mem * len + k] = sw;
        w[k] += w[k] * sw;
      } else {
        const double d = s * w[k] + sa.e_weight;
        g.v.T2[mem * len + k] = d;
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
    double* p = g.part + (mem * tiles + tile) * 4;
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

// ---- phase 2: one workgroup per block reduces the tile partials in a fixed order (a thread's stride of
// tiles in tile order, then the block) and writes what linear_prepare writes, signs included.
template <int MODE>
__global__ void __launch_bounds__(kLinTiledBlock) linear_tiled_finish(LinTiledGroup g, StepArgs sa, int tiles) {
  __shared__ double scratch[kLinTiledBlock / 64];
  const int tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const int id = g.v.ids[mem];
  const double* part = g.part + mem * tiles * 4;
  double mx = MODE == 0 ? 0.0 : -kLinTiledHuge, mn = kLinTiledHuge, s2 = 0, s1 = 0;
  for (int t = tid; t < tiles; t += kLinTiledBlock) {
    const double* p = part + (size_t)t * 4;
    if (MODE == 0) {
      s2 += p[0];
      mx = fmax(mx, p[1]);
    } else {
      mx = fmax(mx, p[0]);
      mn = fmin(mn, p[1]);
      s2 += p[2];
      s1 += p[3];
    }
  }
  mx = LinTiledBlockMax(mx, scratch);
  if (MODE == 1) mn = -LinTiledBlockMax(-mn, scratch);
  s2 = BlockSum(s2, scratch);
  if (MODE == 1) s1 = BlockSum(s1, scratch);
  if (tid == 0) {
    if (MODE == 0) {
      sa.info[2 * id] = s2;
      sa.info[2 * id + 1] = mx;
    } else {
      sa.info[4 * id] = -mx;
      sa.info[4 * id + 1] = -mn;
      sa.info[4 * id + 2] = s2;
      sa.info[4 * id + 3] = -s1;
    }
  }
}

// ---- line search: linear_line_search's per-row interval on the slack kernel's tiling; per tile
// {max lower end, min upper end}.
__global__ void __launch_bounds__(kLinTiledBlock) linear_tiled_line_search(LinTiledGroup g, LineSearchArgs a, int tiles) {
  __shared__ double sy[2][kLinTiledYChunk];
  __shared__ double scratch[kLinTiledBlock / 64];
  const int len = g.v.len, m = g.v.m, tid = threadIdx.x;
  const size_t mem = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int k = tile * kLinTiledRowTile + tid;
  const int id = g.v.ids[mem];
  double t[2] = {0, 0};
  LinTiledRowDots<2>(g.v.A + mem * len * m, len, m, k, a.cl_perm + a.cl_ptr[id], a.y0, a.y1, sy, t);
  double ub = kLinTiledHuge, lb = -kLinTiledHuge;
  if (k < len) {
    const double ck = g.v.c[mem * len + k], wk = g.v.W[mem * len + k];
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
    double* p = g.part + (mem * tiles + tile) * 4;
    p[0] = lb;
    p[1] = ub;
  }
}

__global__ void __launch_bounds__(kLinTiledBlock) linear_tiled_line_finish(LinTiledGroup g, LineSearchArgs a, int tiles) {
  __shared__ double scratch[kLinTiledBlock / 64];
  const int tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const int id = g.v.ids[mem];
  const double* part = g.part + mem * tiles * 4;
  double ub = kLinTiledHuge, lb = -kLinTiledHuge;
  for (int t = tid; t < tiles; t += kLinTiledBlock) {
    lb = fmax(lb, part[(size_t)t * 4]);
    ub = fmin(ub, part[(size_t)t * 4 + 1]);
  }
  lb = LinTiledBlockMax(lb, scratch);
  ub = -LinTiledBlockMax(-ub, scratch);
  if (tid == 0) {
    a.out[2 * id] = lb;
    a.out[2 * id + 1] = ub;
  }
}

}  // namespace cxk
