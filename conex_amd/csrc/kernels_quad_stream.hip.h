// Quadratic cones { (x0, x1) : x0 >= sqrt(x1' Q x1) } held in HBM (cxk_set_streamed_quadratic): the cone and
// its inner-product matrix Q stay in HBM and every stage is a few launches ordered by the stream alone.
// Semantics are those of quad_schur / quad_prepare / quad_take_step (kernels_quad.hip.h; reference
// quadratic_cone_constraint.cc:14-297); what differs is who does the work: the products with Q run on a grid of
// cone x row tiles x column splits (quad_stream_qmv, up to two vectors in ONE pass over Q), the O(n) maps on one
// 256-thread workgroup per cone that strides over the cone, the O(n m) pass of the Schur complement on one
// workgroup per column, the O(m^2) block on a grid of 256 entries per workgroup.
//
// No atomics, no workgroup waits for another: a kernel reads only what an earlier launch on the stream wrote.
// Every sum is a thread's fma chain over its stride followed by BlockSum (fixed butterfly, then the waves in
// order); a product with Q is a thread's fma chain over its columns per split, the splits added in split order
// by the reader (QuadStreamQx).  All orders depend on the shape and the launch shape only: same bits every run.
// Q is multiplied as given (no use of symmetry), column-major, indexed in 64 bits.
//
// Constant per cone, made once at cxk_finalize: Qc1 = Q c1, c1' Q c1, A_gram = A1' Q A1 (two batched GEMMs).
// Work space per cone (QuadStreamGroup): the split partials of up to two products, Q w1, v and A1' Qc1 (m each),
// the slack, d1, Q d1, eight scalars.
//
// Passes over Q: assembly 1 (Q w1); PrepareStep and the eigenvalue query 2 (Q [w1, ms1] in one pass, Q d1);
// TakeStep 0: Q(step f d1) = step f (Q d1), and Q d1 is what PrepareStep's second pass left behind.
#pragma once
#include "kernels_quad.hip.h"

namespace cxk {

constexpr int kQuadStreamBlock = 256;      // threads of every kernel here
constexpr int kQuadStreamRowTile = 256;    // rows of Q one workgroup of quad_stream_qmv forms (one per thread)
constexpr int kQuadStreamXChunk = 64;      // entries of each x staged in LDS at a time
constexpr int kQuadStreamMinSplit = 64;    // Q's columns are split only into pieces at least this long

// How a group's inner-product matrix is held: what a pass out_r = Q x_r launches and whether QuadStreamQx has partials to read.
enum QuadQForm { kQuadQIdentity = 0, kQuadQDense = 1, kQuadQStructured = 2 };

struct QuadStreamGroup {
  int n, m, count, splits;
  int q_form;           // QuadQForm; kQuadQStructured: Q = S + F diag(sigma) F' (kernels_quad_structured.hip.h), splits = 1
  const double* A;      // count x (n + 1) x m; nullptr where A is held by its nonzeros (kernels_quad_sparse.hip.h)
  const double* c;      // count x (n + 1)
  const double* Q;      // count x n x n; nullptr unless q_form is kQuadQDense
  const double* Agram;  // count x m x m
  double* W;            // count x (n + 1)
  double* D;            // count x (n + 1)
  double* S;            // count x (n + 1): wsqrt_q1 (n), wsqrt_q1_norm_sqr
  const int* ids;
  double* part;         // count x splits x 2 x n   split partials of Q x_0, Q x_1 (unused without Q)
  double* qc1;          // count x n                Q c1 (constant)
  double* cqc;          // count                    c1' Q c1 (constant)
  double* qw;           // count x n                Q w1 of the last assembly
  double* v;            // count x m                A1' Q w1 + A0 W0
  double* u;            // count x m                A1' Q c1 (of every assembly; constant, made once, with a sparse A)
  double* ms;           // count x (n + 1)          minus the slack
  double* dv;           // count x n                d1 of PrepareStep / the query
  double* qd;           // count x n                Q d1 as PrepareStep left it (TakeStep reads it)
  double* scal;         // count x 8                det w, scale, <c1, Q w1>, -, d0, d1' Q d1, -, -
};

// Column splits of a product with Q for `count` cones of order n: enough workgroups to fill the chip, none
// shorter than kQuadStreamMinSplit columns.
__host__ __device__ inline int QuadStreamSplits(int n, long long count) {
  const long long tiles = (long long)((n + kQuadStreamRowTile - 1) / kQuadStreamRowTile) * (count > 0 ? count : 1);
  const long long by_len = n / kQuadStreamMinSplit;
  const long long by_fill = (512 + tiles - 1) / tiles;
  const long long s = by_len < by_fill ? by_len : by_fill;
  return s < 1 ? 1 : (int)s;
}

// The vectors one pass multiplies: x_r of cone `mem` starts at p[r] + mem * stride[r].
struct QuadStreamVecs {
  const double* p[2];
  size_t stride[2];
};

// ---- out_r = Q x_r for R vectors in one pass over Q.  Workgroup (cone, row tile, split): one row per thread,
// coalesced across the tile; the split's columns in chunks of kQuadStreamXChunk, the x chunk staged in LDS.
template <int R>
__global__ void __launch_bounds__(kQuadStreamBlock) quad_stream_qmv(QuadStreamGroup g, QuadStreamVecs x, int tiles) {
  __shared__ double sx[R][kQuadStreamXChunk];
  const int n = g.n, splits = g.splits, tid = threadIdx.x;
  const int s = (int)(blockIdx.x % splits);
  const size_t t = blockIdx.x / splits;
  const int i = (int)(t % tiles) * kQuadStreamRowTile + tid;
  const size_t mem = t / tiles;
  const int per = (n + splits - 1) / splits;
  const int j0 = min(n, s * per), j1 = min(n, j0 + per);
  const double* Q = g.Q + mem * (size_t)n * n;
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; r++) acc[r] = 0;
  for (int c0 = j0; c0 < j1; c0 += kQuadStreamXChunk) {
    const int cn = min(kQuadStreamXChunk, j1 - c0);
    __syncthreads();  // the previous chunk has been read
    if (tid < cn) {
#pragma unroll
      for (int r = 0; r < R; r++) sx[r][tid] = x.p[r][mem * x.stride[r] + c0 + tid];
    }
    __syncthreads();
    if (i < n) {
      const double* col = Q + (size_t)c0 * n + i;
#pragma unroll 8
      for (int j = 0; j < cn; j++) {
        const double q = col[(size_t)j * n];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = fma(q, sx[r][j], acc[r]);
      }
    }
  }
  if (i < n) {
#pragma unroll
    for (int r = 0; r < R; r++) g.part[((mem * splits + s) * 2 + r) * (size_t)n + i] = acc[r];
  }
}

// (Q x_r)_i of cone `mem` from the partials, the splits in order; x_i itself where Q is the identity.
__device__ __forceinline__ double QuadStreamQx(const QuadStreamGroup& g, size_t mem, int r, int i, double x_i) {
  if (g.q_form == kQuadQIdentity) return x_i;
  const double* p = g.part + ((mem * g.splits) * 2 + r) * (size_t)g.n + i;
  double t = 0;
  for (int s = 0; s < g.splits; s++) t += p[(size_t)s * 2 * g.n];
  return t;
}

// ---- once, at cxk_finalize: Qc1 = Q c1 and c1' Q c1 from the partials of a pass over c1.  One workgroup per cone.
__global__ void __launch_bounds__(kQuadStreamBlock) quad_stream_constants(QuadStreamGroup g) {
  __shared__ double scratch[kQuadStreamBlock / 64];
  const int n = g.n, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const double* c1 = g.c + mem * (n + 1) + 1;
  double* qc1 = g.qc1 + mem * n;
  double s = 0;
  for (int i = tid; i < n; i += kQuadStreamBlock) {
    const double q = QuadStreamQx(g, mem, 0, i, c1[i]);
    qc1[i] = q;
    s = fma(c1[i], q, s);
  }
  s = BlockSum(s, scratch);
  if (tid == 0) g.cqc[mem] = s;
}

// ---- Schur complement, stage 1 (after the pass Q w1): Q w1 to the work space, det w, scale and <c1, Q w1>
// (quad_schur's sc[0..2]).  One workgroup per cone.
__global__ void __launch_bounds__(kQuadStreamBlock) quad_stream_schur_vectors(QuadStreamGroup g) {
  __shared__ double scratch[kQuadStreamBlock / 64];
  const int n = g.n, len = n + 1, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const double* c = g.c + mem * len;
  const double* W = g.W + mem * len;
  double* qw = g.qw + mem * n;
  double ww = 0, cw = 0;
  for (int i = tid; i < n; i += kQuadStreamBlock) {
    const double q = QuadStreamQx(g, mem, 0, i, W[1 + i]);
    qw[i] = q;
    ww = fma(W[1 + i], q, ww);
    cw = fma(c[1 + i], q, cw);
  }
  ww = BlockSum(ww, scratch);
  cw = BlockSum(cw, scratch);
  if (tid == 0) {
    const double W0 = W[0];
    g.scal[mem * 8] = W0 * W0 - ww;
    g.scal[mem * 8 + 1] = cw + c[0] * W0;
    g.scal[mem * 8 + 2] = cw;
  }
}

// ---- stage 2: one workgroup per column a_i of a cone, one pass down the column (coalesced):
// v_i = A1[:, i] . Q w1 + A0_i W0 and u_i = A1[:, i] . Q c1.
__global__ void __launch_bounds__(kQuadStreamBlock) quad_stream_schur_columns(QuadStreamGroup g) {
  __shared__ double scratch[kQuadStreamBlock / 64];
  const int n = g.n, m = g.m, len = n + 1, tid = threadIdx.x;
  const size_t mem = blockIdx.x / m;
  const int i = (int)(blockIdx.x % m);
  const double* a = g.A + (mem * m + i) * len;
  const double* qw = g.qw + mem * n;
  const double* qc1 = g.qc1 + mem * n;
  double p = 0, q = 0;
  for (int k = tid; k < n; k += kQuadStreamBlock) {
    const double e = a[1 + k];
    p = fma(e, qw[k], p);
    q = fma(e, qc1[k], q);
  }
  p = BlockSum(p, scratch);
  q = BlockSum(q, scratch);
  if (tid == 0) {
    g.v[mem * m + i] = p + a[0] * g.W[mem * len];
    g.u[mem * m + i] = q;
  }
}

// ---- stage 3: G (the full square), AW, AQc and the two scalars from v, u, A_gram and the scalars, by
// quad_schur's expressions.  Grid: cone x `blocks` workgroups of 256 entries of G; the first of a cone also
// writes AW, AQc and the scalars.  Row 0 of A comes as a pointer and the stride between its entries: (g.A, n + 1) where
// A is dense, a count x m vector with stride 1 where A is held by its nonzeros (kernels_quad_sparse.hip.h).
__global__ void __launch_bounds__(kQuadStreamBlock) quad_stream_schur_finish(QuadStreamGroup g, Arena ar, int blocks, const double* a0,
                                                                             int a0_stride) {
  const int n = g.n, m = g.m, len = n + 1, tid = threadIdx.x;
  const size_t mem = blockIdx.x / blocks;
  const int blk = (int)(blockIdx.x % blocks);
  const int id = g.ids[mem];
  const size_t a0s = (size_t)a0_stride;
  const double* A0 = a0 + mem * m * a0s;
  const double* c = g.c + mem * len;
  const double* Agram = g.Agram + mem * m * m;
  const double* v = g.v + mem * m;
  const double* u = g.u + mem * m;
  const double det_w = g.scal[mem * 8], scale = g.scal[mem * 8 + 1], cdx = g.scal[mem * 8 + 2];
  const double W0 = g.W[mem * len], C0 = c[0];
  double* G = ar.G + ar.g_off[id];
  const long long idx = (long long)blk * kQuadStreamBlock + tid;
  if (idx < (long long)m * m) {
    const int i = (int)(idx % m), j = (int)(idx / m);
    double t = (A0[i * a0s] * A0[j * a0s] - Agram[idx]) * -det_w;
    t += v[i] * v[j];
    t += v[i] * v[j];
    G[idx] = t * 2;
  }
  if (blk != 0) return;
  for (int i = tid; i < m; i += kQuadStreamBlock) {
    double q = det_w * (u[i] - A0[i * a0s] * C0);
    q += 2 * v[i] * scale;
    ar.AWc[ar.r_off[id] + i] = v[i] * 2;
    ar.AQcc[ar.r_off[id] + i] = q * 2;
  }
  if (tid == 0) {
    double cq = det_w * (g.cqc[mem] - C0 * C0);
    cq += 2 * (cdx + C0 * W0) * scale;
    ar.sc[2 * id] = scale * 2;
    ar.sc[2 * id + 1] = cq * 2;
  }
}

// ---- PrepareStep (MODE 0) / eigenvalue query (MODE 1), after the slack and the pass Q [w1, ms1]: w^{1/2} (Sqrt at
// k = |w1|_Q, with Q(f w1) = f Q w1), d = Q(w^{1/2}) ms; d1 to the work space, d0 to the scalars; MODE 0 leaves
// S = (w^{1/2}_1, |w^{1/2}_1|_Q^2) and the scalar part of w^{1/2} in W0 (unless the step is skipped), as
// quad_prepare does.  One workgroup per cone.
template <int MODE>
__global__ void __launch_bounds__(kQuadStreamBlock) quad_stream_prepare_mid(QuadStreamGroup g, StepArgs sa) {
  __shared__ double scratch[kQuadStreamBlock / 64];
  const int n = g.n, len = n + 1, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  double* W = g.W + mem * len;
  double* S = g.S + mem * len;
  const double* ms = g.ms + mem * len;
  double* dv = g.dv + mem * n;
  double ww = 0, wm = 0;
  for (int i = tid; i < n; i += kQuadStreamBlock) {
    const double w = W[1 + i];
    ww = fma(w, QuadStreamQx(g, mem, 0, i, w), ww);
    wm = fma(w, QuadStreamQx(g, mem, 1, i, ms[1 + i]), wm);
  }
  ww = BlockSum(ww, scratch);
  wm = BlockSum(wm, scratch);
  const double W0 = W[0], ms0 = ms[0];
  const double k = sqrt(fabs(ww));
  const double f = k > 0 ? .5 * (sqrt(fabs(W0 + k)) - sqrt(fabs(W0 - k))) / k : 1.0;
  const double w0 = .5 * (sqrt(fabs(W0 + k)) + sqrt(fabs(W0 - k)));
  const double nsq = f * f * ww, ip = f * wm;
  const double det_x = w0 * w0 - nsq, scale = 2 * (w0 * ms0 + ip);
  for (int i = tid; i < n; i += kQuadStreamBlock) {
    const double ws = f * W[1 + i];
    dv[i] = scale * ws + det_x * ms[1 + i];
    if (MODE == 0) S[i] = ws;
  }
  __syncthreads();  // every thread has read W0
  if (tid == 0) {
    g.scal[mem * 8 + 4] = scale * w0 - det_x * ms0;
    if (MODE == 0) {
      S[n] = nsq;
      // (`wsqrt_q0` is *W0 itself; not behind a failed factorization: quad_prepare says why)
      if (!StepSkipped(sa)) W[0] = w0;
    }
  }
}

// ---- after the pass Q d1: |d1|_Q, the norms (MODE 0, with D <- d + e and Q d1 kept for TakeStep) or the
// eigenvalue bounds (MODE 1).  One workgroup per cone.
template <int MODE>
__global__ void __launch_bounds__(kQuadStreamBlock) quad_stream_prepare_finish(QuadStreamGroup g, StepArgs sa) {
  __shared__ double scratch[kQuadStreamBlock / 64];
  const int n = g.n, len = n + 1, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const int id = g.ids[mem];
  double* D = g.D + mem * len;
  const double* dv = g.dv + mem * n;
  double* qd = g.qd + mem * n;
  double dd = 0;
  for (int i = tid; i < n; i += kQuadStreamBlock) {
    const double d = dv[i], q = QuadStreamQx(g, mem, 0, i, d);
    dd = fma(d, q, dd);
    if (MODE == 0) {
      D[1 + i] = d;
      qd[i] = q;
    }
  }
  dd = BlockSum(dd, scratch);
  if (tid != 0) return;
  double d0 = g.scal[mem * 8 + 4];
  const double nd = sqrt(fabs(dd));
  if (MODE == 0) {
    d0 += 1;
    D[0] = d0;
    g.scal[mem * 8 + 5] = dd;
    const double e0 = d0 + nd, e1 = d0 - nd;
    sa.info[2 * id] = e0 * e0 + e1 * e1;
    sa.info[2 * id + 1] = fabs(e0) < fabs(e1) ? fabs(e1) : fabs(e0);
  } else {
    const double e0 = d0 + nd, e1 = d0 - nd;
    const double lmax = -fmin(e0, e1), lmin = -fmax(e0, e1);
    sa.info[4 * id] = lmin;
    sa.info[4 * id + 1] = lmax;
    sa.info[4 * id + 2] = lmax * lmax + lmin * lmin;
    sa.info[4 * id + 3] = lmax + lmin;
  }
}

// ---- TakeStep: d <- exp(step d) in place (Exp at k = |step d1|_Q = |step| |d1|_Q), W <- Q(w^{1/2}) exp(d) with
// w^{1/2} = (W0, S) as PrepareStep left it.  No pass over Q: Q(step f d1) = step f (Q d1).  One workgroup per cone.
__global__ void __launch_bounds__(kQuadStreamBlock) quad_stream_take_step(QuadStreamGroup g, StepArgs sa) {
  if (StepSkipped(sa)) return;  // (enqueued before the host saw the factorization fail: leave W alone)
  __shared__ double scratch[kQuadStreamBlock / 64];
  const int n = g.n, len = n + 1, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  double* W = g.W + mem * len;
  double* D = g.D + mem * len;
  const double* S = g.S + mem * len;
  const double* qd = g.qd + mem * n;
  const double step = StepSizeOf(sa);
  const double d0 = step != 1.0 ? step * D[0] : D[0];
  const double k = sqrt(fabs(step != 1.0 ? (step * step) * g.scal[mem * 8 + 5] : g.scal[mem * 8 + 5]));
  double f = step;
  if (k > 0) f = step * (.5 * (exp(d0 + k) - exp(d0 - k)) / k);
  const double e0 = .5 * (exp(d0 + k) + exp(d0 - k));
  double sq = 0;
  for (int i = tid; i < n; i += kQuadStreamBlock) sq = fma(S[i], qd[i], sq);
  const double ip = f * BlockSum(sq, scratch);
  const double W0 = W[0];
  const double det_x = W0 * W0 - S[n], scale = 2 * (W0 * e0 + ip);
  for (int i = tid; i < n; i += kQuadStreamBlock) {
    const double e = f * D[1 + i];
    D[1 + i] = e;  // (the reference exponentiates its d in place)
    W[1 + i] = scale * S[i] + det_x * e;
  }
  __syncthreads();  // every thread has read W0 and D0
  if (tid == 0) {
    D[0] = e0;
    W[0] = scale * W0 - det_x * e0;
  }
}

}  // namespace cxk
