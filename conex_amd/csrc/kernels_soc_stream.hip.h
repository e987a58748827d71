// Second-order cones whose data does not fit LDS (cxk_set_streamed_cones): the cone stays in HBM and
// every stage is a few launches ordered by the stream alone.  Semantics are those of soc_schur /
// soc_prepare / soc_take_step (kernels_soc.hip.h; reference soc_constraint.cc:14-191, 200-303); what
// differs is who does the work: the O(len) maps run on one 256-thread workgroup per cone that strides
// over the cone, the O(len m) passes on a grid of column / row tiles, and the one dense contraction,
// G = 2 WA^T WA, on the batched fp64 MFMA GEMM (gemm_mfma.hip).
//
// No atomics, no workgroup waits for another: a kernel reads only what an earlier launch on the stream
// wrote.  Every sum is a thread's fma chain over its stride followed by BlockSum (fixed butterfly, then
// the waves in order), so its order depends on the length and the block size only: same bits every run.
//
// Work space per cone (SocStreamGroup): WA (len x m), s = w^{1/2}, wc = Q(s) c, ms (each len), det(s).
#pragma once
#include "kernels_soc.hip.h"

namespace cxk {

// (SocStreamGroup, kSocStreamRowTile and the split rule of the Gram product, SocStreamSplits / kSocStreamMinSplitK, are
// cone_types.h's: the units of the quadratic cones and the linear blocks read them too)
constexpr int kSocStreamBlock = 256;     // threads of every kernel here
constexpr int kSocStreamYChunk = 2048;   // entries of y staged in LDS at a time (16 KB)

// s = w^{1/2} of one cone by the whole workgroup (SocSpectral's expressions): s written to `s`, returns
// det(s) = s_0^2 - |s_1|^2 and (optionally) <s, other> to every thread.
__device__ __forceinline__ double SocStreamSqrt(int len, const double* w, double* s,
                                                const double* other, double* dot, double* scratch) {
  const int tid = threadIdx.x;
  const double w0 = w[0];
  double nq = 0;
  for (int k = tid; k < len; k += kSocStreamBlock)
    if (k > 0) nq = fma(w[k], w[k], nq);
  nq = sqrt(BlockSum(nq, scratch));
  const double f0 = sqrt(w0 + nq), f1 = sqrt(w0 - nq);
  const double s0 = f0 * .5 + f1 * .5;
  double t2 = 0, xy = 0;
  for (int k = tid; k < len; k += kSocStreamBlock) {
    double v = s0;
    if (k > 0) {
      const double q = nq > 0 ? w[k] / nq : 0.0;
      v = nq > 0 ? f0 * (.5 * q) + f1 * (-.5 * q) : 0.0;
      t2 = fma(v, v, t2);
    }
    s[k] = v;
    if (other) xy = fma(v, other[k], xy);
  }
  t2 = BlockSum(t2, scratch);
  if (other) *dot = BlockSum(xy, scratch);
  return s0 * s0 - t2;
}

// ---- Schur complement, stage 1: s, det(s), wc = Q(s) c and the two scalars.  One workgroup per cone.
__global__ void __launch_bounds__(kSocStreamBlock) soc_stream_vectors(SocStreamGroup g, Arena ar) {
  __shared__ double scratch[kSocStreamBlock / 64];
  const int len = g.v.len, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const int id = g.v.ids[mem];
  const double* c = g.v.c + mem * len;
  double* s = g.s + mem * len;
  double* wc = g.wc + mem * len;
  double sc_dot = 0;
  const double det = SocStreamSqrt(len, g.v.W + mem * len, s, c, &sc_dot, scratch);
  double q = 0, wc0 = 0;
  for (int k = tid; k < len; k += kSocStreamBlock) {  // (each thread reads back the s it wrote itself)
    const double v = (2 * sc_dot) * s[k] + (k == 0 ? -det * c[k] : det * c[k]);
    wc[k] = v;
    if (k == 0) wc0 = v;
    q = fma(v, v, q);
  }
  q = BlockSum(q, scratch);
  if (tid == 0) {
    g.dets[mem] = det;
    ar.sc[2 * id] = 2 * wc0;
    ar.sc[2 * id + 1] = 2 * q;
  }
}

// ---- stage 2: one workgroup per column a_i of a cone: p = s . a_i, AW_i = 2 a_i . w, then
// WA_i = Q(s) a_i = 2 p s - det(s) R a_i to the work space and AQc_i = 2 WA_i . wc.  Both passes run down
// the column (coalesced); the second finds it in the cache where it fits.
__global__ void __launch_bounds__(kSocStreamBlock) soc_stream_apply(SocStreamGroup g, Arena ar) {
  __shared__ double scratch[kSocStreamBlock / 64];
  const int len = g.v.len, m = g.v.m, tid = threadIdx.x;
  const size_t mem = blockIdx.x / m;
  const int i = (int)(blockIdx.x % m);
  const int id = g.v.ids[mem];
  const double* a = g.v.A + (mem * m + i) * len;
  const double* w = g.v.W + mem * len;
  const double* s = g.s + mem * len;
  const double* wc = g.wc + mem * len;
  double* WA = g.WA + (mem * m + i) * len;
  const double det = g.dets[mem];
  double p = 0, aw = 0;
  for (int k = tid; k < len; k += kSocStreamBlock) {
    const double v = a[k];
    p = fma(s[k], v, p);
    aw = fma(v, w[k], aw);
  }
  p = BlockSum(p, scratch);
  aw = BlockSum(aw, scratch);
  double q = 0;
  for (int k = tid; k < len; k += kSocStreamBlock) {
    const double v = (2 * p) * s[k] + (k == 0 ? -det * a[k] : det * a[k]);
    WA[k] = v;
    q = fma(v, wc[k], q);
  }
  q = BlockSum(q, scratch);
  if (tid == 0) {
    ar.AWc[ar.r_off[id] + i] = 2 * aw;
    ar.AQcc[ar.r_off[id] + i] = 2 * q;
  }
}

// ---- stage 3 is the GEMM (LaunchSocStreamSchur); this copies its lower triangle to the full square
// soc_schur writes.
__global__ void __launch_bounds__(kSocStreamBlock) soc_stream_mirror(SocStreamGroup g, Arena ar) {
  const int m = g.v.m;
  const size_t mm = (size_t)m * m, total = mm * g.v.count;
  for (size_t e = blockIdx.x * (size_t)kSocStreamBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kSocStreamBlock) {
    const size_t mem = e / mm;
    const int idx = (int)(e % mm), i = idx % m, j = idx / m;
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    ar.G[ar.g_off[g.v.ids[mem]] + idx] = g.Gf[mem * mm + hi + (size_t)lo * m];
  }
}

// ---- PrepareStep / eigenvalue query, phase 1: ms = A y - c_weight c on a grid of cone x row tiles, one
// row per thread, y staged in LDS a chunk at a time.
__global__ void __launch_bounds__(kSocStreamBlock) soc_stream_slack(SocStreamGroup g, StepArgs sa, int tiles) {
  sa.c_weight = CWeightOf(sa);  // (the barrier parameter may live on the device: cxk_select_mu_async)
  __shared__ double sy[kSocStreamYChunk];
  const int len = g.v.len, m = g.v.m, tid = threadIdx.x;
  const size_t mem = blockIdx.x / tiles;
  const int k = (int)(blockIdx.x % tiles) * kSocStreamRowTile + tid;
  const int id = g.v.ids[mem];
  const double* A = g.v.A + mem * len * m;
  const int* perm = sa.cl_perm + sa.cl_ptr[id];
  double acc = 0;
  for (int j0 = 0; j0 < m; j0 += kSocStreamYChunk) {
    const int jn = min(kSocStreamYChunk, m - j0);
    __syncthreads();  // the previous chunk has been read
    for (int q = tid; q < jn; q += kSocStreamBlock) sy[q] = sa.y[perm[j0 + q]];
    __syncthreads();
    if (k < len)
      for (int j = 0; j < jn; j++) acc = fma(A[k + (size_t)(j0 + j) * len], sy[j], acc);
  }
  if (k < len) g.ms[mem * len + k] = acc - g.v.c[mem * len + k] * sa.c_weight;
}

// ---- phase 2: d = Q(s) ms (+ e), the norms (MODE 0) or eigenvalue bounds (MODE 1), D <- d, W <- s.  One
// workgroup per cone.  s is formed from W here (not taken from the last assembly): W may have changed since.
template <int MODE>
__global__ void __launch_bounds__(kSocStreamBlock) soc_stream_prepare(SocStreamGroup g, StepArgs sa) {
  __shared__ double scratch[kSocStreamBlock / 64];
  const int len = g.v.len, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  const int id = g.v.ids[mem];
  double* W = g.v.W + mem * len;
  double* D = g.v.T1 + mem * len;
  double* s = g.s + mem * len;
  const double* ms = g.ms + mem * len;
  double xy = 0;
  const double det = SocStreamSqrt(len, W, s, ms, &xy, scratch);
  // PrepareStep leaves w^{1/2} in W (soc_constraint.cc:259-261) -- unless it was enqueued behind a
  // factorization that turns out to have failed (soc_prepare says why)
  const bool keep_w = MODE != 0 || StepSkipped(sa);
  double all = 0, tail = 0, d0 = 0;
  for (int k = tid; k < len; k += kSocStreamBlock) {  // (each thread reads back the s it wrote itself)
    const double sk = s[k];
    double d = (2 * xy) * sk + (k == 0 ? -det * ms[k] : det * ms[k]);
    if (MODE == 0) {
      if (k == 0) d += 1;
      D[k] = d;
      if (!keep_w) W[k] = sk;
      all = fma(d, d, all);
    }
    if (k == 0)
      d0 = d;
    else
      tail = fma(d, d, tail);
  }
  if (MODE == 0) all = BlockSum(all, scratch);
  const double nq = sqrt(BlockSum(tail, scratch));
  if (tid == 0) {  // (thread 0 holds d_0)
    if (MODE == 0) {
      const double e0 = fabs(d0 + nq), e1 = fabs(d0 - nq);
      sa.info[2 * id] = 2 * all;
      sa.info[2 * id + 1] = e0 > e1 ? e0 : e1;
    } else {
      const double e0 = d0 + nq, e1 = d0 - nq;
      const double lmax = -fmin(e0, e1), lmin = -fmax(e0, e1);
      sa.info[4 * id] = lmin;
      sa.info[4 * id + 1] = lmax;
      sa.info[4 * id + 2] = lmax * lmax + lmin * lmin;
      sa.info[4 * id + 3] = lmax + lmin;
    }
  }
}

// ---- TakeStep: d <- step d, W <- Q(w) exp(d) with w the w^{1/2} PrepareStep left in W.  One workgroup per cone.
__global__ void __launch_bounds__(kSocStreamBlock) soc_stream_take_step(SocStreamGroup g, StepArgs sa) {
  if (StepSkipped(sa)) return;  // (enqueued before the host saw the factorization fail: leave W alone)
  __shared__ double scratch[kSocStreamBlock / 64];
  const int len = g.v.len, tid = threadIdx.x;
  const size_t mem = blockIdx.x;
  double* W = g.v.W + mem * len;
  double* D = g.v.T1 + mem * len;
  double* ex = g.ms + mem * len;
  const double step = StepSizeOf(sa);
  const double w0 = W[0];
  const double d0 = step != 1.0 ? D[0] * step : D[0];  // (D[0] itself stays: the reference scales temp1_1 only)
  double nq = 0, t2 = 0;
  for (int k = tid; k < len; k += kSocStreamBlock) {
    if (k == 0) continue;
    double d = D[k];
    if (step != 1.0) {
      d *= step;
      D[k] = d;
    }
    nq = fma(d, d, nq);
    t2 = fma(W[k], W[k], t2);
  }
  nq = sqrt(BlockSum(nq, scratch));
  t2 = BlockSum(t2, scratch);
  const double f0 = exp(d0 + nq), f1 = exp(d0 - nq);
  const double ex0 = f0 * .5 + f1 * .5;
  double xy = 0;
  for (int k = tid; k < len; k += kSocStreamBlock) {  // (D[k] as this thread left it above)
    double v = ex0;
    if (k > 0) {
      const double q = nq > 0 ? D[k] / nq : 0.0;
      v = nq > 0 ? f0 * (.5 * q) + f1 * (-.5 * q) : 0.0;
    }
    ex[k] = v;
    xy = fma(W[k], v, xy);
  }
  xy = BlockSum(xy, scratch);
  const double det = w0 * w0 - t2;
  for (int k = tid; k < len; k += kSocStreamBlock) W[k] = (2 * xy) * W[k] + (k == 0 ? -det * ex[k] : det * ex[k]);
}

}  // namespace cxk
