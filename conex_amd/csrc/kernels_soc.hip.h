// Second-order (spin factor) cone kernels on the LDS route.
//
// Reference semantics:
//   ConstructSchurComplementSystem(SOCConstraint*)     soc_constraint.cc:272-303
//   Sqrt/Exp/QuadraticRepresentation/NormInf           soc_constraint.cc:14-191
//   PrepareStep/TakeStep/GetWeightedSlackEigenvalues   soc_constraint.cc:200-270
#pragma once
#include "cone_types.h"
#include "device_utils.h"

namespace cxk {

// -------------------------------------------------------------------- SOC
// z = f(x) through the spin-factor spectral decomposition; op 0 sqrt, 1 exp. Single thread.
__device__ inline void SocSpectral(int n, double x0, const double* x1, int op, double* z) {
  double nq = 0;
  for (int i = 0; i < n; i++) nq = fma(x1[i], x1[i], nq);
  nq = sqrt(nq);
  const double e0 = x0 + nq, e1 = x0 - nq;
  const double f0 = op == 0 ? sqrt(e0) : exp(e0);
  const double f1 = op == 0 ? sqrt(e1) : exp(e1);
  z[0] = f0 * .5 + f1 * .5;
  for (int i = 0; i < n; i++) {
    const double q = nq > 0 ? x1[i] / nq : 0.0;
    z[1 + i] = nq > 0 ? f0 * (.5 * q) + f1 * (-.5 * q) : 0.0;
  }
}

// out = Q(x) y = 2 (x.y) x - det(x) R y
__device__ inline void SocQuadRep(int len, const double* x, const double* y, double* out) {
  double t2 = 0, xy = 0;
  for (int i = 1; i < len; i++) t2 = fma(x[i], x[i], t2);
  for (int i = 0; i < len; i++) xy = fma(x[i], y[i], xy);
  const double det = x[0] * x[0] - t2;
  for (int i = 0; i < len; i++) out[i] = (2 * xy) * x[i] + (i == 0 ? -det * y[i] : det * y[i]);
}

// The two maps above dealt to the lanes of one wavefront: the reductions stay one lane's fma chain
// (their order is the single-thread order: same bits), the per-element work -- above all the n
// divisions of the spectral map -- runs one element per lane.  A SIMD issues a vector instruction
// in the same 4-8 cycles whether one lane or all are active, and with five single-lane cones
// resident per SIMD the serial forms cost 16 us per launch of 5000 cones.  x / y may be global or
// LDS; z / out LDS (read back by other lanes: the caller synchronises the wavefront afterwards).
__device__ __forceinline__ void SocSpectralWave(int n, double x0, const double* x1, int op, double* z, int lane) {
  double nq = 0;
  for (int i = 0; i < n; i++) nq = fma(x1[i], x1[i], nq);  // every lane the same chain: no broadcast needed
  nq = sqrt(nq);
  const double e0 = x0 + nq, e1 = x0 - nq;
  const double f0 = op == 0 ? sqrt(e0) : exp(e0);
  const double f1 = op == 0 ? sqrt(e1) : exp(e1);
  if (lane == 0) z[0] = f0 * .5 + f1 * .5;
  for (int i = lane; i < n; i += 64) {
    const double q = nq > 0 ? x1[i] / nq : 0.0;
    z[1 + i] = nq > 0 ? f0 * (.5 * q) + f1 * (-.5 * q) : 0.0;
  }
}
__device__ __forceinline__ void SocQuadRepWave(int len, const double* x, const double* y, double* out, int lane) {
  double t2 = 0, xy = 0;
  for (int i = 1; i < len; i++) t2 = fma(x[i], x[i], t2);
  for (int i = 0; i < len; i++) xy = fma(x[i], y[i], xy);
  const double det = x[0] * x[0] - t2;
  for (int i = lane; i < len; i += 64) out[i] = (2 * xy) * x[i] + (i == 0 ? -det * y[i] : det * y[i]);
}

// One wavefront per cone, four cones per workgroup.
// STAGED: the cone's data (A, c, W) is copied to LDS in one round trip first; large cones whose
// staged image would not fit read their operands where they are.
template <bool STAGED>
__global__ void __launch_bounds__(256) soc_schur(VecGroup g, Arena ar) {
  extern __shared__ double lds_all[];
  const int len = g.len, n = len - 1, m = g.m;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int mem = blockIdx.x * nw + wave;
  if (mem >= g.count) return;  // wave-uniform; only wavefront-level synchronisation below
  double* lds = lds_all + (size_t)wave * (len * (STAGED ? 2 * m + 4 : m + 2));
  const int id = g.ids[mem];
  const double* A = g.A + (size_t)mem * len * m;
  const double* c = g.c + (size_t)mem * len;
  const double* W = g.W + (size_t)mem * len;
  double* wsqrt = lds;            // len
  double* wc = wsqrt + len;       // len
  double* WA = wc + len;          // len x m
  const double *sA = A, *sW = W, *sC = c;
  double* G = ar.G + ar.g_off[id];
  double* AW = ar.AWc + ar.r_off[id];
  double* AQc = ar.AQcc + ar.r_off[id];
  if constexpr (STAGED) {  // (otherwise the phases below fetch their operands themselves: four dependent round trips)
    double* tA = WA + len * m;  // len x m
    double* tW = tA + len * m;  // len
    double* tC = tW + len;      // len
    for (int q = lane; q < len * m; q += 64) tA[q] = A[q];
    for (int q = lane; q < len; q += 64) {
      tW[q] = W[q];
      tC[q] = c[q];
    }
    sA = tA;
    sW = tW;
    sC = tC;
    WaveSync();
  }
  SocSpectralWave(n, sW[0], sW + 1, 0, wsqrt, lane);
  WaveSync();
  SocQuadRepWave(len, wsqrt, sC, wc, lane);
  WaveSync();
  for (int i = lane; i < m; i += 64) SocQuadRep(len, wsqrt, sA + (size_t)i * len, WA + i * len);
  WaveSync();
  for (int idx = lane; idx < m * m; idx += 64) {
    const int i = idx % m, j = idx / m;
    double s = 0;
    for (int k = 0; k < len; k++) s = fma(WA[k + i * len], WA[k + j * len], s);
    G[idx] = 2 * s;
  }
  for (int i = lane; i < m; i += 64) {
    double a = 0, q = 0;
    for (int k = 0; k < len; k++) {
      a = fma(sA[k + (size_t)i * len], sW[k], a);
      q = fma(WA[k + i * len], wc[k], q);
    }
    AW[i] = 2 * a;
    AQc[i] = 2 * q;
  }
  if (lane == 0) {
    double s = 0;
    for (int k = 0; k < len; k++) s = fma(wc[k], wc[k], s);
    ar.sc[2 * id] = 2 * wc[0];
    ar.sc[2 * id + 1] = 2 * s;
  }
}

template <int MODE>
__global__ void __launch_bounds__(64) soc_prepare(VecGroup g, StepArgs sa) {
  sa.c_weight = CWeightOf(sa);  // (the barrier parameter may live on the device: cxk_select_mu_async)
  extern __shared__ double lds[];
  const int len = g.len, n = len - 1, m = g.m;
  const int mem = blockIdx.x, id = g.ids[mem];
  const double* A = g.A + (size_t)mem * len * m;
  const double* c = g.c + (size_t)mem * len;
  double* W = g.W + (size_t)mem * len;
  double* D = g.T1 + (size_t)mem * len;
  double* sy = lds;          // m
  double* ms = sy + m;       // len
  double* wsqrt = ms + len;  // len
  double* d = wsqrt + len;   // len
  for (int q = threadIdx.x; q < m; q += blockDim.x) sy[q] = sa.y[sa.cl_perm[sa.cl_ptr[id] + q]];
  __syncthreads();
  for (int k = threadIdx.x; k < len; k += blockDim.x) {
    double s = 0;
    for (int j = 0; j < m; j++) s = fma(A[k + (size_t)j * len], sy[j], s);
    ms[k] = s - c[k] * sa.c_weight;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    SocSpectral(n, W[0], W + 1, 0, wsqrt);
    SocQuadRep(len, wsqrt, ms, d);
    double nq = 0;
    if (MODE == 0) {
      // PrepareStep leaves w^{1/2} in W (soc_constraint.cc:259-261) -- unless it was enqueued behind a
      // factorization that turns out to have failed: the reference returns before PrepareStep then,
      // with W untouched (cone_program.cc:360-371)
      if (!StepSkipped(sa))
        for (int k = 0; k < len; k++) W[k] = wsqrt[k];
      d[0] += 1;
      double s = 0;
      for (int k = 0; k < len; k++) {
        D[k] = d[k];
        s = fma(d[k], d[k], s);
      }
      for (int k = 1; k < len; k++) nq = fma(d[k], d[k], nq);
      nq = sqrt(nq);
      const double e0 = fabs(d[0] + nq), e1 = fabs(d[0] - nq);
      sa.info[2 * id] = 2 * s;
      sa.info[2 * id + 1] = e0 > e1 ? e0 : e1;
    } else {
      for (int k = 1; k < len; k++) nq = fma(d[k], d[k], nq);
      nq = sqrt(nq);
      const double e0 = d[0] + nq, e1 = d[0] - nq;
      const double lmax = -fmin(e0, e1), lmin = -fmax(e0, e1);
      sa.info[4 * id] = lmin;
      sa.info[4 * id + 1] = lmax;
      sa.info[4 * id + 2] = lmax * lmax + lmin * lmin;
      sa.info[4 * id + 3] = lmax + lmin;
    }
  }
}

__global__ void __launch_bounds__(64) soc_take_step(VecGroup g, StepArgs sa) {
  if (StepSkipped(sa)) return;  // (enqueued before the host saw the factorization fail: leave W alone)
  extern __shared__ double lds[];
  const int len = g.len, n = len - 1;
  const int mem = blockIdx.x;
  double* W = g.W + (size_t)mem * len;
  double* D = g.T1 + (size_t)mem * len;
  double* d = lds;
  double* ex = d + len;
  double* wn = ex + len;
  double* w = wn + len;
  if (threadIdx.x == 0) {
    for (int k = 0; k < len; k++) {
      d[k] = D[k];
      w[k] = W[k];
    }
    const double step = StepSizeOf(sa);
    if (step != 1.0) {
      for (int k = 0; k < len; k++) d[k] *= step;
      for (int k = 1; k < len; k++) D[k] = d[k];  // the reference scales temp1_1 in place
    }
    SocSpectral(n, d[0], d + 1, 1, ex);
    SocQuadRep(len, w, ex, wn);
    for (int k = 0; k < len; k++) W[k] = wn[k];
  }
}

}  // namespace cxk
