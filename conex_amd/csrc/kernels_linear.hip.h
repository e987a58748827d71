// Linear (nonnegative orthant) cone kernels on the LDS route: one workgroup per constraint.  linear_take_step and
// vec_set_identity are grid-wide and serve every route of the family (vec_set_identity the second-order and
// quadratic cones too, through cone_linear.hip's launcher).
//
// Reference semantics:
//   ConstructSchurComplementSystem(LinearConstraint*)  linear_constraint.cc:177-205
//   PrepareStep/TakeStep/GetWeightedSlackEigenvalues   linear_constraint.cc:108-175
#pragma once
#include "cone_types.h"
#include "device_utils.h"

namespace cxk {

// ------------------------------------------------------------------ linear
__global__ void __launch_bounds__(256) linear_schur(VecGroup g, Arena ar) {
  __shared__ double red[8];
  const int r = g.len, m = g.m;
  const int mem = blockIdx.x, id = g.ids[mem];
  const double* A = g.A + (size_t)mem * r * m;
  const double* c = g.c + (size_t)mem * r;
  const double* w = g.W + (size_t)mem * r;
  double* G = ar.G + ar.g_off[id];
  double* AW = ar.AWc + ar.r_off[id];
  double* AQc = ar.AQcc + ar.r_off[id];
  for (int idx = threadIdx.x; idx < m * m; idx += blockDim.x) {
    const int i = idx % m, j = idx / m;
    double s = 0;
    for (int k = 0; k < r; k++) {
      const double wk = w[k];
      s = fma(wk * A[k + (size_t)i * r], wk * A[k + (size_t)j * r], s);
    }
    G[idx] = s;
  }
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    double a = 0, q = 0;
    for (int k = 0; k < r; k++) {
      const double wk = w[k];
      a = fma(A[k + (size_t)i * r], wk, a);
      q = fma(wk * A[k + (size_t)i * r], wk * c[k], q);
    }
    AW[i] = a;
    AQc[i] = q;
  }
  double s1 = 0, s2 = 0;
  for (int k = threadIdx.x; k < r; k += blockDim.x) {
    const double wc = w[k] * c[k];
    s1 += wc;
    s2 = fma(wc, wc, s2);
  }
  s1 = BlockSum(s1, red);
  s2 = BlockSum(s2, red);
  if (threadIdx.x == 0) {
    ar.sc[2 * id] = s1;
    ar.sc[2 * id + 1] = s2;
  }
}

// PerformLineSearch(LinearConstraint*) + FindMinimumMu (LineSearchArgs, cone_types.h)
__global__ void __launch_bounds__(256) linear_line_search(VecGroup g, LineSearchArgs a) {
  extern __shared__ double lds[];
  __shared__ double red[8];
  const int r = g.len, m = g.m;
  const int mem = blockIdx.x, id = g.ids[mem];
  const double* A = g.A + (size_t)mem * r * m;
  const double* c = g.c + (size_t)mem * r;
  const double* w = g.W + (size_t)mem * r;
  double* s0 = lds;
  double* s1 = lds + m;
  for (int q = threadIdx.x; q < m; q += blockDim.x) {
    const int v = a.cl_perm[a.cl_ptr[id] + q];
    s0[q] = a.y0[v];
    s1[q] = a.y1[v];
  }
  __syncthreads();
  double ub = 1.7976931348623157e308, lb = -1.7976931348623157e308;
  for (int k = threadIdx.x; k < r; k += blockDim.x) {
    double t0 = 0, t1 = 0;
    for (int j = 0; j < m; j++) {
      t0 = fma(A[k + (size_t)j * r], s0[j], t0);
      t1 = fma(A[k + (size_t)j * r], s1[j], t1);
    }
    t0 -= c[k] * a.c0_weight;
    t1 -= c[k] * a.c1_weight;
    const double d0 = t0 * w[k] + 1, d1 = t1 * w[k] + 1;
    const double delta = d1 - d0;
    double ubi = (a.dinfmax - d0) / delta, lbi = (-a.dinfmax - d0) / delta;
    if (lbi > ubi) {
      const double t = ubi;
      ubi = lbi;
      lbi = t;
    }
    ub = fmin(ub, ubi);
    lb = fmax(lb, lbi);
  }
  lb = WaveMax(lb);
  ub = -WaveMax(-ub);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave] = lb;
    red[4 + wave] = ub;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = blockDim.x >> 6;
    for (int q = 1; q < nw; q++) {
      lb = fmax(lb, red[q]);
      ub = fmin(ub, red[4 + q]);
    }
    a.out[2 * id] = lb;
    a.out[2 * id + 1] = ub;
  }
}

// mode 0 PrepareStep, mode 1 GetWeightedSlackEigenvalues
template <int MODE>
__global__ void __launch_bounds__(256) linear_prepare(VecGroup g, StepArgs sa) {
  sa.c_weight = CWeightOf(sa);  // (the barrier parameter may live on the device: cxk_select_mu_async)
  extern __shared__ double lds[];
  __shared__ double red[8];
  const int r = g.len, m = g.m;
  const int mem = blockIdx.x, id = g.ids[mem];
  const double* A = g.A + (size_t)mem * r * m;
  const double* c = g.c + (size_t)mem * r;
  double* w = g.W + (size_t)mem * r;
  double* T1 = g.T1 + (size_t)mem * r;
  double* T2 = g.T2 + (size_t)mem * r;
  double* sy = lds;
  for (int q = threadIdx.x; q < m; q += blockDim.x) sy[q] = sa.y[sa.cl_perm[sa.cl_ptr[id] + q]];
  __syncthreads();
  const double kc = (MODE == 0 && sa.affine) ? 0.0 : sa.c_weight;
  double mx = 0, mn = 0, s2 = 0, s1 = 0;
  bool first = true;
  for (int k = threadIdx.x; k < r; k += blockDim.x) {
    double s = 0;
    for (int j = 0; j < m; j++) s = fma(A[k + (size_t)j * r], sy[j], s);
    s -= c[k] * kc;
    if (MODE == 0) {
      if (sa.affine) {  // AffineUpdate: SW = minus_s .* W ; W += W .* SW
        const double sw = s * w[k];
        T1[k] = sw;
        w[k] += w[k] * sw;
      } else {
        const double d = s * w[k] + sa.e_weight;
        T2[k] = d;
        mx = fmax(mx, fabs(d));
        s2 = fma(d, d, s2);
      }
    } else {
      const double ws = w[k] * s;
      mx = first ? ws : fmax(mx, ws);
      mn = first ? ws : fmin(mn, ws);
      first = false;
      s2 = fma(ws, ws, s2);
      s1 += ws;
    }
  }
  if (MODE == 0 && sa.affine) return;
  if (MODE == 1) {  // lanes without rows must not disturb min/max
    if (first) {
      mx = -1.7976931348623157e308;
      mn = 1.7976931348623157e308;
    }
    mn = -WaveMax(-mn);
  }
  mx = WaveMax(mx);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    red[wave] = mx;
    red[4 + wave] = mn;
  }
  __syncthreads();
  const int nw = blockDim.x >> 6;
  double gmx = red[0], gmn = red[4];
  for (int q = 1; q < nw; q++) {
    gmx = fmax(gmx, red[q]);
    gmn = fmin(gmn, red[4 + q]);
  }
  __syncthreads();
  s2 = BlockSum(s2, red);
  s1 = BlockSum(s1, red);
  if (threadIdx.x == 0) {
    if (MODE == 0) {
      sa.info[2 * id] = s2;
      sa.info[2 * id + 1] = gmx;
    } else {
      sa.info[4 * id] = -gmx;
      sa.info[4 * id + 1] = -gmn;
      sa.info[4 * id + 2] = s2;
      sa.info[4 * id + 3] = -s1;
    }
  }
}

__global__ void linear_take_step(VecGroup g, StepArgs sa) {
  if (StepSkipped(sa)) return;  // (enqueued before the host saw the factorization fail: leave W alone)
  const size_t total = (size_t)g.count * g.len;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total;
       q += (size_t)gridDim.x * blockDim.x) {
    double d = g.T2[q];
    const double step = StepSizeOf(sa);
    if (step != 1) d *= step;
    g.T2[q] = d;
    g.W[q] *= exp(d);
  }
}

__global__ void vec_set_identity(VecGroup g, int soc) {
  const size_t total = (size_t)g.count * g.len;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total;
       q += (size_t)gridDim.x * blockDim.x)
    g.W[q] = soc ? ((q % g.len) == 0 ? 1.0 : 0.0) : 1.0;
}

}  // namespace cxk
