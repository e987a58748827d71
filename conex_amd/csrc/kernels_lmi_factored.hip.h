// Dense-LMI constraints given by factors: A_i = sum_{k in i} sigma_k f_k f_k^T, the columns k of
// F = [f_1 .. f_R] (n x R) in [ptr[i], ptr[i+1]) belonging to A_i.  The A_i are never formed.  With
// Z = W F, P = F^T Z, Y = C Z (three batched GEMMs of kernels_gemm.hip.h):
//   G(i,j) = tr(A_i W A_j W)  = sum_{k in i, l in j} sigma_k sigma_l P_kl^2
//   AW(i)  = tr(A_i W)        = sum_{k in i} sigma_k P_kk
//   AQc(i) = tr(A_i W C W)    = sum_{k in i} sigma_k z_k^T (C z_k)
//   S      = sum_i y_i A_i - kC = F diag(sigma_k y_i(k)) F^T - kC
// (DenseLMIConstraint semantics: dense_lmi_constraint.cc:8-27, 72-103.)  <w,c> and <c,Qc> come from
// X = W C W as for a sparse group with a dense C (lmi_dense_c_scalars).  Everything behind the slack is
// the large-order route's (LmiLargeAfterSlack, LmiLargeTakeStep) on this group's S.
// Every sum has a fixed order, nothing is atomic, no workgroup waits for another: same input, same bits.
#pragma once
#include "kernels_lmi_large.hip.h"
#include "kernels_lmi_sparse.hip.h"

namespace cxk {

struct LmiFactoredGroup {
  int R;                // columns of F per member
  int rank_one;         // every A_i of every member has exactly one column (R == m, column i is A_i's)
  const double* F;      // count x (n x R), column-major
  const double* sigma;  // count x R
  const int* ptr;       // count x (m + 1): columns of A_i
  const int* var;       // count x R: column -> its variable
  double* Z;            // count x (n x R)   W F
  double* Y;            // count x (n x R)   C Z
  double* Fs;           // count x (n x R)   F diag(sigma_k y_i(k))  (slack)
  double* P;            // count x (R x R)   F^T W F, lower triangle
  double* part;         // count x npart x 2 partial sums of <w,c>, <c,Qc>
  int npart;
};

// G (lower triangle), AW, AQc and the two scalars into the arena.  grid (gb + wb, count): the first
// gb = ceil(m^2 / 256) workgroups give a thread to every (i, j) of G; behind them a wavefront per variable
// forms AQc(i) and AW(i), and one more adds the partial sums of the scalars.  Only P(k, l) with k >= l is read
// (P(k, l) and P(l, k) are different sums of the GEMM).  RANK1: G(i, j) = sigma_i sigma_j P_ij^2, no block sums.
template <bool RANK1>
__global__ void __launch_bounds__(256) lmi_factored_finalize(LmiGroup g, LmiFactoredGroup f, Arena ar, int gb) {
  const int n = g.n, m = g.m, R = f.R;
  const int mem = blockIdx.y, id = g.ids[mem];
  const double* P = f.P + (size_t)mem * R * R;
  const double* sg = f.sigma + (size_t)mem * R;
  const int* ptr = f.ptr + (size_t)mem * (m + 1);
  if ((int)blockIdx.x < gb) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)m * m) return;
    const int i = (int)(e % m), j = (int)(e / m);
    if (i < j) return;
    double acc = 0.0;
    if constexpr (RANK1) {
      const double p = P[i + (size_t)j * R];
      acc = (p * p) * (sg[i] * sg[j]);
    } else {
      const int k0 = ptr[i], k1 = ptr[i + 1], l0 = ptr[j], l1 = ptr[j + 1];
      for (int k = k0; k < k1; k++) {
        double row = 0.0;
        for (int l = l0; l < l1; l++) {
          const double p = k >= l ? P[k + (size_t)l * R] : P[l + (size_t)k * R];
          row = fma(sg[l] * p, p, row);
        }
        acc = fma(sg[k], row, acc);
      }
    }
    ar.G[ar.g_off[id] + i + (size_t)j * m] = acc;
    return;
  }
  const int lane = threadIdx.x & 63;
  const int w = ((int)blockIdx.x - gb) * 4 + (threadIdx.x >> 6);
  if (w < m) {
    const double* Z = f.Z + (size_t)mem * n * R;
    const double* Y = f.Y + (size_t)mem * n * R;
    const int k0 = RANK1 ? w : ptr[w], k1 = RANK1 ? w + 1 : ptr[w + 1];
    double aw = 0.0, aq = 0.0;
    for (int k = k0; k < k1; k++) {
      double d = 0.0;
      for (int r = lane; r < n; r += 64) d = fma(Z[r + (size_t)k * n], Y[r + (size_t)k * n], d);
      d = WaveSum(d);
      aq = fma(sg[k], d, aq);
      aw = fma(sg[k], P[k + (size_t)k * R], aw);
    }
    if (lane == 0) {
      ar.AWc[ar.r_off[id] + w] = aw;
      ar.AQcc[ar.r_off[id] + w] = aq;
    }
  } else if (w == m) {
    // <w,c>, <c,Qc>: the slices of lmi_dense_c_scalars, lane l adds slices l, l + 64, .. then the fixed butterfly
    const double* part = f.part + (size_t)mem * f.npart * 2;
    double wc = 0.0, cq = 0.0;
    for (int q = lane; q < f.npart; q += 64) {
      wc += part[2 * q];
      cq += part[2 * q + 1];
    }
    wc = WaveSum(wc);
    cq = WaveSum(cq);
    if (lane == 0) {
      ar.sc[2 * id] = wc;
      ar.sc[2 * id + 1] = cq;
    }
  }
}

// S = -k C and Fs = F diag(sigma_k y_i(k)); grid (blocks over n^2 + n R, count).  The GEMM behind it adds Fs F^T.
__global__ void __launch_bounds__(256) lmi_factored_slack(LmiGroup g, LmiFactoredGroup f, StepArgs sa, double* __restrict__ S) {
  const int n = g.n, R = f.R;
  const int mem = blockIdx.y, id = g.ids[mem];
  const int64_t nn = (int64_t)n * n, nr = (int64_t)n * R;
  const double* Cm = g.C + (size_t)mem * nn;
  const double* F = f.F + (size_t)mem * nr;
  double* Fs = f.Fs + (size_t)mem * nr;
  const double* sg = f.sigma + (size_t)mem * R;
  const int* var = f.var + (size_t)mem * R;
  const int cl0 = sa.cl_ptr[id];
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nn + nr; q += (int64_t)gridDim.x * blockDim.x) {
    if (q < nn) {
      S[(size_t)mem * nn + q] = -(sa.c_weight * Cm[q]);
    } else {
      const int64_t e = q - nn;
      const int k = (int)(e / n);
      Fs[e] = F[e] * (sg[k] * sa.y[sa.cl_perm[cl0 + var[k]]]);
    }
  }
}

// ---- host-side drivers --------------------------------------------------------------------
inline hipError_t LmiFactoredSchur(const LmiGroup& g, const LmiFactoredGroup& f, const Arena& ar, const LmiLargeWs& ws,
                                   hipStream_t st) {
  const int n = g.n, m = g.m, R = f.R;
  const int64_t nn = (int64_t)n * n, nr = (int64_t)n * R;
  hipError_t e;
  if (R > 0) {
    GemmArgs a{};
    a.inner = 1;
    a.alpha = 1.0;
    a.beta = 0.0;
    a.splits = 1;
    // Z = W F
    a.M = n, a.N = R, a.K = n;
    a.A = g.W, a.lda = n, a.sA1 = nn;
    a.B = f.F, a.ldb = n, a.sB1 = nr;
    a.C = f.Z, a.ldc = n, a.sC1 = nr;
    if ((e = LaunchGemm(a, false, false, g.count, st)) != hipSuccess) return e;
    // Y = C Z
    a.A = g.C;
    a.B = f.Z;
    a.C = f.Y;
    if ((e = LaunchGemm(a, false, false, g.count, st)) != hipSuccess) return e;
    // P = F^T Z, lower triangle
    a.M = a.N = R, a.K = n;
    a.A = f.F, a.lda = n, a.sA1 = nr;
    a.B = f.Z, a.ldb = n, a.sB1 = nr;
    a.C = f.P, a.ldc = R, a.sC1 = (int64_t)R * R;
    a.lower_only = 1;
    if ((e = LaunchGemm(a, true, false, g.count, st)) != hipSuccess) return e;
  }
  {  // X = W (C W), then the slices of <C, W> and <C, X>
    double* CW = ws.tmp;
    double* X = ws.tmp + (size_t)g.count * nn;
    GemmArgs a = SquareGemm(n, g.C, nn, g.W, nn, CW, nn);
    if ((e = LaunchGemm(a, false, false, g.count, st)) != hipSuccess) return e;
    a = SquareGemm(n, g.W, nn, CW, nn, X, nn);
    if ((e = LaunchGemm(a, false, false, g.count, st)) != hipSuccess) return e;
    lmi_dense_c_scalars<<<dim3(f.npart, g.count), 256, 0, st>>>(g, X, f.part);
  }
  const int gb = (int)(((int64_t)m * m + 255) / 256), wb = (m + 1 + 3) / 4;
  if (f.rank_one)
    lmi_factored_finalize<true><<<dim3(gb + wb, g.count), 256, 0, st>>>(g, f, ar, gb);
  else
    lmi_factored_finalize<false><<<dim3(gb + wb, g.count), 256, 0, st>>>(g, f, ar, gb);
  return hipGetLastError();
}

// S of a factored group into ws.tmp, where LmiLargeAfterSlack expects it
inline hipError_t LmiFactoredSlack(const LmiGroup& g, const LmiFactoredGroup& f, const StepArgs& sa, const LmiLargeWs& ws,
                                   hipStream_t st) {
  const int n = g.n, R = f.R;
  const int64_t nn = (int64_t)n * n, nr = (int64_t)n * R;
  double* S = ws.tmp;
  const int blocks = (int)std::min<int64_t>((nn + nr + 255) / 256, 1024);
  lmi_factored_slack<<<dim3(blocks, g.count), 256, 0, st>>>(g, f, sa, S);
  if (R == 0) return hipGetLastError();
  GemmArgs a{};
  a.M = a.N = n, a.K = R;
  a.A = f.Fs, a.lda = n, a.sA1 = nr;
  a.B = f.F, a.ldb = n, a.sB1 = nr;
  a.C = S, a.ldc = n, a.sC1 = nn;
  a.inner = 1;
  a.alpha = 1.0;
  a.beta = 1.0;
  a.splits = 1;
  return LaunchGemm(a, false, true, g.count, st);
}

}  // namespace cxk
