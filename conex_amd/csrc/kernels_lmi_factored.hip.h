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
//
// Hermitian A_i = sum sigma_k f_k f_k^* over R / C / H (cxk_add_hermitian_factored, d = 1 / 2 / 4 planes) in the real
// representation L(.) of order N = d n: L(f f^*) = L(f) L(f)^T, and the group holds L(F) (N x dR, column block p of R
// columns = L_p; L_0 = F0 is the stacked planes of F).  Only F0 passes through W and C:
//   Z = W F0, Y = C Z (N x R),  P_p = L_p^T Z (d planes of R x R, one GEMM of dR x R x N; P_0 symmetric, the others skew)
//   G(i,j) = sum sigma_k sigma_l sum_p P_p(k,l)^2,  AW(i) = sum sigma_k P_0(k,k),  AQc(i) = sum sigma_k z_k^T y_k
//   S      = L(F) diag(sigma_k y_i(k), once per column block) L(F)^T - k L(C): its first n columns from the GEMM, the other
//            d - 1 block columns filled from them (lmi_factored_herm_fill), so that S is exactly a real representation
// every contraction being tr / d of the real representation's (cxk_add_hermitian's scaling).  These hold for a W that
// is a real representation; the assembly makes it one first (lmi_factored_herm_project).
#pragma once
#include "kernels_lmi_large.hip.h"
#include "kernels_lmi_sparse.hip.h"

namespace cxk {

struct LmiFactoredGroup {
  int R;                // columns of F per member
  int d;                // 1: real symmetric or Hermitian over R; 2 / 4: Hermitian over C / H, F is L(F) (n x dR, n = d x order)
  int rank_one;         // every A_i of every member has exactly one column (R == m, column i is A_i's)
  const double* F;      // count x (n x dR), column-major
  const double* sigma;  // count x R
  const int* ptr;       // count x (m + 1): columns of A_i
  const int* var;       // count x R: column -> its variable
  double* Z;            // count x (n x R)   W F0
  double* Y;            // count x (n x R)   C Z
  double* Fs;           // count x (n x dR)  F diag(sigma_k y_i(k))  (slack)
  double* P;            // count x (dR x R)  F^T Z: d planes of R x R; d = 1: the lower triangle only
  double* part;         // count x npart x 2 partial sums of <w,c>, <c,Qc>
  int npart;
};

// G (lower triangle), AW, AQc and the two scalars into the arena.  grid (gb + wb, count): the first
// gb = ceil(m^2 / 256) workgroups give a thread to every (i, j) of G; behind them a wavefront per variable
// forms AQc(i) and AW(i), and one more adds the partial sums of the scalars.  Only P(k, l) with k >= l is read
// (P(k, l) and P(l, k) are different sums of the GEMM).  RANK1: G(i, j) = sigma_i sigma_j P_ij^2, no block sums.
// D planes (f.d): P_kl^2 is the sum of the D plane squares, plane 0 first (the transposed entry of a skew plane has
// the same square); D = 1 is the real form, term by term as it has always been.
template <int D, bool RANK1>
__global__ void __launch_bounds__(256) lmi_factored_finalize(LmiGroup g, LmiFactoredGroup f, Arena ar, int gb) {
  const int n = g.n, m = g.m, R = f.R;
  const int mem = blockIdx.y, id = g.ids[mem];
  const size_t ldp = (size_t)D * R;  // plane q of P(k, l) is q * R further on
  const double* P = f.P + (size_t)mem * ldp * R;
  auto planes_sq = [P, R, ldp](int k, int l) {  // sum_q P_q(k, l)^2, k >= l
    const double* p = P + k + (size_t)l * ldp;
    double s = p[0] * p[0];
    for (int q = 1; q < D; q++) s = fma(p[(size_t)q * R], p[(size_t)q * R], s);
    return s;
  };
  const double* sg = f.sigma + (size_t)mem * R;
  const int* ptr = f.ptr + (size_t)mem * (m + 1);
  if ((int)blockIdx.x < gb) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)m * m) return;
    const int i = (int)(e % m), j = (int)(e / m);
    if (i < j) return;
    double acc = 0.0;
    if constexpr (RANK1) {
      acc = planes_sq(i, j) * (sg[i] * sg[j]);
    } else if constexpr (D > 1) {
      const int k0 = ptr[i], k1 = ptr[i + 1], l0 = ptr[j], l1 = ptr[j + 1];
      for (int k = k0; k < k1; k++) {
        double row = 0.0;
        for (int l = l0; l < l1; l++) row = fma(sg[l], k >= l ? planes_sq(k, l) : planes_sq(l, k), row);
        acc = fma(sg[k], row, acc);
      }
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
      aw = fma(sg[k], P[k + (size_t)k * ldp], aw);
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
    if (lane == 0) {  // (tr / D of the real representation: exact, a power of two)
      ar.sc[2 * id] = D > 1 ? wc * (1.0 / D) : wc;
      ar.sc[2 * id + 1] = D > 1 ? cq * (1.0 / D) : cq;
    }
  }
}

// S = -k C and Fs = F diag(sigma_k y_i(k)); grid (blocks over n^2 + n dR, count).  The GEMM behind it adds Fs F^T.
// (Column block p of L(F) repeats the columns of F0: column c of F is column c % R's sigma and variable.)
__global__ void __launch_bounds__(256) lmi_factored_slack(LmiGroup g, LmiFactoredGroup f, StepArgs sa, double* __restrict__ S) {
  const int n = g.n, R = f.R;
  const int mem = blockIdx.y, id = g.ids[mem];
  const int64_t nn = (int64_t)n * n, nr = (int64_t)n * R * f.d;
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
      const int k = (int)(e / n) % R;
      Fs[e] = F[e] * (sg[k] * sa.y[sa.cl_perm[cl0 + var[k]]]);
    }
  }
}

// Hermitian slack (d > 1) behind the first-columns product: T (n x n0, n0 = n / d) is block column 0 of Fs F^T, plane p
// in its rows [p n0, (p + 1) n0).  S += L(herm(T)): block (k, j) = sign[k ^ j][j] x plane k ^ j (kkt_context.hip,
// EmbedPlanes), the planes made exactly Hermitian, (T_0 + T_0^T) / 2 and (T_p - T_p^T) / 2.  S is then exactly a real
// representation, as the slack of the dense Hermitian route is: the d^2 blocks of the full product are different sums
// of the GEMM, and what they differ by is no perturbation of the program's data.  grid (blocks over n^2, count).
__global__ void __launch_bounds__(256) lmi_factored_herm_fill(int n, int d, const double* __restrict__ T, double* __restrict__ S) {
  constexpr int kSign[4][4] = {{1, 1, 1, 1}, {1, -1, -1, 1}, {1, 1, -1, -1}, {1, -1, 1, -1}};
  const int n0 = n / d, mem = blockIdx.y;
  const int64_t nn = (int64_t)n * n;
  const double* Tm = T + (size_t)mem * n * n0;
  double* Sm = S + (size_t)mem * nn;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nn; q += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(q % n), col = (int)(q / n);
    const int k = row / n0, r = row - k * n0, j = col / n0, c = col - j * n0, p = k ^ j;
    const double a = Tm[p * n0 + r + (size_t)c * n], b = Tm[p * n0 + c + (size_t)r * n];
    const double v = 0.5 * (p == 0 ? a + b : a - b);
    Sm[q] += kSign[p][j] < 0 ? -v : v;
  }
}

// W <- the real representation nearest to it (d > 1), in place: plane p = the mean over j of sign[p][j] x block
// (p ^ j, j), written back to those d blocks.  TakeStep's products leave W a real representation only to rounding (its
// d^2 blocks are different sums of the GEMM).  The folded assembly reads W through the first column block of L(F)
// alone, and what it forms is the Schur complement of the iteration's W only if W is a real representation exactly;
// the mean of d equal numbers is exact, so a W that is one (cxk_set_W, cxk_set_identity) keeps its bits.
// grid (blocks over n^2 / d, count).
__global__ void __launch_bounds__(256) lmi_factored_herm_project(int n, int d, double* __restrict__ W) {
  constexpr int kSign[4][4] = {{1, 1, 1, 1}, {1, -1, -1, 1}, {1, 1, -1, -1}, {1, -1, 1, -1}};
  const int n0 = n / d, mem = blockIdx.y;
  double* Wm = W + (size_t)mem * n * n;
  const int64_t per = (int64_t)n0 * n0, total = per * d;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(q / per), e = (int)(q - p * per), r = e % n0, c = e / n0;
    double sum = 0.0;
    for (int j = 0; j < d; j++) {
      const double v = Wm[(size_t)(j * n0 + c) * n + (p ^ j) * n0 + r];
      sum += kSign[p][j] < 0 ? -v : v;
    }
    const double x = sum * (1.0 / d);
    for (int j = 0; j < d; j++) Wm[(size_t)(j * n0 + c) * n + (p ^ j) * n0 + r] = kSign[p][j] < 0 ? -x : x;
  }
}

// ---- host-side drivers --------------------------------------------------------------------
inline hipError_t LmiFactoredSchur(const LmiGroup& g, const LmiFactoredGroup& f, const Arena& ar, const LmiLargeWs& ws,
                                   hipStream_t st) {
  const int n = g.n, m = g.m, R = f.R, d = f.d;
  const int64_t nn = (int64_t)n * n, nr = (int64_t)n * R, nf = nr * d;  // (nf: a member's F, d column blocks)
  hipError_t e;
  if (d > 1) lmi_factored_herm_project<<<ElemGrid(n, g.count), 256, 0, st>>>(n, d, g.W);
  if (R > 0) {
    GemmArgs a{};
    a.inner = 1;
    a.alpha = 1.0;
    a.beta = 0.0;
    a.splits = 1;
    // Z = W F (d > 1: F0, the first R columns of L(F))
    a.M = n, a.N = R, a.K = n;
    a.A = g.W, a.lda = n, a.sA1 = nn;
    a.B = f.F, a.ldb = n, a.sB1 = nf;
    a.C = f.Z, a.ldc = n, a.sC1 = nr;
    if ((e = LaunchGemm(a, false, false, g.count, st)) != hipSuccess) return e;
    // Y = C Z
    a.A = g.C;
    a.B = f.Z, a.sB1 = nr;
    a.C = f.Y;
    if ((e = LaunchGemm(a, false, false, g.count, st)) != hipSuccess) return e;
    // P = F^T Z: the lower triangle (d = 1), or the d planes of R x R below each other in one dR x R product
    a.M = d * R, a.N = R, a.K = n;
    a.A = f.F, a.lda = n, a.sA1 = nf;
    a.B = f.Z, a.ldb = n, a.sB1 = nr;
    a.C = f.P, a.ldc = (int64_t)d * R, a.sC1 = (int64_t)d * R * R;
    a.lower_only = d == 1;
    if ((e = LaunchGemm(a, true, false, g.count, st)) != hipSuccess) return e;
  }
  {  // X = W (C W), then the slices of <C, W> and <C, X> (the finalize kernel adds them and takes tr / d)
    double* CW = ws.tmp;
    double* X = ws.tmp + (size_t)g.count * nn;
    GemmArgs a = SquareGemm(n, g.C, nn, g.W, nn, CW, nn);
    if ((e = LaunchGemm(a, false, false, g.count, st)) != hipSuccess) return e;
    a = SquareGemm(n, g.W, nn, CW, nn, X, nn);
    if ((e = LaunchGemm(a, false, false, g.count, st)) != hipSuccess) return e;
    lmi_dense_c_scalars<<<dim3(f.npart, g.count), 256, 0, st>>>(g, X, f.part);
  }
  const int gb = (int)(((int64_t)m * m + 255) / 256), wb = (m + 1 + 3) / 4;
  const dim3 grid(gb + wb, g.count);
  switch (2 * d + (f.rank_one ? 1 : 0)) {
    case 2: lmi_factored_finalize<1, false><<<grid, 256, 0, st>>>(g, f, ar, gb); break;
    case 3: lmi_factored_finalize<1, true><<<grid, 256, 0, st>>>(g, f, ar, gb); break;
    case 4: lmi_factored_finalize<2, false><<<grid, 256, 0, st>>>(g, f, ar, gb); break;
    case 5: lmi_factored_finalize<2, true><<<grid, 256, 0, st>>>(g, f, ar, gb); break;
    case 8: lmi_factored_finalize<4, false><<<grid, 256, 0, st>>>(g, f, ar, gb); break;
    case 9: lmi_factored_finalize<4, true><<<grid, 256, 0, st>>>(g, f, ar, gb); break;
    default: return hipErrorInvalidValue;  // (cxk_add_hermitian_factored admits d = 1, 2, 4)
  }
  return hipGetLastError();
}

// S of a factored group into ws.tmp, where LmiLargeAfterSlack expects it
inline hipError_t LmiFactoredSlack(const LmiGroup& g, const LmiFactoredGroup& f, const StepArgs& sa, const LmiLargeWs& ws,
                                   hipStream_t st) {
  const int n = g.n, R = f.R, d = f.d;
  const int64_t nn = (int64_t)n * n, nf = (int64_t)n * R * d;
  double* S = ws.tmp;
  const int blocks = (int)std::min<int64_t>((nn + nf + 255) / 256, 1024);
  lmi_factored_slack<<<dim3(blocks, g.count), 256, 0, st>>>(g, f, sa, S);
  if (R == 0) return hipGetLastError();
  GemmArgs a{};
  a.M = a.N = n, a.K = d * R;
  a.A = f.Fs, a.lda = n, a.sA1 = nf;
  a.B = f.F, a.ldb = n, a.sB1 = nf;
  a.C = S, a.ldc = n, a.sC1 = nn;
  a.inner = 1;
  a.alpha = 1.0;
  a.beta = 1.0;
  a.splits = 1;
  if (d == 1) return LaunchGemm(a, false, true, g.count, st);
  // d > 1: the first n / d columns of Fs F^T alone (1 / d of the product), into the step temporaries behind S and WS
  // (LmiLargeAfterSlack's T, written after this), then the fill
  double* T = ws.tmp + 2 * (size_t)g.count * nn;
  a.N = n / d;
  a.C = T, a.sC1 = (int64_t)n * (n / d);
  a.beta = 0.0;
  const hipError_t e = LaunchGemm(a, false, true, g.count, st);
  if (e != hipSuccess) return e;
  lmi_factored_herm_fill<<<ElemGrid(n, g.count), 256, 0, st>>>(n, d, T, S);
  return hipGetLastError();
}

}  // namespace cxk
