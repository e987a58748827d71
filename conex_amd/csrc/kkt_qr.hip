// kkt_solver = CONEX_QR_FACTORIZATION: the dense KKT matrix factored and solved on the host (host code only).
#include "kkt_launch.h"

namespace cxk_host {

constexpr int kQrMaxOrder = 1500;

// Column-pivoted Householder QR, A P = Q R, of the n x n column-major matrix `a` (overwritten:
// R on and above the diagonal, the essential parts of the reflectors below).  Pivot rule and solve
// are those of Eigen::ColPivHouseholderQR: largest remaining column norm first; solve() works with
// nonzeroPivots() -- NOT rank(): the factorization stops counting pivots at the first step k whose
// largest remaining squared column norm is below (eps * largest initial column norm)^2 / n * (n - k)
// -- applies that many reflectors, solves with the leading triangle of that size and leaves the
// remaining unknowns zero.  `rank` returns that count.
void DenseQrFactor(int n, std::vector<double>& a, std::vector<double>& tau, std::vector<int>& piv, int* rank) {
  tau.assign(n, 0.0);
  piv.resize(n);
  std::vector<double> norm2(n);
  for (int j = 0; j < n; j++) {
    piv[j] = j;
    double t = 0;
    for (int i = 0; i < n; i++) t += a[i + (size_t)j * n] * a[i + (size_t)j * n];
    norm2[j] = t;
  }
  double maxnorm2 = 0;
  for (int j = 0; j < n; j++) maxnorm2 = std::max(maxnorm2, norm2[j]);
  const double threshold_helper = maxnorm2 * DBL_EPSILON * DBL_EPSILON / n;  // abs2(max col norm * eps) / rows
  int nonzero = n;
  for (int k = 0; k < n; k++) {
    int best = k;
    for (int j = k; j < n; j++) {  // column norms of the trailing block, recomputed (n is small)
      double t = 0;
      for (int i = k; i < n; i++) t += a[i + (size_t)j * n] * a[i + (size_t)j * n];
      norm2[j] = t;
      if (t > norm2[best]) best = j;
    }
    if (nonzero == n && norm2[best] < threshold_helper * (n - k)) nonzero = k;
    if (best != k) {
      for (int i = 0; i < n; i++) std::swap(a[i + (size_t)k * n], a[i + (size_t)best * n]);
      std::swap(piv[k], piv[best]);
      std::swap(norm2[k], norm2[best]);
    }
    double* col = &a[(size_t)k * n];
    const double alpha = col[k];
    double tail = 0;
    for (int i = k + 1; i < n; i++) tail += col[i] * col[i];
    double beta = alpha;
    if (tail > 0) {
      beta = std::sqrt(alpha * alpha + tail);
      if (alpha >= 0) beta = -beta;
      tau[k] = (beta - alpha) / beta;
      const double scale = 1.0 / (alpha - beta);
      for (int i = k + 1; i < n; i++) col[i] *= scale;
      col[k] = beta;
      for (int j = k + 1; j < n; j++) {  // apply H_k = I - tau v v^T, v = [1; col[k+1:]]
        double* cj = &a[(size_t)j * n];
        double w = cj[k];
        for (int i = k + 1; i < n; i++) w += col[i] * cj[i];
        w *= tau[k];
        cj[k] -= w;
        for (int i = k + 1; i < n; i++) cj[i] -= w * col[i];
      }
    }
  }
  *rank = nonzero;
}

void DenseQrSolve(const cxk_context::DenseQr& Q, std::vector<double>& b) {
  const int n = Q.n;
  const std::vector<double>& a = Q.qr;
  for (int k = 0; k < Q.rank; k++) {  // c = Q^T b, the first nonzeroPivots() reflectors (householderQ().setLength)
    if (Q.tau[k] == 0.0) continue;
    double w = b[k];
    for (int i = k + 1; i < n; i++) w += a[i + (size_t)k * n] * b[i];
    w *= Q.tau[k];
    b[k] -= w;
    for (int i = k + 1; i < n; i++) b[i] -= w * a[i + (size_t)k * n];
  }
  std::vector<double> z(n, 0.0);
  for (int k = Q.rank - 1; k >= 0; k--) {
    double t = b[k];
    for (int j = k + 1; j < Q.rank; j++) t -= a[k + (size_t)j * n] * z[j];
    z[k] = t / a[k + (size_t)k * n];
  }
  for (int k = 0; k < n; k++) b[Q.piv[k]] = z[k];
}

// Factor(): kkt_matrix_ = KKTMatrix() = Pt G Pt^T from the assembled slab (kkt_solver.cc:175-178,
// 265-269; supernodal_solver.cc:117-137 ToDense), qr_decomp_.compute(kkt_matrix_) (:196).
int QrFactor(cxk_context* ctx) {
  const Layout& L = ctx->lay;
  const int N = ctx->md.N;
  CXK_DEMAND(N <= kQrMaxOrder, "kkt_solver = QR factors the dense N x N KKT matrix on one host core: N exceeds the limit (1500)");
  CXK_DEMAND(ctx->world == 1, "the QR solver mode is single-GPU");
  std::vector<double> slab((size_t)L.slab_size);
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(slab.data(), ctx->slab.p, sizeof(double) * slab.size(), hipMemcpyDeviceToHost));
  std::vector<double> G((size_t)N * N, 0.0);  // permuted order, then both triangles
  for (int e = 0; e < L.K; e++) {
    const int ns = L.supernode_size[e], st = L.supernode_start[e];
    for (int j = 0; j < ns; j++)
      for (int i = j; i < ns; i++) G[(size_t)(st + i) + (size_t)(st + j) * N] = slab[L.diag_off[e] + i + (int64_t)j * ns];
    for (size_t c = 0; c < L.separators[e].size(); c++)
      for (int i = 0; i < ns; i++) G[(size_t)L.separators[e][c] + (size_t)(st + i) * N] = slab[L.offd_off[e] + i + (int64_t)c * ns];
  }
  auto& Q = ctx->qr;
  Q.n = N;
  Q.qr.assign((size_t)N * N, 0.0);
  const std::vector<int>& pinv = ctx->md.permutation_inverse;  // permuted position -> original variable
  for (int j = 0; j < N; j++)
    for (int i = j; i < N; i++) {
      const double v = G[(size_t)i + (size_t)j * N];
      Q.qr[(size_t)pinv[i] + (size_t)pinv[j] * N] = v;
      Q.qr[(size_t)pinv[j] + (size_t)pinv[i] * N] = v;
    }
  DenseQrFactor(N, Q.qr, Q.tau, Q.piv, &Q.rank);
  Q.valid = true;
  CXK_TRY(hipMemsetAsync(ctx->d_fail.p, 0, sizeof(int), ctx->stream));  // Factor() returns true (:197)
  ctx->fail_tag = 0;
  return CXK_SUCCESS;
}

// SolveInPlace with the QR (kkt_solver.cc:227-231): the device's right-hand side is in permuted
// order, the factorization in the original one.
int QrSolve(cxk_context* ctx) {
  CXK_DEMAND(ctx->qr.valid, "QR solve before a QR factorization");
  const int N = ctx->md.N;
  std::vector<double> yp(N), y(N);
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(yp.data(), ctx->y.p, sizeof(double) * N, hipMemcpyDeviceToHost));
  for (int i = 0; i < N; i++) y[ctx->md.permutation_inverse[i]] = yp[i];
  DenseQrSolve(ctx->qr, y);
  for (int i = 0; i < N; i++) yp[i] = y[ctx->md.permutation_inverse[i]];
  CXK_TRY(hipMemcpy(ctx->y.p, yp.data(), sizeof(double) * N, hipMemcpyHostToDevice));
  return CXK_SUCCESS;
}

}  // namespace cxk_host
