// Streamed quadratic cones whose (n + 1) x m matrix A is held by its nonzeros (cxk_add_quadratic_csr): by rows (CSR,
// columns ascending) for the slack, by columns (CSC, rows ascending) for everything else; row 0 is A0.  The dense A
// never exists, on the host or on the device.  The streamed route reads A in four places; these kernels and two
// arguments replace them, every other kernel of the route serves as it is (quad_stream_qmv or the structured pass,
// _schur_vectors, _prepare_mid / _finish, _take_step):
//   columns  v = A' (W0, Q w1) per assembly, and u = A1' Q c1 ONCE at cxk_finalize (the same kernel on (0, Q c1); the
//            dense form recomputes that constant on every assembly): quad_sparse_columns, one wavefront per column.
//   finish   quad_stream_schur_finish takes A0 as a pointer and a stride; such a group keeps row 0 as a dense
//            count x m vector (stride 1).
//   slack    soc_sparse_slack as it is, on a SocSparseGroup view whose ms is this group's (cone_soc.hip).
//   Gram     A_gram = A1' Q A1 once at cxk_finalize, in panels of P columns (cone_route.h: QuadGramPanelCols):
//            quad_sparse_scatter writes the panel's columns into a zeroed buffer that has the dense form's layout
//            ((n + 1) x P per cone), so that the code that forms T = Q A1 for a dense A forms T = Q panel unchanged;
//            quad_sparse_gather makes A_gram[i, j] = sum over the entries k of column i of a_ki T[r_k, j].
//            Work space 2 count n P doubles (and count P for the panel's row 0), whatever m is.  The factors' F' A1
//            (rank x m) is the same gather on T = F, once and outside the panels: nnz rank multiply-adds.
//
// Members of a group have equal (n, m) but their own patterns: `eptr` gives each member's first nonzero in the group's
// arrays, colptr is relative to it (NonzeroLists, as kernels_soc_sparse.hip.h reads them).
//
// The route's discipline holds: 256-thread workgroups, no atomics, no workgroup waits for another, and every sum is a
// lane's fma chain over every 64th entry of a column in ascending row followed by WaveSum (a fixed butterfly): the
// order depends on the pattern and the launch shape only, same bits every run.  No LDS, no scratch.
#pragma once
#include "kernels_quad_structured.hip.h"  // (quad_struct_sa forms S panel; on top of kernels_quad_stream.hip.h)

namespace cxk {

constexpr int kQuadSparseBlock = 256;  // threads of every kernel here: four wavefronts, one column each

struct QuadSparseGroup {
  int n, m, count;
  const int* eptr;     // count + 1        first nonzero of each member
  const int* colptr;   // count x (m + 1)
  const int* crow;     // by columns, rows ascending within a column; row 0 is A0, row r > 0 is row r - 1 of A1
  const double* cval;
};

// ---- out_j = A0_j x0 + A1[:, j] . x1 for every column j of every cone: x0 of cone `mem` is x0[mem * x0_stride] (0
// when x0 is null), its x1 starts at x1 + mem * n.  One wavefront per column.
__global__ void __launch_bounds__(kQuadSparseBlock) quad_sparse_columns(QuadSparseGroup s, const double* x0, size_t x0_stride,
                                                                        const double* x1, double* out) {
  const int n = s.n, m = s.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t cj = (size_t)blockIdx.x * (kQuadSparseBlock / 64) + wave;
  if (cj >= (size_t)s.count * m) return;  // (whole wavefronts: nothing below waits for another)
  const int j = (int)(cj % m);
  const size_t mem = cj / m;
  const size_t base = (size_t)s.eptr[mem];
  const int* colptr = s.colptr + mem * ((size_t)m + 1);
  const int* crow = s.crow + base;
  const double* cval = s.cval + base;
  const double h0 = x0 ? x0[mem * x0_stride] : 0.0;
  const double* x = x1 + mem * n;
  const int e1 = colptr[j + 1];
  double acc = 0;
  for (int e = colptr[j] + lane; e < e1; e += 64) {
    const int r = crow[e];
    const double xr = x[r > 0 ? r - 1 : 0];
    acc = fma(cval[e], r > 0 ? xr : h0, acc);
  }
  acc = WaveSum(acc);
  if (lane == 0) out[mem * m + j] = acc;
}

// ---- once per panel, at cxk_finalize: columns j0 .. j0 + pw - 1 of every cone into `panel` (count x P columns of
// n + 1 rows, zeroed before the launch; row 0 takes A0, which nobody reads).  One wavefront per column of the panel.
__global__ void __launch_bounds__(kQuadSparseBlock) quad_sparse_scatter(QuadSparseGroup s, double* panel, int j0, int pw, int P) {
  const int len = s.n + 1, m = s.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t cj = (size_t)blockIdx.x * (kQuadSparseBlock / 64) + wave;
  if (cj >= (size_t)s.count * pw) return;
  const int jj = (int)(cj % pw);
  const size_t mem = cj / pw;
  const size_t base = (size_t)s.eptr[mem];
  const int* colptr = s.colptr + mem * ((size_t)m + 1);
  const int* crow = s.crow + base;
  const double* cval = s.cval + base;
  double* col = panel + (mem * P + jj) * (size_t)len;
  const int e1 = colptr[j0 + jj + 1];
  for (int e = colptr[j0 + jj] + lane; e < e1; e += 64) col[crow[e]] = cval[e];  // (a column's rows are distinct)
}

// ---- out[i, jj] = sum over the entries k of column i of A1 of a_ki T[r_k, jj], jj < pw: A1' T for a T of n rows and pw
// columns per cone (column jj of cone `mem` starts at T + mem * t_stride + jj * ldt), written to
// out[mem * out_stride + i * out_i + jj * out_j].  Once per panel with T = Q panel and `out` the panel's columns of
// A_gram; once per group with T = F, which makes F' A1.  One wavefront per column i of a cone, across the pw columns.
__global__ void __launch_bounds__(kQuadSparseBlock) quad_sparse_gather(QuadSparseGroup s, const double* T, size_t ldt, size_t t_stride,
                                                                       int pw, double* out, size_t out_stride, size_t out_i, size_t out_j) {
  const int m = s.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t ci = (size_t)blockIdx.x * (kQuadSparseBlock / 64) + wave;
  if (ci >= (size_t)s.count * m) return;
  const int i = (int)(ci % m);
  const size_t mem = ci / m;
  const size_t base = (size_t)s.eptr[mem];
  const int* colptr = s.colptr + mem * ((size_t)m + 1);
  const int* crow = s.crow + base;
  const double* cval = s.cval + base;
  const int e0 = colptr[i], e1 = colptr[i + 1];
  double* o = out + mem * out_stride + i * out_i;
  for (int jj = 0; jj < pw; jj++) {  // (pw is the launch's: every lane of the wavefront makes every trip)
    const double* t = T + mem * t_stride + (size_t)jj * ldt;
    double acc = 0;
    for (int e = e0 + lane; e < e1; e += 64) {
      const int r = crow[e];
      const double tr = t[r > 0 ? r - 1 : 0];
      acc = fma(cval[e], r > 0 ? tr : 0.0, acc);
    }
    acc = WaveSum(acc);
    if (lane == 0) o[jj * out_j] = acc;
  }
}

}  // namespace cxk
