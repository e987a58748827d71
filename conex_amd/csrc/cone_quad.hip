// Quadratic cones on their two routes (kQuadLds, kQuadStreamed): the views, the stages of cxk_finalize and every
// launch.  Owns the kernels of kernels_quad / _quad_stream / _quad_structured / _quad_sparse; the streamed route's slack is the second-order
// cones' kernel (cone_soc.hip: LaunchSocStreamSlack, LaunchSocSparseSlack), the scaling point's identity the vector cones' (cone_linear.hip).
// The family's state is Group::quad (cone_state.h).
#include "cone_units.h"
#include "kernels_gemm.hip.h"
#include "kernels_quad.hip.h"
#include "kernels_quad_sparse.hip.h"  // (on top of kernels_quad_structured.hip.h and kernels_quad_stream.hip.h, which it includes)

namespace cxk_host {

// ---- The views the kernels take of a group, each beside the stage of cxk_finalize that allocates what it lays out,
// so that a layout and its size are read together.  What those stages call further down:
int QuadStreamConstants(cxk_context* ctx, Group& g);

QuadGroup MakeQuad(Group& g) {
  QuadGroup d;
  d.n = g.n;
  d.m = g.m;
  d.count = static_cast<int>(g.ids.size());
  d.A = g.A.p;
  d.c = g.C.p;
  d.Q = g.quad.has_q ? g.quad.Q.p : nullptr;
  d.Agram = g.quad.Gram.p;
  d.W = g.W.p;
  d.D = g.T1.p;
  d.S = g.quad.S.p;
  d.ids = g.dids.p;
  return d;
}
// A_gram = A1' (Q A1) of a group of quadratic cones on the LDS route, made once on the host
// (QuadraticConstraintBase::Initialize, quadratic_cone_constraint.cc:216-219), Q, and the state S.
int UploadQuadGram(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size();
  const int n = g.n, m = g.m, len = n + 1;
  std::vector<double> hQ(g.quad.has_q ? (size_t)n * n * cnt : 0), hG((size_t)m * m * cnt, 0.0), qa((size_t)n);
  for (size_t k = 0; k < cnt; k++) {
    const ConstraintRec& c = ctx->cons[g.ids[k]];
    if (g.quad.has_q) std::copy(c.Q.begin(), c.Q.end(), hQ.begin() + k * (size_t)n * n);
    for (int j = 0; j < m; j++) {
      const double* aj = c.A.data() + (size_t)j * len + 1;
      for (int i = 0; i < n; i++) {
        double s2 = g.quad.has_q ? 0.0 : aj[i];
        if (g.quad.has_q)
          for (int q2 = 0; q2 < n; q2++) s2 += c.Q[(size_t)q2 * n + i] * aj[q2];
        qa[(size_t)i] = s2;
      }
      for (int i = 0; i < m; i++) {
        const double* ai = c.A.data() + (size_t)i * len + 1;
        double s2 = 0;
        for (int q2 = 0; q2 < n; q2++) s2 += ai[q2] * qa[(size_t)q2];
        hG[k * (size_t)m * m + (size_t)j * m + i] = s2;
      }
    }
  }
  CXK_TRY(g.quad.Q.upload(hQ));
  CXK_TRY(g.quad.Gram.upload(hG));
  CXK_TRY(g.quad.S.alloc((size_t)len * cnt));
  return CXK_SUCCESS;
}
QuadStreamGroup MakeQuadStream(Group& g) {
  QuadStreamGroup d;
  const size_t cnt = g.ids.size(), n = (size_t)g.n, m = (size_t)g.m;
  d.n = g.n;
  d.m = g.m;
  d.count = static_cast<int>(cnt);
  d.splits = g.quad.splits;
  d.q_form = g.quad.sq.on ? kQuadQStructured : g.quad.has_q ? kQuadQDense : kQuadQIdentity;  // (structured: Q.p is null)
  d.A = g.A.p;
  d.c = g.C.p;
  d.Q = g.quad.has_q ? g.quad.Q.p : nullptr;
  d.Agram = g.quad.Gram.p;
  d.W = g.W.p;
  d.D = g.T1.p;
  d.S = g.quad.S.p;
  d.ids = g.dids.p;
  d.part = g.quad.part.p;
  double* p = g.quad.vec.p;  // (the layout UploadQuadStream sizes: QuadStreamVecDoubles)
  d.qc1 = p;
  d.qw = (p += cnt * n);
  d.dv = (p += cnt * n);
  d.qd = (p += cnt * n);
  d.ms = (p += cnt * n);
  d.v = (p += cnt * (n + 1));
  d.u = (p += cnt * m);
  d.scal = (p += cnt * m);
  d.cqc = (p += cnt * 8);
  return d;
}
size_t QuadStreamVecDoubles(size_t cnt, size_t n, size_t m) { return cnt * (4 * n + (n + 1) + 2 * m + 8 + 1); }
// A group of streamed quadratic cones with a dense Q or none: Q as it is, the work space, the constants (QuadStreamConstants).
int UploadQuadStream(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size();
  const size_t n = (size_t)g.n, m = (size_t)g.m, tiles = (n + kQuadStreamRowTile - 1) / kQuadStreamRowTile;
  g.quad.splits = g.quad.has_q ? QuadStreamSplits(g.n, (long long)cnt) : 1;
  if (g.quad.has_q && sw.gram_splits > 0) g.quad.splits = sw.gram_splits;  // (comparison runs)
  CXK_DEMAND(cnt * std::max<size_t>(std::max<size_t>(m, (m * m + kQuadStreamBlock - 1) / kQuadStreamBlock),
                                    std::max<size_t>(tiles * (size_t)g.quad.splits, (n + 1 + kSocStreamRowTile - 1) / kSocStreamRowTile)) <=
                 (size_t)INT_MAX,
             "a group of streamed quadratic cones with more than 2^31 columns, row tiles or blocks is not supported");
  std::vector<double> hQ(g.quad.has_q ? n * n * cnt : 0);
  if (g.quad.has_q)
    for (size_t k = 0; k < cnt; k++) std::copy(ctx->cons[g.ids[k]].Q.begin(), ctx->cons[g.ids[k]].Q.end(), hQ.begin() + k * n * n);
  CXK_TRY(g.quad.Q.upload(hQ));
  CXK_TRY(g.quad.Gram.alloc(m * m * cnt));
  CXK_TRY(g.quad.S.alloc((n + 1) * cnt));
  CXK_TRY(g.quad.vec.alloc(QuadStreamVecDoubles(cnt, n, m)));
  CXK_TRY(g.quad.part.alloc(g.quad.has_q ? cnt * (size_t)g.quad.splits * 2 * n : 0));
  return g.quad.sa.on ? QuadSparseConstants(ctx, g) : QuadStreamConstants(ctx, g);
}
// soc_stream_slack serves the streamed quadratic cone as it is (same layout, same formula): what it reads of the group.
SocStreamGroup QuadStreamSlackView(Group& g, const QuadStreamGroup& d) {
  SocStreamGroup s{};
  s.v = MakeVec(g);
  s.ms = d.ms;
  return s;
}

// Kernels of this unit that may be launched with more than the default 64 KB of dynamic LDS.
hipError_t RaiseQuadLdsLimits() {
  return RaiseDynamicLds({
    reinterpret_cast<const void*>(&quad_schur),
    reinterpret_cast<const void*>(&quad_prepare<0>),
    reinterpret_cast<const void*>(&quad_prepare<1>),
    reinterpret_cast<const void*>(&quad_take_step),
  });
}

// One pass over Q of a group of streamed quadratic cones: out_r = Q x_r for the R vectors of `x` (partials per
// column split; QuadStreamQx adds them).  Nothing to do where Q is the identity; its parts' own pass where Q is held by them.
template <int R>
hipError_t LaunchQuadStreamQmv(Group& g, const QuadStreamGroup& d, const QuadStreamVecs& x, hipStream_t st) {
  if (d.q_form != kQuadQDense) return d.q_form == kQuadQIdentity ? hipSuccess : LaunchQuadStructuredQmv<R>(g, d, x, st);
  const int tiles = (d.n + kQuadStreamRowTile - 1) / kQuadStreamRowTile;
  quad_stream_qmv<R><<<(unsigned)((size_t)d.count * tiles * d.splits), kQuadStreamBlock, 0, st>>>(d, x, tiles);
  return hipGetLastError();
}
QuadStreamVecs QuadStreamOne(const double* p, size_t stride) {
  QuadStreamVecs x;
  x.p[0] = x.p[1] = p;
  x.stride[0] = x.stride[1] = stride;
  return x;
}

// The Schur complement of a group of quadratic cones on the LDS route: one workgroup per cone.
void LaunchQuadLdsSchur(Group& g, const Arena& ar, hipStream_t st) {
  quad_schur<<<(int)g.ids.size(), 64, QuadSchurLds(g.n, g.m), st>>>(MakeQuad(g), ar);
}

// The Schur complement of a group of streamed quadratic cones: Q w1, the scalars, the columns, the block.
hipError_t LaunchQuadStreamSchur(Group& g, const Arena& ar, hipStream_t st) {
  const QuadStreamGroup d = MakeQuadStream(g);
  const int cnt = d.count, m = d.m, a0s = g.quad.sa.on ? 1 : d.n + 1;  // (row 0 of A: dense count x m with a sparse A)
  hipError_t e = LaunchQuadStreamQmv<1>(g, d, QuadStreamOne(d.W + 1, (size_t)d.n + 1), st);
  if (e != hipSuccess) return e;
  quad_stream_schur_vectors<<<cnt, kQuadStreamBlock, 0, st>>>(d);
  if (m > 0) LaunchQuadSchurColumns(g, d, st);
  const int blocks = (int)std::max<size_t>(1, ((size_t)m * m + kQuadStreamBlock - 1) / kQuadStreamBlock);
  quad_stream_schur_finish<<<(unsigned)((size_t)cnt * blocks), kQuadStreamBlock, 0, st>>>(d, ar, blocks, g.quad.sa.on ? g.quad.sa.a0.p : d.A, a0s);
  return hipGetLastError();
}

// The constants of a group of streamed quadratic cones, once at cxk_finalize, on the device: Qc1 = Q c1 and
// c1' Q c1 by the pass kernel, A_gram = A1' (Q A1) as two batched GEMMs (A1 = A + 1 with leading dimension
// n + 1; T = Q A1 in a buffer that lives for this call only).
int QuadStreamConstants(cxk_context* ctx, Group& g) {
  const QuadStreamGroup d = MakeQuadStream(g);
  const int cnt = d.count, n = d.n, m = d.m, len = n + 1;
  CXK_TRY(LaunchQuadStreamQmv<1>(g, d, QuadStreamOne(d.c + 1, (size_t)len), ctx->stream));
  quad_stream_constants<<<cnt, kQuadStreamBlock, 0, ctx->stream>>>(d);
  CXK_TRY(hipGetLastError());
  DevBuf<double> T;
  if (g.quad.has_q && m > 0) CXK_TRY(T.alloc((size_t)cnt * n * m));
  constexpr int kMaxBatch = 65535;  // gridDim.z
  for (int b0 = 0; b0 < cnt && m > 0; b0 += kMaxBatch) {
    const int nb = std::min(kMaxBatch, cnt - b0);
    const double* A1 = g.A.p + (size_t)b0 * len * m + 1;
    GemmArgs a{};
    a.inner = 1;
    a.alpha = 1.0;
    a.beta = 0.0;
    a.splits = 1;
    if (g.quad.has_q) {  // T = Q A1
      a.M = n;
      a.N = m;
      a.K = n;
      a.A = g.quad.Q.p + (size_t)b0 * n * n;
      a.lda = n;
      a.sA1 = (int64_t)n * n;
      a.B = A1;
      a.ldb = len;
      a.sB1 = (int64_t)len * m;
      a.C = T.p + (size_t)b0 * n * m;
      a.ldc = n;
      a.sC1 = (int64_t)n * m;
      CXK_TRY(LaunchGemm(a, false, false, nb, ctx->stream));
    }
    // A_gram = A1' T (A1' A1 where Q is the identity)
    a.M = a.N = m;
    a.K = n;
    a.A = A1;
    a.lda = len;
    a.sA1 = (int64_t)len * m;
    a.B = g.quad.has_q ? T.p + (size_t)b0 * n * m : A1;
    a.ldb = g.quad.has_q ? n : len;
    a.sB1 = g.quad.has_q ? (int64_t)n * m : (int64_t)len * m;
    a.C = g.quad.Gram.p + (size_t)b0 * m * m;
    a.ldc = m;
    a.sC1 = (int64_t)m * m;
    CXK_TRY(LaunchGemm(a, true, false, nb, ctx->stream));
  }
  CXK_TRY(hipStreamSynchronize(ctx->stream));  // (T is released on return)
  return CXK_SUCCESS;
}

// ---- Streamed quadratic cones whose Q = S + F diag(sigma) F' is held by its parts (cxk_add_quadratic_structured; the
// kernels of kernels_quad_structured.hip.h).  Such a group is a streamed group in everything but the two places that
// read Q: the pass (LaunchQuadStreamQmv hands it to LaunchQuadStructuredQmv) and A_gram at finalize.

// What those kernels read of the group (UploadQuadStructured allocates it): the products land in d.part as one split.
QuadStructured MakeQuadStructured(const Group& g, const QuadStreamGroup& d) {
  QuadStructured q;
  q.n = g.n;
  q.count = d.count;
  q.rank = g.quad.sq.rank;
  q.segs = g.quad.sq.segs;
  q.has_s = g.quad.sq.has_s;
  q.rowptr = g.quad.sq.rowptr.p;
  q.col = g.quad.sq.col.p;
  q.val = g.quad.sq.val.p;
  q.F = g.quad.sq.F.p;
  q.sigma = g.quad.sq.sigma.p;
  q.tpart = g.quad.sq.tpart.p;
  q.part = d.part;
  return q;
}
// The pass out_r = Q x_r: the factor dots (rank > 0), then the rows at the group's lanes.
template <int R>
hipError_t LaunchQuadStructuredQmv(Group& g, const QuadStreamGroup& d, const QuadStreamVecs& x, hipStream_t st) {
  const QuadStructured q = MakeQuadStructured(g, d);
  const int tiles = (d.n + kQuadStreamRowTile - 1) / kQuadStreamRowTile;
  const unsigned grid = (unsigned)((size_t)d.count * tiles);
  if (q.rank > 0) quad_struct_dots<R><<<(unsigned)((size_t)d.count * q.rank * q.segs), kQuadStreamBlock, 0, st>>>(q, x);
  switch (g.quad.sq.lanes) {
    case 1: quad_struct_rows<R, 1><<<grid, kQuadStreamBlock, 0, st>>>(q, x, tiles); break;
    case 8: quad_struct_rows<R, 8><<<grid, kQuadStreamBlock, 0, st>>>(q, x, tiles); break;
    default: quad_struct_rows<R, 64><<<grid, kQuadStreamBlock, 0, st>>>(q, x, tiles); break;
  }
  return hipGetLastError();
}

// The factors' share of A_gram from P = F' A1 (rank x m per cone): Ps = diag(sigma) P, A_gram += P' Ps (beta = 1; 0
// without S).  Both forms of A end here: the dense one below, the one held by its nonzeros in QuadSparseConstants.
static int QuadFactorGram(cxk_context* ctx, Group& g, const QuadStructured& q, int m, const double* P, double* Ps) {
  const int cnt = q.count, rank = q.rank;
  constexpr int kMaxBatch = 65535;  // gridDim.z
  const size_t blocks = ((size_t)cnt * rank * m + kQuadStreamBlock - 1) / kQuadStreamBlock;
  CXK_DEMAND(blocks <= (size_t)INT_MAX, "a group of structured quadratic cones with more than 2^39 entries of F' A is not supported");
  quad_struct_scale_rows<<<(unsigned)blocks, kQuadStreamBlock, 0, ctx->stream>>>(q, P, m, Ps);
  CXK_TRY(hipGetLastError());
  for (int b0 = 0; b0 < cnt; b0 += kMaxBatch) {  // A_gram += P' Ps
    const int nb = std::min(kMaxBatch, cnt - b0);
    GemmArgs a{};
    a.inner = 1;
    a.alpha = 1.0;
    a.beta = q.has_s ? 1.0 : 0.0;
    a.splits = 1;
    a.M = a.N = m;
    a.K = rank;
    a.A = P + (size_t)b0 * rank * m;
    a.lda = rank;
    a.sA1 = (int64_t)rank * m;
    a.B = Ps + (size_t)b0 * rank * m;
    a.ldb = rank;
    a.sB1 = (int64_t)rank * m;
    a.C = g.quad.Gram.p + (size_t)b0 * m * m;
    a.ldc = m;
    a.sC1 = (int64_t)m * m;
    CXK_TRY(LaunchGemm(a, true, false, nb, ctx->stream));
  }
  return CXK_SUCCESS;
}

// A_gram = A1' Q A1 without forming Q:
//   T = S A1 (n x m, lives for this call) by quad_struct_sa, A_gram = A1' T;
//   P = F' A1 (rank x m), Ps = diag(sigma) P, A_gram += P' Ps (beta = 1; 0 without S).
// The products on the batched GEMM, as the dense form's.
static int QuadStructuredGram(cxk_context* ctx, Group& g, const QuadStreamGroup& d) {
  const QuadStructured q = MakeQuadStructured(g, d);
  const int cnt = d.count, n = d.n, m = d.m, len = n + 1, rank = q.rank;
  if (m == 0) return CXK_SUCCESS;
  DevBuf<double> T, P, Ps;
  const int tiles = (n + kQuadStreamRowTile - 1) / kQuadStreamRowTile, ctiles = (m + kQuadStructColTile - 1) / kQuadStructColTile;
  if (q.has_s) {
    CXK_DEMAND((size_t)cnt * tiles * ctiles <= (size_t)INT_MAX,
               "a group of structured quadratic cones with more than 2^31 row tiles x column tiles is not supported");
    CXK_TRY(T.alloc((size_t)cnt * n * m));
    quad_struct_sa<<<(unsigned)((size_t)cnt * tiles * ctiles), kQuadStreamBlock, 0, ctx->stream>>>(q, g.A.p, m, T.p, tiles, ctiles);
    CXK_TRY(hipGetLastError());
  }
  if (rank > 0) {
    CXK_TRY(P.alloc((size_t)cnt * rank * m));
    CXK_TRY(Ps.alloc((size_t)cnt * rank * m));
  }
  constexpr int kMaxBatch = 65535;  // gridDim.z
  for (int b0 = 0; b0 < cnt; b0 += kMaxBatch) {
    const int nb = std::min(kMaxBatch, cnt - b0);
    const double* A1 = g.A.p + (size_t)b0 * len * m + 1;
    GemmArgs a{};
    a.inner = 1;
    a.alpha = 1.0;
    a.beta = 0.0;
    a.splits = 1;
    if (q.has_s) {  // A_gram = A1' T
      a.M = a.N = m;
      a.K = n;
      a.A = A1;
      a.lda = len;
      a.sA1 = (int64_t)len * m;
      a.B = T.p + (size_t)b0 * n * m;
      a.ldb = n;
      a.sB1 = (int64_t)n * m;
      a.C = g.quad.Gram.p + (size_t)b0 * m * m;
      a.ldc = m;
      a.sC1 = (int64_t)m * m;
      CXK_TRY(LaunchGemm(a, true, false, nb, ctx->stream));
    }
    if (rank > 0) {  // P = F' A1
      a.M = rank;
      a.N = m;
      a.K = n;
      a.A = q.F + (size_t)b0 * n * rank;
      a.lda = n;
      a.sA1 = (int64_t)n * rank;
      a.B = A1;
      a.ldb = len;
      a.sB1 = (int64_t)len * m;
      a.C = P.p + (size_t)b0 * rank * m;
      a.ldc = rank;
      a.sC1 = (int64_t)rank * m;
      CXK_TRY(LaunchGemm(a, true, false, nb, ctx->stream));
    }
  }
  if (rank > 0 && QuadFactorGram(ctx, g, q, m, P.p, Ps.p)) return CXK_FAILURE;
  CXK_TRY(hipStreamSynchronize(ctx->stream));  // (T, P and Ps are released on return)
  return CXK_SUCCESS;
}

// A group of structured quadratic cones at cxk_finalize: the members' CSR lists one after the other, each member's row
// pointers shifted by where its list starts, F and sigma member by member; the streamed route's work space with one
// split; then the constants on the device: Qc1 and c1' Q c1 by the pass and quad_stream_constants, as the dense form's,
// and A_gram.  Nothing of n x n, on either side.
int UploadQuadStructured(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size(), n = (size_t)g.n, m = (size_t)g.m, rank = (size_t)g.quad.sq.rank;
  const size_t tiles = (n + kQuadStreamRowTile - 1) / kQuadStreamRowTile;
  QuadState::Structured& q = g.quad.sq;
  size_t nnz = 0;
  for (size_t k = 0; k < cnt; k++) nnz += ctx->cons[g.ids[k]].sq.col.size();
  CXK_DEMAND(nnz <= (size_t)INT_MAX,
             "a group of structured quadratic cones whose sparse parts have more than 2^31 nonzeros is not supported");
  g.quad.splits = 1;
  q.lanes = sw.quad_csr_lanes > 0 ? sw.quad_csr_lanes : QuadCsrLanes((double)nnz, (double)(cnt * n));
  q.segs = QuadFactorSegments(g.n, (long long)(cnt * rank));
  CXK_DEMAND(cnt * std::max<size_t>(std::max<size_t>(m, (m * m + kQuadStreamBlock - 1) / kQuadStreamBlock),
                                    std::max<size_t>(std::max<size_t>(tiles, rank * (size_t)q.segs),
                                                     (n + 1 + kSocStreamRowTile - 1) / kSocStreamRowTile)) <=
                 (size_t)INT_MAX,
             "a group of structured quadratic cones with more than 2^31 columns, row tiles, factor segments or blocks is not supported");
  if (q.has_s) {
    std::vector<long long> hp(cnt * (n + 1));
    std::vector<int> hc(nnz);
    std::vector<double> hv(nnz);
    size_t base = 0;
    for (size_t k = 0; k < cnt; k++) {
      const ConstraintRec::StructuredQ& c = ctx->cons[g.ids[k]].sq;
      for (size_t r = 0; r <= n; r++) hp[k * (n + 1) + r] = (long long)base + c.ptr[r];
      std::copy(c.col.begin(), c.col.end(), hc.begin() + base);
      std::copy(c.val.begin(), c.val.end(), hv.begin() + base);
      base += c.col.size();
    }
    CXK_TRY(q.rowptr.upload(hp));
    CXK_TRY(q.col.upload(hc));
    CXK_TRY(q.val.upload(hv));
  }
  if (rank > 0) {
    std::vector<double> hF(cnt * n * rank), hs(cnt * rank);
    for (size_t k = 0; k < cnt; k++) {
      const ConstraintRec::StructuredQ& c = ctx->cons[g.ids[k]].sq;
      std::copy(c.F.begin(), c.F.end(), hF.begin() + k * n * rank);
      std::copy(c.sigma.begin(), c.sigma.end(), hs.begin() + k * rank);
    }
    CXK_TRY(q.F.upload(hF));
    CXK_TRY(q.sigma.upload(hs));
    CXK_TRY(q.tpart.alloc(cnt * 2 * rank * (size_t)q.segs));
  }
  CXK_TRY(g.quad.Gram.alloc(m * m * cnt));
  CXK_TRY(g.quad.S.alloc((n + 1) * cnt));
  CXK_TRY(g.quad.vec.alloc(QuadStreamVecDoubles(cnt, n, m)));
  CXK_TRY(g.quad.part.alloc(cnt * 2 * n));
  if (g.quad.sa.on) return QuadSparseConstants(ctx, g);
  const QuadStreamGroup d = MakeQuadStream(g);
  CXK_TRY(LaunchQuadStreamQmv<1>(g, d, QuadStreamOne(d.c + 1, n + 1), ctx->stream));
  quad_stream_constants<<<(int)cnt, kQuadStreamBlock, 0, ctx->stream>>>(d);
  CXK_TRY(hipGetLastError());
  return QuadStructuredGram(ctx, g, d);
}

// ---- Streamed quadratic cones whose A is held by its nonzeros (cxk_add_quadratic_csr; the kernels of
// kernels_quad_sparse.hip.h), whatever the form of Q.  Such a group is a streamed group in everything but the four
// places that read A: the columns and row 0 of the assembly, the slack, and A_gram at finalize.  Nothing of
// (n + 1) x m or n x m is allocated.

// What those kernels read of the group (UploadQuadSparseA uploads it).
QuadSparseGroup MakeQuadSparse(const Group& g) {
  QuadSparseGroup s;
  s.n = g.n;
  s.m = g.m;
  s.count = static_cast<int>(g.ids.size());
  s.eptr = g.quad.sa.nz.eptr.p;
  s.colptr = g.quad.sa.nz.colptr.p;
  s.crow = g.quad.sa.nz.crow.p;
  s.cval = g.quad.sa.nz.cval.p;
  return s;
}
// The nonzeros by rows and by columns (the lists of the sparse second-order cones), and row 0 as a dense vector per cone.
int UploadQuadSparseA(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), m = (size_t)g.m;
  CXK_DEMAND(cnt * (size_t)kQuadGramPanelMaxCols <= (size_t)INT_MAX,
             "a group of quadratic cones added by cxk_add_quadratic_csr with more than 2^25 members is not supported");
  if (UploadSparseNonzeros(ctx, g, g.quad.sa.nz)) return CXK_FAILURE;
  std::vector<double> h0(cnt * m, 0.0);
  for (size_t k = 0; k < cnt; k++) {
    const ConstraintRec::RowNonzeros& r = ctx->cons[g.ids[k]].rows;
    for (int s = r.ptr[0]; s < r.ptr[1]; s++) h0[k * m + (size_t)r.col[(size_t)s]] = r.val[(size_t)s];
  }
  CXK_TRY(g.quad.sa.a0.upload(h0));
  return CXK_SUCCESS;
}

// v = A1' Q w1 + A0 W0 of an assembly.  A dense A: one workgroup per column, which forms u = A1' Q c1 beside it.  By
// nonzeros: one wavefront per column through the CSC; u is constant and was made at finalize.
void LaunchQuadSchurColumns(Group& g, const QuadStreamGroup& d, hipStream_t st) {
  const size_t cols = (size_t)d.count * d.m;
  if (!g.quad.sa.on) {
    quad_stream_schur_columns<<<(unsigned)cols, kQuadStreamBlock, 0, st>>>(d);
    return;
  }
  constexpr int per = kQuadSparseBlock / 64;  // columns per workgroup
  quad_sparse_columns<<<(unsigned)((cols + per - 1) / per), kQuadSparseBlock, 0, st>>>(MakeQuadSparse(g), d.W, (size_t)d.n + 1, d.qw, d.v);
}

// The constants of such a group, once at cxk_finalize, on the device: Qc1 and c1' Q c1 as every streamed group's,
// u = A1' Q c1 by the columns kernel on (0, Qc1), and A_gram = A1' Q A1 in panels of P columns of A1
// (cone_route.h: QuadGramPanelCols).  Per panel: its columns scattered into a zeroed buffer of the dense form's layout
// ((n + 1) x P per cone, row 0 unread), T = Q panel by the code of the dense A -- the GEMM for a dense Q, quad_struct_sa
// for S, nothing for the identity (T is the panel) -- and A_gram[:, panel] = A1' T gathered through the CSC.  The
// factors' F' A1 (rank x m) is not made panel by panel: a GEMM of M = rank, N = P and K = n is one workgroup's loop over
// n (55 ms a panel at n = 2^20, measured); it is the same gather on T = F, once, nnz rank multiply-adds.  Their share of
// A_gram follows once, as with a dense A; where Q is the factors alone there are no panels at all.
int QuadSparseConstants(cxk_context* ctx, Group& g) {
  const QuadStreamGroup d = MakeQuadStream(g);
  const QuadSparseGroup s = MakeQuadSparse(g);
  const int cnt = d.count, n = d.n, m = d.m, len = n + 1;
  constexpr int per = kQuadSparseBlock / 64;
  CXK_TRY(LaunchQuadStreamQmv<1>(g, d, QuadStreamOne(d.c + 1, (size_t)len), ctx->stream));
  quad_stream_constants<<<cnt, kQuadStreamBlock, 0, ctx->stream>>>(d);
  CXK_TRY(hipGetLastError());
  if (m == 0) return CXK_SUCCESS;
  const unsigned col_grid = (unsigned)(((size_t)cnt * m + per - 1) / per);
  quad_sparse_columns<<<col_grid, kQuadSparseBlock, 0, ctx->stream>>>(s, nullptr, 0, d.qc1, d.u);
  CXK_TRY(hipGetLastError());
  const bool structured = d.q_form == kQuadQStructured;
  QuadStructured q{};
  if (structured) q = MakeQuadStructured(g, d);
  const int rank = structured ? q.rank : 0;
  const bool with_t = d.q_form == kQuadQDense || (structured && q.has_s);  // (else T is the panel, or A_gram is the factors' alone)
  const bool gathers = with_t || d.q_form == kQuadQIdentity;
  const int P = std::min(m, QuadGramPanelCols(n, cnt));
  DevBuf<double> panel, T, Pf, Ps;
  if (gathers) CXK_TRY(panel.alloc((size_t)cnt * P * len));
  if (with_t) CXK_TRY(T.alloc((size_t)cnt * n * P));
  if (rank > 0) {  // Pf = F' A1: entry (k, i) from column i of A1 and column k of F
    CXK_TRY(Pf.alloc((size_t)cnt * rank * m));
    CXK_TRY(Ps.alloc((size_t)cnt * rank * m));
    quad_sparse_gather<<<col_grid, kQuadSparseBlock, 0, ctx->stream>>>(s, q.F, (size_t)n, (size_t)n * rank, rank, Pf.p, (size_t)rank * m,
                                                                      (size_t)rank, 1);
    CXK_TRY(hipGetLastError());
  }
  const int tiles = (n + kQuadStreamRowTile - 1) / kQuadStreamRowTile;
  constexpr int kMaxBatch = 65535;  // gridDim.z
  for (int j0 = 0; gathers && j0 < m; j0 += P) {
    const int pw = std::min(P, m - j0);
    CXK_TRY(hipMemsetAsync(panel.p, 0, sizeof(double) * (size_t)cnt * P * len, ctx->stream));
    quad_sparse_scatter<<<(unsigned)(((size_t)cnt * pw + per - 1) / per), kQuadSparseBlock, 0, ctx->stream>>>(s, panel.p, j0, pw, P);
    CXK_TRY(hipGetLastError());
    if (structured && q.has_s) {  // T = S panel (the panel as an A of P columns)
      const int ctiles = (pw + kQuadStructColTile - 1) / kQuadStructColTile;
      CXK_DEMAND((size_t)cnt * tiles * ctiles <= (size_t)INT_MAX,
                 "a group of structured quadratic cones with more than 2^31 row tiles x column tiles is not supported");
      quad_struct_sa<<<(unsigned)((size_t)cnt * tiles * ctiles), kQuadStreamBlock, 0, ctx->stream>>>(q, panel.p, P, T.p, tiles, ctiles);
      CXK_TRY(hipGetLastError());
    }
    for (int b0 = 0; d.q_form == kQuadQDense && b0 < cnt; b0 += kMaxBatch) {  // T = Q panel
      const int nb = std::min(kMaxBatch, cnt - b0);
      GemmArgs a{};
      a.inner = 1;
      a.alpha = 1.0;
      a.beta = 0.0;
      a.splits = 1;
      a.M = n;
      a.N = pw;
      a.K = n;
      a.A = g.quad.Q.p + (size_t)b0 * n * n;
      a.lda = n;
      a.sA1 = (int64_t)n * n;
      a.B = panel.p + (size_t)b0 * len * P + 1;
      a.ldb = len;
      a.sB1 = (int64_t)len * P;
      a.C = T.p + (size_t)b0 * n * P;
      a.ldc = n;
      a.sC1 = (int64_t)n * P;
      CXK_TRY(LaunchGemm(a, false, false, nb, ctx->stream));
    }
    double* out = g.quad.Gram.p + (size_t)j0 * m;  // A_gram[i, j0 + jj]
    if (with_t)
      quad_sparse_gather<<<col_grid, kQuadSparseBlock, 0, ctx->stream>>>(s, T.p, (size_t)n, (size_t)n * P, pw, out, (size_t)m * m, 1, (size_t)m);
    else
      quad_sparse_gather<<<col_grid, kQuadSparseBlock, 0, ctx->stream>>>(s, panel.p + 1, (size_t)len, (size_t)len * P, pw, out, (size_t)m * m, 1, (size_t)m);
    CXK_TRY(hipGetLastError());
  }
  if (rank > 0 && QuadFactorGram(ctx, g, q, m, Pf.p, Ps.p)) return CXK_FAILURE;
  CXK_TRY(hipStreamSynchronize(ctx->stream));  // (the panel, T, F' A1 and its scaled copy are released on return)
  return CXK_SUCCESS;
}

// PrepareStep (MODE 0) or the eigenvalue query (MODE 1) of one group.
namespace {
template <int MODE>
int QuadPrepare(cxk_context* ctx, Group& g, const StepArgs& sa) {
  const int cnt = (int)g.ids.size();
  switch (g.route) {
    case ConeRoute::kQuadLds: quad_prepare<MODE><<<cnt, 64, QuadPrepareLds(g.n, g.m), ctx->stream>>>(MakeQuad(g), sa); break;
    case ConeRoute::kQuadStreamed: {
      const QuadStreamGroup d = MakeQuadStream(g);
      if (g.quad.sa.on)  // (A by its nonzeros: the sparse second-order cones' slack, on this group's rows and ms)
        LaunchSocSparseSlack(MakeVec(g), d.ms, g.quad.sa.nz, sa, ctx->stream);
      else
        LaunchSocStreamSlack(QuadStreamSlackView(g, d), sa, ctx->stream);
      QuadStreamVecs x;  // Q [w1, ms1] in one pass
      x.p[0] = d.W + 1;
      x.p[1] = d.ms + 1;
      x.stride[0] = x.stride[1] = (size_t)g.n + 1;
      CXK_TRY(LaunchQuadStreamQmv<2>(g, d, x, ctx->stream));
      quad_stream_prepare_mid<MODE><<<cnt, kQuadStreamBlock, 0, ctx->stream>>>(d, sa);
      CXK_TRY(LaunchQuadStreamQmv<1>(g, d, QuadStreamOne(d.dv, (size_t)g.n), ctx->stream));
      quad_stream_prepare_finish<MODE><<<cnt, kQuadStreamBlock, 0, ctx->stream>>>(d, sa);
      break;
    }
    default: CXK_DEMAND(false, "internal error: not a route of the quadratic cones");
  }
  return CXK_SUCCESS;
}
}  // namespace

int LaunchQuadPrepare(cxk_context* ctx, Group& g, int mode, const StepArgs& sa) {
  return mode == 0 ? QuadPrepare<0>(ctx, g, sa) : QuadPrepare<1>(ctx, g, sa);
}

int LaunchQuadTakeStep(cxk_context* ctx, Group& g, const StepArgs& sa) {
  const int cnt = (int)g.ids.size();
  switch (g.route) {
    case ConeRoute::kQuadLds: quad_take_step<<<cnt, 64, QuadTakeLds(g.n), ctx->stream>>>(MakeQuad(g), sa); break;
    case ConeRoute::kQuadStreamed: quad_stream_take_step<<<cnt, kQuadStreamBlock, 0, ctx->stream>>>(MakeQuadStream(g), sa); break;
    default: CXK_DEMAND(false, "internal error: not a route of the quadratic cones");
  }
  return CXK_SUCCESS;
}

}  // namespace cxk_host
