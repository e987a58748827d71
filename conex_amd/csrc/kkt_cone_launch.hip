// The per-cone stages of the cxk_* path: Schur complement, PrepareStep, eigenvalue query, TakeStep of
// every cone type, the choosers that name the LMI kernel of each stage, the per-group stages of cxk_finalize
// and the host mailbox.  Owns the kernels of kernels_cone / _oct / _quad / _lmi* (and mailbox_pack,
// newton_from_three below).
#include <hip/hip_ext.h>
#include "kkt_launch.h"
#include "kernels_cone.hip.h"
#include "kernels_gemm.hip.h"
#include "kernels_oct.hip.h"
#include "kernels_lmi.hip.h"
#include "lmi_fused_mfma.h"
#include "kernels_lmi_sparse.hip.h"
#include "kernels_lmi_rows.hip.h"
#include "kernels_lmi_large.hip.h"
#include "kernels_lmi_factored.hip.h"
#include "kernels_quad.hip.h"
#include "kernels_soc_stream.hip.h"
#include "kernels_linear_tiled.hip.h"
#include "kernels_linear_sparse.hip.h"
#include "kernels_soc_sparse.hip.h"
#include "kernels_quad_stream.hip.h"

namespace cxk_host {

// ---- The views the kernels take of a group, each beside the stage of cxk_finalize (UploadGroup) that allocates what
// it lays out, so that a layout and its size are read together.  What those stages call further down:
int UploadSparseLmi(cxk_context* ctx, Group& g);
int QuadStreamConstants(cxk_context* ctx, Group& g);
int SocSparseConstants(cxk_context* ctx, Group& g);
static int UploadSparseNonzeros(cxk_context* ctx, Group& g);
static int SocSparseGramChunks(int m);
static int SocSparseCombineTiles(int m);

LmiGroup MakeLmi(Group& g) {
  LmiGroup d;
  d.n = g.n;
  d.m = g.m;
  d.count = static_cast<int>(g.ids.size());
  d.A = g.A.p;
  d.a_stride = (long long)(g.assembly != LmiAssembly::kGeneric ? g.m + 1 : g.m) * g.n * g.n;
  d.C = g.C.p;
  d.W = g.W.p;
  d.T1 = g.T1.p;
  d.ids = g.dids.p;
  d.Apk = g.Apk.n ? g.Apk.p : nullptr;
  d.herm_d = g.herm_d;
  const bool sparse = g.route == ConeRoute::kLmiSparse;
  d.sp_eptr = sparse ? g.sp_eptr.p : nullptr;
  d.sp_erc = sparse ? g.sp_erc.p : nullptr;
  d.sp_pairs = sparse ? g.sp_pairs.p : nullptr;
  d.sp_eval = sparse ? g.sp_eval.p : nullptr;
  d.sp_pptr = sparse ? g.sp_pptr.p : nullptr;
  d.sp_pvar = sparse ? g.sp_pvar.p : nullptr;
  d.sp_pval = sparse ? g.sp_pval.p : nullptr;
  return d;
}
// Doubles of one member's A, C and W (T1, T2 and the quadratic cone's S are W's size).
struct GroupSizes {
  size_t a = 0, c = 0, w = 0;
};
static GroupSizes SizesOf(const Group& g) {
  const size_t n = (size_t)g.n, m = (size_t)g.m;
  switch (g.type) {
    case CXK_LMI: return {m * n * n, n * n, n * n};
    case CXK_LINEAR: return {n * m, n, n};
    case CXK_SOC: case CXK_QUAD: return {(n + 1) * m, n + 1, n + 1};
    case CXK_STATIC: return {m * m, m, 0};  // constant AQc (zeros for a quadratic-cost block)
    case CXK_OCT: return {m * 8 * n * n, 8 * n * n, 8 * n * n};
  }
  return {};
}
// The dense A and C of every member as the kernels of every route but the sparse and factored ones read them
// (`a_sz` 0: no dense copy of A on the device).
static int UploadDenseData(cxk_context* ctx, Group& g, size_t a_sz, size_t c_sz) {
  const size_t cnt = g.ids.size();
  // lmi_schur_mfma reads [A_1 .. A_m | C] of a constraint as one contiguous array of stacked
  // rows: such groups keep a copy of C right behind the A_i (LmiGroup::a_stride)
  const size_t a_blk = a_sz + (g.assembly != LmiAssembly::kGeneric ? c_sz : 0);
  std::vector<double> hA(a_blk * cnt), hC(c_sz * cnt);
  for (size_t k = 0; k < cnt; k++) {
    const ConstraintRec& c = ctx->cons[g.ids[k]];
    if (a_sz) std::copy(c.A.begin(), c.A.end(), hA.begin() + k * a_blk);
    if (a_blk > a_sz) std::copy(c.C.begin(), c.C.end(), hA.begin() + k * a_blk + a_sz);
    std::copy(c.C.begin(), c.C.end(), hC.begin() + k * c_sz);
  }
  CXK_TRY(g.A.upload(hA));
  CXK_TRY(g.C.upload(hC));
  return CXK_SUCCESS;
}
static int AllocGemmAssembly(cxk_context* ctx, Group& g, const FinalizeSwitches& sw);
// The three side copies of a dense LMI group's matrices: Apad (lmi_schur_mfma at a padded order), Aleft (the folded
// form of a Hermitian group on the GEMM assembly), Apk (the packed lower triangles of the slack pass); then the work
// space of the GEMM assembly (beside MakeLargeWs).
static int UploadLmiDense(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size();
  if (g.assembly == LmiAssembly::kMfma && LmiMfmaPaddedOrder(g.n) != g.n && !(g.herm_d == 2 && g.n == 24)) {
    const int np = LmiMfmaPaddedOrder(g.n), n = g.n;
    const size_t blk = (size_t)(g.m + 1) * np * np;
    std::vector<double> hp(blk * cnt, 0.0);
    for (size_t k = 0; k < cnt; k++) {
      const ConstraintRec& c = ctx->cons[g.ids[k]];
      for (int i = 0; i <= g.m; i++) {
        const double* src = i < g.m ? c.A.data() + (size_t)i * n * n : c.C.data();
        double* dst = hp.data() + k * blk + (size_t)i * np * np;
        for (int col = 0; col < n; col++) std::copy(src + (size_t)col * n, src + (size_t)col * n + n, dst + (size_t)col * np);
      }
    }
    CXK_TRY(g.Apad.upload(hp));
  }
  if (g.herm_d > 1 && g.assembly == LmiAssembly::kGemm && !g.literal && !sw.no_herm_fold) {
    // Hermitian cones over C / H on the batched-GEMM assembly: the folded form needs only the first
    // n / herm_d columns of every matrix of the real representation (kernels_lmi_large.hip.h)
    const int n = g.n, n0 = g.n / g.herm_d;
    const size_t per = (size_t)n * n0, m1 = (size_t)g.m + 1;
    std::vector<double> hl(per * m1 * cnt);
    for (size_t k = 0; k < cnt; k++) {
      const ConstraintRec& c = ctx->cons[g.ids[k]];
      for (size_t i = 0; i < m1; i++) {
        const double* src = i < (size_t)g.m ? c.A.data() + i * (size_t)n * n : c.C.data();
        std::copy(src, src + per, hl.begin() + (k * m1 + i) * per);
      }
    }
    CXK_TRY(g.Aleft.upload(hl));
  }
  if (!g.literal && !sw.no_packed_slack && g.n == 20 && LmiPrepareRowsSupports(g.n, g.m, g.herm_d, false)) {
    // the slack pass of PrepareStep / the eigenvalue query streams every A_i once more per call: a
    // packed copy of the lower triangles (the data is exactly symmetric) halves those bytes
    const int n = g.n, pk = n * (n + 1) / 2;
    std::vector<double> hp((size_t)pk * g.m * cnt);
    for (size_t k = 0; k < cnt; k++) {
      const ConstraintRec& c = ctx->cons[g.ids[k]];
      for (int i = 0; i < g.m; i++) {
        const double* src = c.A.data() + (size_t)i * n * n;
        double* dst = hp.data() + (k * g.m + i) * (size_t)pk;
        for (int col = 0; col < n; col++)
          for (int row = col; row < n; row++) *dst++ = src[row + (size_t)col * n];
      }
    }
    CXK_TRY(g.Apk.upload(hp));
  }
  return g.assembly == LmiAssembly::kGemm ? AllocGemmAssembly(ctx, g, sw) : CXK_SUCCESS;
}
// A sparse LMI group: its entry lists, and beyond the LDS-resident shapes the large-order work space.
static int UploadLmiSparse(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), nn = (size_t)g.n * g.n;
  if (UploadSparseLmi(ctx, g)) return CXK_FAILURE;
  if (g.large || !g.sp_small) {
    CXK_TRY(g.ws_main.alloc(cnt * 8 * nn));  // step temporaries; C W and W C W during assembly
    CXK_TRY(g.ws_part.alloc(cnt * 2 * kSparseCParts));
    CXK_TRY(g.ws_piv.alloc(cnt * (size_t)g.n));
  }
  return CXK_SUCCESS;
}
QuadGroup MakeQuad(Group& g) {
  QuadGroup d;
  d.n = g.n;
  d.m = g.m;
  d.count = static_cast<int>(g.ids.size());
  d.A = g.A.p;
  d.c = g.C.p;
  d.Q = g.has_q ? g.qQ.p : nullptr;
  d.Agram = g.qGram.p;
  d.W = g.W.p;
  d.D = g.T1.p;
  d.S = g.qS.p;
  d.ids = g.dids.p;
  return d;
}
// A_gram = A1' (Q A1) of a group of quadratic cones on the LDS route, made once on the host
// (QuadraticConstraintBase::Initialize, quadratic_cone_constraint.cc:216-219), Q, and the state S.
static int UploadQuadGram(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size();
  const int n = g.n, m = g.m, len = n + 1;
  std::vector<double> hQ(g.has_q ? (size_t)n * n * cnt : 0), hG((size_t)m * m * cnt, 0.0), qa((size_t)n);
  for (size_t k = 0; k < cnt; k++) {
    const ConstraintRec& c = ctx->cons[g.ids[k]];
    if (g.has_q) std::copy(c.Q.begin(), c.Q.end(), hQ.begin() + k * (size_t)n * n);
    for (int j = 0; j < m; j++) {
      const double* aj = c.A.data() + (size_t)j * len + 1;
      for (int i = 0; i < n; i++) {
        double s2 = g.has_q ? 0.0 : aj[i];
        if (g.has_q)
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
  CXK_TRY(g.qQ.upload(hQ));
  CXK_TRY(g.qGram.upload(hG));
  CXK_TRY(g.qS.alloc((size_t)len * cnt));
  return CXK_SUCCESS;
}
OctGroup MakeOct(Group& g) {
  OctGroup d;
  d.n = g.n;
  d.m = g.m;
  d.count = static_cast<int>(g.ids.size());
  d.A = g.A.p;
  d.C = g.C.p;
  d.W = g.W.p;
  d.S = g.T1.p;
  d.ids = g.dids.p;
  return d;
}
VecGroup MakeVec(Group& g) {
  VecGroup d;
  d.len = (g.type == CXK_SOC || g.type == CXK_QUAD) ? g.n + 1 : g.n;
  d.m = g.m;
  d.count = static_cast<int>(g.ids.size());
  d.A = g.A.p;
  d.c = g.C.p;
  d.W = g.W.p;
  d.T1 = g.T1.p;
  d.T2 = g.T2.p;
  d.ids = g.dids.p;
  return d;
}
SocStreamGroup MakeSocStream(Group& g) {
  SocStreamGroup d;
  const size_t per = g.ids.size() * ((size_t)g.n + 1);
  d.v = MakeVec(g);
  d.WA = g.ws_main.p;
  d.s = g.st_vec.p;
  d.wc = g.st_vec.p + per;
  d.ms = g.st_vec.p + 2 * per;
  d.dets = g.st_det.p;
  d.Gf = g.ws_gf.p;
  return d;
}
// The work space of the Gram product of LaunchGramLower, for streamed second-order cones (len = n + 1) and tiled
// linear blocks (len = n) alike: the scaled copy of A in ws_main, the products in ws_gf, the split partials in ws_part.
static int AllocGramWorkspace(cxk_context* ctx, Group& g, size_t len, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size(), m = (size_t)g.m;
  g.splits = SocStreamSplits((int)len, g.m, (long long)cnt);
  if (sw.gram_splits > 0) g.splits = sw.gram_splits;  // (comparison runs)
  CXK_TRY(g.ws_main.alloc(cnt * len * m));
  CXK_TRY(g.ws_gf.alloc(cnt * m * m));
  CXK_TRY(g.ws_part.alloc(g.splits > 1 ? (size_t)g.splits * std::min<size_t>(cnt, 65535) * m * m : 0));
  return CXK_SUCCESS;
}
static int UploadSocStream(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size(), len = (size_t)g.n + 1, m = (size_t)g.m;
  CXK_DEMAND(cnt * std::max<size_t>(m, (len + kSocStreamRowTile - 1) / kSocStreamRowTile) <= (size_t)INT_MAX,
             "a group of streamed second-order cones with more than 2^31 columns or row tiles is not supported");
  g.st_stages = sw.soc_stream_stages;
  if (AllocGramWorkspace(ctx, g, len, sw)) return CXK_FAILURE;
  CXK_TRY(g.st_vec.alloc(3 * cnt * len));
  CXK_TRY(g.st_det.alloc(cnt));
  return CXK_SUCCESS;
}
QuadStreamGroup MakeQuadStream(Group& g) {
  QuadStreamGroup d;
  const size_t cnt = g.ids.size(), n = (size_t)g.n, m = (size_t)g.m;
  d.n = g.n;
  d.m = g.m;
  d.count = static_cast<int>(cnt);
  d.splits = g.splits;
  d.A = g.A.p;
  d.c = g.C.p;
  d.Q = g.has_q ? g.qQ.p : nullptr;
  d.Agram = g.qGram.p;
  d.W = g.W.p;
  d.D = g.T1.p;
  d.S = g.qS.p;
  d.ids = g.dids.p;
  d.part = g.ws_part.p;
  double* p = g.st_vec.p;  // (the layout UploadQuadStream sizes: QuadStreamVecDoubles)
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
// A group of streamed quadratic cones: Q as it is, the work space, and the constants (Q c1, c1' Q c1, A_gram) on the
// device (QuadStreamConstants).
static int UploadQuadStream(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size();
  const size_t n = (size_t)g.n, m = (size_t)g.m, tiles = (n + kQuadStreamRowTile - 1) / kQuadStreamRowTile;
  g.splits = g.has_q ? QuadStreamSplits(g.n, (long long)cnt) : 1;
  if (g.has_q && sw.gram_splits > 0) g.splits = sw.gram_splits;  // (comparison runs)
  CXK_DEMAND(cnt * std::max<size_t>(std::max<size_t>(m, (m * m + kQuadStreamBlock - 1) / kQuadStreamBlock),
                                    std::max<size_t>(tiles * (size_t)g.splits, (n + 1 + kSocStreamRowTile - 1) / kSocStreamRowTile)) <=
                 (size_t)INT_MAX,
             "a group of streamed quadratic cones with more than 2^31 columns, row tiles or blocks is not supported");
  std::vector<double> hQ(g.has_q ? n * n * cnt : 0);
  if (g.has_q)
    for (size_t k = 0; k < cnt; k++) std::copy(ctx->cons[g.ids[k]].Q.begin(), ctx->cons[g.ids[k]].Q.end(), hQ.begin() + k * n * n);
  CXK_TRY(g.qQ.upload(hQ));
  CXK_TRY(g.qGram.alloc(m * m * cnt));
  CXK_TRY(g.qS.alloc((n + 1) * cnt));
  CXK_TRY(g.st_vec.alloc(QuadStreamVecDoubles(cnt, n, m)));
  CXK_TRY(g.ws_part.alloc(g.has_q ? cnt * (size_t)g.splits * 2 * n : 0));
  return QuadStreamConstants(ctx, g);
}
// soc_stream_slack serves the streamed quadratic cone as it is (same layout, same formula): what it reads of the group.
SocStreamGroup QuadStreamSlackView(Group& g, const QuadStreamGroup& d) {
  SocStreamGroup s{};
  s.v = MakeVec(g);
  s.ms = d.ms;
  return s;
}
LinTiledGroup MakeLinTiled(Group& g) {
  LinTiledGroup d;
  d.v = MakeVec(g);
  d.WA = g.ws_main.p;
  d.Gf = g.ws_gf.p;
  d.part = g.lt_part.p;
  return d;
}
static int UploadLinearTiled(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size(), len = (size_t)g.n, m = (size_t)g.m, tiles = (len + kLinTiledRowTile - 1) / kLinTiledRowTile;
  CXK_DEMAND(cnt * std::max(m, tiles) <= (size_t)INT_MAX,
             "a group of tiled linear blocks with more than 2^31 columns or row tiles is not supported");
  if (AllocGramWorkspace(ctx, g, len, sw)) return CXK_FAILURE;
  CXK_TRY(g.lt_part.alloc(cnt * tiles * 4));
  return CXK_SUCCESS;
}
LinSparseGroup MakeLinSparse(Group& g) {
  LinSparseGroup d;
  d.t = MakeLinTiled(g);  // (A is null, WA and Gf unused: the scalars and finish kernels read v and part only)
  d.eptr = g.ls_eptr.p;
  d.rowptr = g.ls_rowptr.p;
  d.col = g.ls_col.p;
  d.val = g.ls_val.p;
  d.colptr = g.ls_colptr.p;
  d.crow = g.ls_crow.p;
  d.cval = g.ls_cval.p;
  return d;
}
static int UploadLinearSparse(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), len = (size_t)g.n, m = (size_t)g.m, tiles = (len + kLinTiledRowTile - 1) / kLinTiledRowTile;
  const size_t chunks = m <= (size_t)kLinSparseWaveCols ? 1 : (m + kLinSparseColChunk - 1) / kLinSparseColChunk;
  if (UploadSparseNonzeros(ctx, g)) return CXK_FAILURE;
  CXK_DEMAND(cnt * std::max(m * chunks, tiles) <= (size_t)INT_MAX,
             "a group of sparse linear blocks with more than 2^31 column chunks or row tiles is not supported");
  CXK_TRY(g.lt_part.alloc(cnt * tiles * 4));
  return CXK_SUCCESS;
}
SocSparseGroup MakeSocSparse(Group& g) {
  SocSparseGroup d{};
  const size_t cnt = g.ids.size(), len = (size_t)g.n + 1, m = (size_t)g.m;
  d.st.v = MakeVec(g);  // (A is null; WA, wc, dets and Gf stay null: the step kernels read v, s and ms only)
  double* p = g.st_vec.p;  // (the layouts UploadSocSparse sizes: SocSparseVecDoubles, SocSparseConstDoubles)
  d.st.s = p;
  d.st.ms = (p += cnt * len);
  d.u = (p += cnt * len);
  d.scal = (p += cnt * m);
  p = g.ss_const.p;
  d.H = p;
  d.h = (p += cnt * m * m);
  d.z = (p += cnt * m);
  d.eptr = g.ls_eptr.p;
  d.rowptr = g.ls_rowptr.p;
  d.col = g.ls_col.p;
  d.val = g.ls_val.p;
  d.colptr = g.ls_colptr.p;
  d.crow = g.ls_crow.p;
  d.cval = g.ls_cval.p;
  return d;
}
size_t SocSparseVecDoubles(size_t cnt, size_t len, size_t m) { return cnt * (2 * len + m + 2); }
size_t SocSparseConstDoubles(size_t cnt, size_t m) { return cnt * (m * m + m + 1); }
// A group of sparse second-order cones: the nonzeros, the work space, and the constants on the device (SocSparseConstants).
static int UploadSocSparse(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), len = (size_t)g.n + 1, m = (size_t)g.m, tiles = (len + kSocStreamRowTile - 1) / kSocStreamRowTile;
  if (UploadSparseNonzeros(ctx, g)) return CXK_FAILURE;
  CXK_DEMAND(cnt * std::max(std::max(m * (size_t)SocSparseGramChunks(g.m), tiles), (size_t)SocSparseCombineTiles(g.m)) <=
                 (size_t)INT_MAX,
             "a group of sparse second-order cones with more than 2^31 column chunks, row tiles or tiles of the Schur "
             "block is not supported");
  CXK_TRY(g.st_vec.alloc(SocSparseVecDoubles(cnt, len, m)));
  CXK_TRY(g.ss_const.alloc(SocSparseConstDoubles(cnt, m)));
  return SocSparseConstants(ctx, g);
}
StaticGroup MakeStatic(Group& g) {
  StaticGroup d;
  d.m = g.m;
  d.count = static_cast<int>(g.ids.size());
  d.Gc = g.A.p;
  d.AQc0 = g.C.p;
  d.ids = g.dids.p;
  return d;
}
Arena MakeArena(cxk_context* ctx) {
  Arena a;
  a.G = ctx->G.p;
  a.g_off = ctx->d_g_off.p;
  a.AWc = ctx->AWc.p;
  a.AQcc = ctx->AQcc.p;
  a.r_off = ctx->d_r_off.p;
  a.sc = ctx->sc.p;
  return a;
}
StepArgs MakeStep(cxk_context* ctx, double* info, int affine, double cw, double ew, double ss) {
  StepArgs s{};  // (no three-part direction, no step length, cost weight or skip flag from the device: null)
  s.y = ctx->y.p;
  s.cl_ptr = ctx->cl_ptr.p;
  s.cl_perm = ctx->cl_perm.p;
  s.info = info;
  s.affine = affine;
  s.c_weight = cw;
  s.e_weight = ew;
  s.step_size = ss;
  s.cw_scale = 1.0;
  s.call = ctx->lanczos_calls;
  s.no_clamp = ctx->reference_identity > 0;
  return s;
}

LmiLargeWs MakeLargeWs(Group& g) {
  LmiLargeWs w;
  const size_t cnt = g.ids.size(), nn = (size_t)g.n * g.n, m1 = (size_t)g.m + 1;
  w.P = g.ws_main.p;
  w.PT = g.ws_main.p + cnt * m1 * nn;
  w.tmp = g.ws_main.p;
  w.Gf = g.ws_gf.p;
  w.part = g.ws_part.p;
  w.piv = g.ws_piv.p;
  w.splits = g.splits;
  w.fold = g.Aleft.n ? g.n / g.herm_d : 0;
  w.Aleft = g.Aleft.p;
  w.wide = g.ws_wide.n ? g.ws_wide.p : nullptr;
  w.wide_reduce = g.wide_reduce;
  return w;
}

// The work space of the batched-GEMM assembly (P and P' in ws_main, which the step kernels of a large group reuse),
// and the number of K splits of its contraction.
static int AllocGemmAssembly(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size(), nn = (size_t)g.n * g.n, m1 = (size_t)g.m + 1;
  // split-K of the contraction: enough workgroups to fill the chip, at most one K step each
  const int ksteps = (int)((nn + kGemmBK - 1) / kGemmBK);
  const int tiles = (int)(((m1 + 63) / 64) * ((m1 + 63) / 64));
  // (measured on BASELINE config 2, one constraint, K = 40 000: 39 / 78 / 156 / 312 / 512 / 768 / 1024
  // splits -> 115 / 93 / 82 / 81 / 76 / 80 / 82 us per KKT solve)
  g.splits = std::max(1, std::min(std::max(1, ksteps / 4), (int)((512 + cnt * tiles - 1) / (cnt * tiles))));
  if (sw.gram_splits > 0) g.splits = sw.gram_splits;  // (comparison runs)
  CXK_TRY(g.ws_main.alloc(cnt * std::max(2 * m1 * nn, 8 * nn)));
  CXK_TRY(g.ws_gf.alloc(cnt * m1 * m1));
  CXK_TRY(g.ws_piv.alloc(cnt * (size_t)g.n));
  CXK_TRY(g.ws_part.alloc(g.splits > 1 ? (size_t)g.splits * cnt * m1 * m1 : 0));
  return CXK_SUCCESS;
}

int LmiLargeSpectrumMaxOrder() {
  int n = 1;
  while (LmiLargeSpectrumLds(n + 1) <= kLdsLimit) n++;
  return n;
}

LmiFactoredGroup MakeLmiFactored(Group& g) {
  LmiFactoredGroup f{};
  const size_t cnt = g.ids.size(), nr = (size_t)g.n * g.f_R;
  f.R = g.f_R;
  f.d = g.herm_d > 1 ? g.herm_d : 1;
  f.rank_one = g.f_rank_one;
  f.F = g.f_F.p;
  f.sigma = g.f_sigma.p;
  f.ptr = g.f_ptr.p;
  f.var = g.f_var.p;
  f.Z = g.f_ws.p;  // (the layout UploadLmiFactored sizes: LmiFactoredWsDoubles)
  f.Y = f.Z + cnt * nr;
  f.Fs = f.Y + cnt * nr;
  f.P = f.Fs + cnt * nr * f.d;
  f.part = g.ws_part.p;
  f.npart = kSparseCParts;
  return f;
}
// (d: the column blocks of a Hermitian member's L(F); Z and Y keep R columns, Fs and P have d R)
size_t LmiFactoredWsDoubles(size_t cnt, size_t n, size_t R, size_t d) { return cnt * ((2 + d) * n * R + d * R * R); }

// A group of LMIs given by factors: every member's F, sigma, column pointers and column -> variable map, the work
// space of the factored kernels and of the large-order step kernels behind them.
static int UploadLmiFactored(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), n = (size_t)g.n, R = (size_t)g.f_R, m = (size_t)g.m;
  const size_t d = g.herm_d > 1 ? (size_t)g.herm_d : 1;  // (a Hermitian member's f_F is L(F): n x dR)
  CXK_DEMAND(cnt <= 65535, "a group of more than 65535 equal-shaped factored LMIs is not supported");
  std::vector<double> hF(cnt * n * R * d), hs(cnt * R);
  std::vector<int> hp(cnt * (m + 1)), hv(cnt * R);
  g.f_rank_one = true;
  for (size_t k = 0; k < cnt; k++) {
    const ConstraintRec& c = ctx->cons[g.ids[k]];
    std::copy(c.f_F.begin(), c.f_F.end(), hF.begin() + k * n * R * d);
    std::copy(c.f_sigma.begin(), c.f_sigma.end(), hs.begin() + k * R);
    std::copy(c.f_ptr.begin(), c.f_ptr.end(), hp.begin() + k * (m + 1));
    for (size_t i = 0; i < m; i++) {
      g.f_rank_one = g.f_rank_one && c.f_ptr[i + 1] - c.f_ptr[i] == 1;
      for (int q = c.f_ptr[i]; q < c.f_ptr[i + 1]; q++) hv[k * R + (size_t)q] = (int)i;
    }
  }
  CXK_TRY(g.f_F.upload(hF));
  CXK_TRY(g.f_sigma.upload(hs));
  CXK_TRY(g.f_ptr.upload(hp));
  CXK_TRY(g.f_var.upload(hv));
  CXK_TRY(g.f_ws.alloc(LmiFactoredWsDoubles(cnt, n, R, d)));
  CXK_TRY(g.ws_main.alloc(cnt * 8 * n * n));  // step temporaries; C W and W C W during assembly
  CXK_TRY(g.ws_part.alloc(cnt * 2 * kSparseCParts));
  CXK_TRY(g.ws_piv.alloc(cnt * n));
  return CXK_SUCCESS;
}

// ---- The kernel instance each per-constraint stage of an LMI group runs.  One chooser per stage: the
// launch sites switch on its answer and cxk_lmi_kernels reports it, so the two cannot disagree.  The
// choosers read only the group's shape and the flags fixed at create / initialize.
// One list for the codes and the names cxk_lmi_kernel_name reports: X(code, name), in code order.
#define CXK_LMI_KERNELS(X) \
  /* Schur complement (LaunchSchur) */                                                                          \
  X(kSchurGenericLiteral, "lmi_schur_generic literal")                                                          \
  X(kSchurGenericSym, "lmi_schur_generic symmetric")                                                            \
  X(kSchurMfma8, "lmi_schur_mfma<8> exact two-images")  /* lmi_schur_mfma<N, false> at order N, two P images */ \
  X(kSchurMfma8Pad, "lmi_schur_mfma<8> padded two-images")  /* ... at a smaller order, zero-padded */           \
  X(kSchurMfma12, "lmi_schur_mfma<12> exact two-images")                                                        \
  X(kSchurMfma12Pad, "lmi_schur_mfma<12> padded two-images")                                                    \
  X(kSchurMfma16, "lmi_schur_mfma<16> exact two-images")                                                        \
  X(kSchurMfma16Single, "lmi_schur_mfma<16> exact one-image")  /* ... one P image */                            \
  X(kSchurMfma16Pad, "lmi_schur_mfma<16> padded two-images")                                                    \
  X(kSchurMfma16PadSingle, "lmi_schur_mfma<16> padded one-image")                                               \
  X(kSchurMfma20, "lmi_schur_mfma<20> exact two-images")                                                        \
  X(kSchurMfma20Single, "lmi_schur_mfma<20> exact one-image")                                                   \
  X(kSchurMfma20Pad, "lmi_schur_mfma<20> padded two-images")                                                    \
  X(kSchurMfma20PadSingle, "lmi_schur_mfma<20> padded one-image")                                               \
  X(kSchurMfma24, "lmi_schur_mfma<24> exact two-images")                                                        \
  X(kSchurMfma24Single, "lmi_schur_mfma<24> exact one-image")                                                   \
  X(kSchurMfma24Pad, "lmi_schur_mfma<24> padded two-images")                                                    \
  X(kSchurMfma24PadSingle, "lmi_schur_mfma<24> padded one-image")                                               \
  X(kSchurMfma24Folded, "lmi_schur_mfma<24,folded> two-images")                                                 \
  X(kSchurMfma24FoldedSingle, "lmi_schur_mfma<24,folded> one-image")                                            \
  X(kSchurGemm, "schur_gemm full lds")  /* batched-GEMM assembly: full form, LDS-resident order, one K split */ \
  X(kSchurGemmSplit, "schur_gemm full lds split")                                                               \
  X(kSchurGemmLarge, "schur_gemm full large")                                                                   \
  X(kSchurGemmLargeSplit, "schur_gemm full large split")                                                        \
  X(kSchurGemmFolded, "schur_gemm folded lds")                                                                  \
  X(kSchurGemmFoldedSplit, "schur_gemm folded lds split")                                                       \
  X(kSchurGemmFoldedLarge, "schur_gemm folded large")                                                           \
  X(kSchurGemmFoldedLargeSplit, "schur_gemm folded large split")                                                \
  X(kSchurSparseSmall, "lmi_schur_sparse small")                                                                \
  X(kSchurSparseSmallDenseC, "lmi_schur_sparse small dense-C")                                                  \
  X(kSchurSparse, "lmi_schur_sparse hbm")                                                                       \
  X(kSchurSparseDenseC, "lmi_schur_sparse hbm dense-C")                                                         \
  /* PrepareStep (MODE 0) and the eigenvalue query (MODE 1): the same order of instances each */                \
  X(kPrepareRowsPacked, "lmi_prepare_rows<0,20,exact> packed")                                                  \
  X(kPrepareRowsExact, "lmi_prepare_rows<0,20,exact> unpacked")  /* order 20, Apk null */                       \
  X(kPrepareRowsOdd, "lmi_prepare_rows<0,20> odd")                                                              \
  X(kPrepareRowsEven, "lmi_prepare_rows<0,20> even")                                                            \
  X(kPrepareGeneric20, "lmi_prepare_generic<0,20>")                                                             \
  X(kPrepareGeneric, "lmi_prepare_generic<0,0>")                                                                \
  X(kPrepareLarge, "LmiLargePrepare<0>")                                                                        \
  X(kQueryRowsPacked, "lmi_prepare_rows<1,20,exact> packed")                                                    \
  X(kQueryRowsExact, "lmi_prepare_rows<1,20,exact> unpacked")                                                   \
  X(kQueryRowsOdd, "lmi_prepare_rows<1,20> odd")                                                                \
  X(kQueryRowsEven, "lmi_prepare_rows<1,20> even")                                                              \
  X(kQueryGeneric20, "lmi_prepare_generic<1,20>")                                                               \
  X(kQueryGeneric, "lmi_prepare_generic<1,0>")                                                                  \
  X(kQueryLarge, "LmiLargePrepare<1>")                                                                          \
  /* the affine update (PrepareStep with affine != 0) */                                                        \
  X(kAffineGeneric20, "lmi_prepare_generic<0,20> affine")                                                       \
  X(kAffineGeneric, "lmi_prepare_generic<0,0> affine")                                                          \
  X(kAffineLarge, "LmiLargePrepare<0> affine")                                                                  \
  /* TakeStep */                                                                                                \
  X(kTakeRows20, "lmi_take_step_rows<20> exact")                                                                \
  X(kTakeRows20Pad, "lmi_take_step_rows<20> padded")                                                            \
  X(kTakeRows32, "lmi_take_step_rows<32> exact")                                                                \
  X(kTakeRows32Pad, "lmi_take_step_rows<32> padded")                                                            \
  X(kTakeTaylor24, "lmi_take_step_rows_taylor<24> exact")                                                       \
  X(kTakeTaylor24Pad, "lmi_take_step_rows_taylor<24> padded")                                                   \
  X(kTakeTaylor32, "lmi_take_step_rows_taylor<32> exact")                                                       \
  X(kTakeTaylor32Pad, "lmi_take_step_rows_taylor<32> padded")                                                   \
  X(kTakeGeneric20, "lmi_take_step_generic<20>")                                                                \
  X(kTakeGeneric, "lmi_take_step_generic<0>")                                                                   \
  X(kTakeLargePade, "LmiLargeTakeStep pade")                                                                    \
  X(kTakeLargeTaylor, "LmiLargeTakeStep taylor")

enum LmiKernel : int {
#define CXK_LMI_CODE(id, name) id,
  CXK_LMI_KERNELS(CXK_LMI_CODE)
#undef CXK_LMI_CODE
  kLmiKernelCount
};

const char* const kLmiKernelNames[kLmiKernelCount] = {
#define CXK_LMI_NAME(id, name) name,
    CXK_LMI_KERNELS(CXK_LMI_NAME)
#undef CXK_LMI_NAME
};

bool IsSchurMfma(LmiKernel k) { return k >= kSchurMfma8 && k <= kSchurMfma24FoldedSingle; }
bool IsSchurGemm(LmiKernel k) { return k >= kSchurGemm && k <= kSchurGemmFoldedLargeSplit; }
bool IsSchurSparse(LmiKernel k) { return k >= kSchurSparseSmall && k <= kSchurSparseDenseC; }
bool IsPrepareRows(LmiKernel k) {
  return (k >= kPrepareRowsPacked && k <= kPrepareRowsEven) || (k >= kQueryRowsPacked && k <= kQueryRowsEven);
}
bool IsTakeRows(LmiKernel k) { return k >= kTakeRows20 && k <= kTakeTaylor32Pad; }

LmiKernel LmiSchurKernel(const Group& g) {
  // not one of the instances: a code outside the reported range, which no Is*() test accepts and
  // cxk_lmi_kernel_name has no name for (LaunchSchur switches on the route first, cxk_lmi_kernels refuses the constraint)
  if (g.route == ConeRoute::kLmiFactored) return kLmiKernelCount;
  if (g.route == ConeRoute::kLmiSparse) return (LmiKernel)((g.sp_small ? kSchurSparseSmall : kSchurSparse) + (g.sp_cdense ? 1 : 0));
  if (g.assembly == LmiAssembly::kGemm) {  // (fold and split counts as LmiLargeSchur reads them: MakeLargeWs, LmiFoldedSplits)
    const bool fold = g.Aleft.n != 0;
    const int splits = fold ? LmiFoldedSplits(g.splits, g.n, g.n / g.herm_d) : g.splits;
    return (LmiKernel)(kSchurGemm + (fold ? 4 : 0) + (g.large ? 2 : 0) + (splits > 1 ? 1 : 0));
  }
  if (g.assembly == LmiAssembly::kMfma) {
    const LmiMfmaInstance inst = LmiMfmaChoose(g.n, g.m, g.herm_d);
    if (inst.folded) return inst.single ? kSchurMfma24FoldedSingle : kSchurMfma24Folded;
    const bool pad = g.Apad.p != nullptr;
    switch (inst.order) {
      case 8: return pad ? kSchurMfma8Pad : kSchurMfma8;
      case 12: return pad ? kSchurMfma12Pad : kSchurMfma12;
      case 16: return (LmiKernel)(kSchurMfma16 + (pad ? 2 : 0) + (inst.single ? 1 : 0));
      case 20: return (LmiKernel)(kSchurMfma20 + (pad ? 2 : 0) + (inst.single ? 1 : 0));
      default: return (LmiKernel)(kSchurMfma24 + (pad ? 2 : 0) + (inst.single ? 1 : 0));
    }
  }
  return g.literal ? kSchurGenericLiteral : kSchurGenericSym;
}

// mode 0 PrepareStep, 1 the eigenvalue query, 2 the affine update
LmiKernel LmiPrepareKernel(const cxk_context* ctx, const Group& g, int mode) {
  const int base = mode == 0 ? kPrepareRowsPacked : kQueryRowsPacked;
  if (g.large) return mode == 2 ? kAffineLarge : (LmiKernel)(base + 6);
  if (mode != 2 && !ctx->prepare_lds && !g.literal && LmiPrepareRowsSupports(g.n, g.m, g.herm_d, g.route == ConeRoute::kLmiSparse)) {
    if (g.n == 20) return (LmiKernel)(base + (g.Apk.p ? 0 : 1));
    return (LmiKernel)(base + ((g.n & 1) ? 2 : 3));
  }
  if (mode == 2) return g.n == 20 ? kAffineGeneric20 : kAffineGeneric;
  return (LmiKernel)(base + (g.n == 20 ? 4 : 5));
}

bool TakeStepLdsSwitch() {
  static const bool on = getenv("CXK_TAKE_STEP_LDS") != nullptr;  // A/B switch (tests, timing)
  return on;
}

LmiKernel LmiTakeKernel(const Group& g) {
  if (g.large) return g.herm_d ? kTakeLargeTaylor : kTakeLargePade;
  if (LmiTakeStepRowsSupports(g.n) && !TakeStepLdsSwitch() && !g.literal) {
    if (g.herm_d == 0) return g.n <= 20 ? (g.n == 20 ? kTakeRows20 : kTakeRows20Pad) : (g.n == 32 ? kTakeRows32 : kTakeRows32Pad);
    return g.n <= 24 ? (g.n == 24 ? kTakeTaylor24 : kTakeTaylor24Pad) : (g.n == 32 ? kTakeTaylor32 : kTakeTaylor32Pad);
  }
  return g.n == 20 ? kTakeGeneric20 : kTakeGeneric;
}

// Kernels of this unit that may be launched with more than the default 64 KB of dynamic LDS.
hipError_t RaiseConeLdsLimits() {
  static PerDeviceOnce once;  // function attributes are per device: every device a context is built on
  return once.run([] {
    return RaiseDynamicLds({
        reinterpret_cast<const void*>(&lmi_schur_generic),
        reinterpret_cast<const void*>(&lmi_prepare_generic<0, 0>),
        reinterpret_cast<const void*>(&lmi_prepare_generic<1, 0>),
        reinterpret_cast<const void*>(&lmi_take_step_generic<0>),
        reinterpret_cast<const void*>(&soc_schur<true>),
        reinterpret_cast<const void*>(&soc_schur<false>),
        // a long thin cone ((n + 1) x (m + 2) within LDS, n in the thousands) passes 64 KB in its step kernels too
        reinterpret_cast<const void*>(&soc_prepare<0>),
        reinterpret_cast<const void*>(&soc_prepare<1>),
        reinterpret_cast<const void*>(&soc_take_step),
        reinterpret_cast<const void*>(&quad_schur),
        reinterpret_cast<const void*>(&quad_prepare<0>),
        reinterpret_cast<const void*>(&quad_prepare<1>),
        reinterpret_cast<const void*>(&quad_take_step),
    });
  });
}

// Entry lists of a sparse LMI group (kernels_lmi_sparse.hip.h) from the dense host matrices.
int UploadSparseLmi(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), nn = (size_t)g.n * g.n;
  const int n = g.n, m = g.m, m1 = m + 1;
  // a dense affine term stays out of the pair sums (X = W C W is formed instead)
  g.sp_cdense = false;
  for (size_t k = 0; k < cnt; k++) {
    size_t nz = 0;
    for (double v : ctx->cons[g.ids[k]].C) nz += (v != 0.0);
    if (nz > 64) g.sp_cdense = true;  // (C, C) alone would be nz^2 terms on one wavefront
  }
  std::vector<int> eptr(cnt * m1 + 1, 0), erc, pptr(cnt * nn + 1, 0), pvar;
  std::vector<double> eval, pval;
  g.sp_emax = 0;
  for (size_t k = 0; k < cnt; k++) {
    const ConstraintRec& c = ctx->cons[g.ids[k]];
    for (int i = 0; i < m1; i++) {
      const double* M = i < m ? c.A.data() + (size_t)i * nn : c.C.data();
      if (i < m || !g.sp_cdense)
        for (int col = 0; col < n; col++)
          for (int row = 0; row < n; row++) {
            const double v = M[row + (size_t)col * n];
            if (v != 0.0) {
              erc.push_back(row | (col << 16));
              eval.push_back(v);
            }
          }
      CXK_DEMAND(eval.size() < ((size_t)1 << 31), "sparse LMI group: too many nonzeros");
      eptr[k * m1 + i + 1] = (int)eval.size();
    }
    g.sp_emax = std::max(g.sp_emax, eptr[k * m1 + m1] - eptr[k * m1]);
    for (size_t q = 0; q < nn; q++) {
      for (int i = 0; i < m; i++) {
        const double v = c.A[(size_t)i * nn + q];
        if (v != 0.0) {
          pvar.push_back(i);
          pval.push_back(v);
        }
      }
      pptr[k * nn + q + 1] = (int)pval.size();
    }
  }
  g.sp_small = !g.large && LmiSparseLds(n, m, true, g.sp_cdense, 0) <= kLdsLimit;
  // work split: lanes per pair from the average number of terms of a pair (each lane takes four
  // terms at a time); enough workgroups to fill the chip when the group is small
  const double per_mat = cnt ? (double)eval.size() / (double)(cnt * m1) : 0.0;
  const double avg_terms = per_mat * per_mat;
  g.sp_lpp = avg_terms <= 8 ? 1 : avg_terms <= 64 ? 4 : avg_terms <= 1024 ? 16 : 64;
  const double pairs = 0.5 * m1 * (m1 + 1.0);
  const double per_block = (256.0 / g.sp_lpp) * 4.0;  // pairs one workgroup takes in stride
  int chunks = (int)std::ceil(pairs / per_block);
  const int cap = (int)std::max<size_t>(1, 2048 / std::max<size_t>(cnt, 1));
  g.sp_chunks = std::max(1, std::min(chunks, cap));
  {
    std::vector<int> pr;
    pr.reserve((size_t)m1 * (m1 + 1) / 2);
    for (int i = 0; i < m1; i++)
      for (int j = 0; j <= i; j++) pr.push_back(i | (j << 16));
    CXK_TRY(g.sp_pairs.upload(pr));
  }
  CXK_TRY(g.sp_eptr.upload(eptr));
  CXK_TRY(g.sp_erc.upload(erc));
  CXK_TRY(g.sp_eval.upload(eval));
  CXK_TRY(g.sp_pptr.upload(pptr));
  CXK_TRY(g.sp_pvar.upload(pvar));
  CXK_TRY(g.sp_pval.upload(pval));
  return CXK_SUCCESS;
}

// Sparse LMI group: the nonzero sums; a dense C first needs X = W C W (LDS for small orders, two
// GEMMs otherwise).

template <bool SMALL, int LPP>
hipError_t LaunchLmiSparseKernelL(Group& g, const LmiGroup& d, const Arena& ar, const double* X, hipStream_t st) {
  const dim3 grid(d.count, g.sp_chunks);
  const int emax = (g.sp_emax + 1) & ~1;  // keeps the arrays behind it 8-byte aligned
  const bool stage = LmiSparseLds(g.n, g.m, SMALL, g.sp_cdense, emax) <= kLdsLimit;
  const size_t lds = LmiSparseLds(g.n, g.m, SMALL, g.sp_cdense, stage ? emax : 0);
  SparseLaunch L;
  L.Xg = X;
  L.part = g.ws_part.p;
  L.npart = kSparseCParts;
  L.emax = stage ? emax : 0;
  L.cdense = g.sp_cdense;
  auto raise = [&](const void* k) -> hipError_t {  // dynamic LDS beyond 64 KB needs the attribute
    return lds > 64 * 1024 ? hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit)
                           : hipSuccess;
  };
  hipError_t e;
  if (stage) {
    if ((e = raise(reinterpret_cast<const void*>(&lmi_schur_sparse<SMALL, LPP, true>))) != hipSuccess) return e;
    lmi_schur_sparse<SMALL, LPP, true><<<grid, 256, lds, st>>>(d, ar, L);
  } else {
    if ((e = raise(reinterpret_cast<const void*>(&lmi_schur_sparse<SMALL, LPP, false>))) != hipSuccess) return e;
    lmi_schur_sparse<SMALL, LPP, false><<<grid, 256, lds, st>>>(d, ar, L);
  }
  return hipGetLastError();
}

template <bool SMALL>
hipError_t LaunchLmiSparseKernel(Group& g, const LmiGroup& d, const Arena& ar, const double* X, hipStream_t st) {
  switch (g.sp_lpp) {
    case 1: return LaunchLmiSparseKernelL<SMALL, 1>(g, d, ar, X, st);
    case 4: return LaunchLmiSparseKernelL<SMALL, 4>(g, d, ar, X, st);
    case 16: return LaunchLmiSparseKernelL<SMALL, 16>(g, d, ar, X, st);
    default: return LaunchLmiSparseKernelL<SMALL, 64>(g, d, ar, X, st);
  }
}

hipError_t LaunchLmiSchurSparse(Group& g, LmiKernel kern, const Arena& ar, hipStream_t st) {
  const LmiGroup d = MakeLmi(g);
  const int n = g.n;
  if (kern == kSchurSparseSmall || kern == kSchurSparseSmallDenseC) return LaunchLmiSparseKernel<true>(g, d, ar, nullptr, st);
  double* X = nullptr;
  if (g.sp_cdense) {
    const int64_t nn = (int64_t)n * n;
    double* CW = g.ws_main.p;                  // count x nn
    X = g.ws_main.p + (size_t)d.count * nn;    // count x nn
    hipError_t e;
    GemmArgs a = SquareGemm(n, d.C, nn, d.W, nn, CW, nn);
    if ((e = LaunchGemm(a, false, false, d.count, st)) != hipSuccess) return e;
    a = SquareGemm(n, d.W, nn, CW, nn, X, nn);
    if ((e = LaunchGemm(a, false, false, d.count, st)) != hipSuccess) return e;
    lmi_dense_c_scalars<<<dim3(kSparseCParts, d.count), 256, 0, st>>>(d, X, g.ws_part.p);
  }
  return LaunchLmiSparseKernel<false>(g, d, ar, X, st);
}

// Gf = alpha WA' WA of every member of a group (WA: len x m per member), lower triangles only: the batched GEMM with
// SYRK-shaped output, split along len when that is long (the work space of AllocGramWorkspace).
static hipError_t LaunchGramLower(Group& g, const double* WA, double* Gf, int cnt, int len, int m, double alpha, hipStream_t st) {
  const int64_t mm = (int64_t)m * m;
  constexpr int kMaxBatch = 65535;  // gridDim.z
  for (int b0 = 0; b0 < cnt; b0 += kMaxBatch) {
    const int nb = std::min(kMaxBatch, cnt - b0);
    GemmArgs a{};
    a.M = a.N = m;
    a.K = len;
    a.A = a.B = WA + (size_t)b0 * len * m;
    a.lda = a.ldb = len;
    a.sA1 = a.sB1 = (int64_t)len * m;
    a.C = Gf + (size_t)b0 * mm;
    a.ldc = m;
    a.sC1 = mm;
    a.inner = 1;
    a.alpha = alpha;
    a.beta = 0.0;
    a.lower_only = 1;
    a.splits = g.splits;
    a.sCs = (int64_t)std::min(cnt, kMaxBatch) * mm;
    const hipError_t e = LaunchGemmSplitK(a, true, false, nb, g.ws_part.p, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The Schur complement of a group of streamed second-order cones: vectors, apply, Gram (LaunchGramLower, alpha = 2),
// mirror.  Stream order is the only dependency.
hipError_t LaunchSocStreamSchur(Group& g, const Arena& ar, hipStream_t st) {
  const SocStreamGroup d = MakeSocStream(g);
  const int cnt = d.v.count, len = d.v.len, m = d.v.m;
  soc_stream_vectors<<<cnt, kSocStreamBlock, 0, st>>>(d, ar);
  if (m == 0 || g.st_stages == 1) return hipGetLastError();
  soc_stream_apply<<<(unsigned)((size_t)cnt * m), kSocStreamBlock, 0, st>>>(d, ar);
  if (g.st_stages == 2) return hipGetLastError();
  const hipError_t e = LaunchGramLower(g, d.WA, d.Gf, cnt, len, m, 2.0, st);
  if (e != hipSuccess) return e;
  soc_stream_mirror<<<GridFor((size_t)cnt * m * m, kSocStreamBlock), kSocStreamBlock, 0, st>>>(d, ar);
  return hipGetLastError();
}

// The Schur complement of a group of linear blocks on the tiled route: scalars, apply, Gram (LaunchGramLower,
// alpha = 1), mirror.  Stream order is the only dependency.
hipError_t LaunchLinearTiledSchur(Group& g, const Arena& ar, hipStream_t st) {
  const LinTiledGroup d = MakeLinTiled(g);
  const int cnt = d.v.count, len = d.v.len, m = d.v.m;
  linear_tiled_scalars<<<cnt, kLinTiledBlock, 0, st>>>(d, ar);
  if (m == 0) return hipGetLastError();
  linear_tiled_apply<<<(unsigned)((size_t)cnt * m), kLinTiledBlock, 0, st>>>(d, ar);
  const hipError_t e = LaunchGramLower(g, d.WA, d.Gf, cnt, len, m, 1.0, st);
  if (e != hipSuccess) return e;
  linear_tiled_mirror<<<GridFor((size_t)cnt * m * m, kLinTiledBlock), kLinTiledBlock, 0, st>>>(d, ar);
  return hipGetLastError();
}

// The Schur complement of a group of linear blocks on the sparse route: the scalars (the tiled route's kernel), then
// every column of every block from its nonzeros: one wavefront per column up to kLinSparseWaveCols variables, 256
// threads per column and chunk of kLinSparseColChunk entries beyond.
hipError_t LaunchLinearSparseSchur(Group& g, const Arena& ar, hipStream_t st) {
  const LinSparseGroup d = MakeLinSparse(g);
  const int cnt = d.t.v.count, m = d.t.v.m;
  linear_tiled_scalars<<<cnt, kLinTiledBlock, 0, st>>>(d.t, ar);
  if (m == 0) return hipGetLastError();
  if (m <= kLinSparseWaveCols) {
    linear_sparse_schur<kLinSparseWaveCols><<<(unsigned)((size_t)cnt * m), 64, 0, st>>>(d, ar, 1);
  } else {
    const int chunks = (m + kLinSparseColChunk - 1) / kLinSparseColChunk;
    linear_sparse_schur<kLinSparseColChunk><<<(unsigned)((size_t)cnt * m * chunks), 256, 0, st>>>(d, ar, chunks);
  }
  return hipGetLastError();
}

// Launch shapes of a group of sparse second-order cones: chunks of a column of H, tiles of the combine kernel.
static int SocSparseGramChunks(int m) { return m <= kSocSparseWaveCols ? 1 : (m + kSocSparseColChunk - 1) / kSocSparseColChunk; }
static int SocSparseCombineTiles(int m) { return (int)(((size_t)m * m + kSocSparseCombineTile - 1) / kSocSparseCombineTile); }

// The Schur complement of a group of second-order cones on the sparse route: det(w), w . c and the scalars, the
// column dots u = A' w with AW and AQc, then G = 4 u u' + 2 det(w) H.  Stream order is the only dependency.
hipError_t LaunchSocSparseSchur(Group& g, const Arena& ar, hipStream_t st) {
  const SocSparseGroup d = MakeSocSparse(g);
  const int cnt = d.st.v.count, m = d.st.v.m;
  soc_sparse_vectors<<<cnt, kSocSparseBlock, 0, st>>>(d, ar);
  if (m == 0) return hipGetLastError();
  constexpr int per = kSocSparseBlock / 64;  // columns per workgroup
  soc_sparse_dots<<<(unsigned)(((size_t)cnt * m + per - 1) / per), kSocSparseBlock, 0, st>>>(d, ar);
  const int tiles = SocSparseCombineTiles(m);
  soc_sparse_combine<<<(unsigned)((size_t)cnt * tiles), kSocSparseBlock, 0, st>>>(d, ar, tiles);
  return hipGetLastError();
}

// The constants of a group of sparse second-order cones, once at cxk_finalize, on the device: z = c' J c, then
// H = A' J A and h = A' J c column by column: one wavefront per column up to kSocSparseWaveCols variables, 256 threads
// per column and chunk of kSocSparseColChunk entries beyond.
// The launches carry a hipEvent pair: cxk_sparse_soc_setup_ms reports what this one-off step cost.
int SocSparseConstants(cxk_context* ctx, Group& g) {
  const SocSparseGroup d = MakeSocSparse(g);
  const int cnt = d.st.v.count, m = d.st.v.m;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  CXK_TRY(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    CXK_DEMAND(false, "hipEventCreate failed");
  }
  hipError_t err = hipEventRecord(e0, ctx->stream);
  soc_sparse_cjc<<<cnt, kSocSparseBlock, 0, ctx->stream>>>(d);
  if (m > 0 && m <= kSocSparseWaveCols) {
    soc_sparse_gram<kSocSparseWaveCols><<<(unsigned)((size_t)cnt * m), 64, 0, ctx->stream>>>(d, 1);
  } else if (m > 0) {
    const int chunks = SocSparseGramChunks(m);
    soc_sparse_gram<kSocSparseColChunk><<<(unsigned)((size_t)cnt * m * chunks), 256, 0, ctx->stream>>>(d, chunks);
  }
  if (err == hipSuccess) err = hipGetLastError();
  if (err == hipSuccess) err = hipEventRecord(e1, ctx->stream);
  if (err == hipSuccess) err = hipEventSynchronize(e1);
  float ms = 0;
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  CXK_TRY(err);
  ctx->sparse_soc_setup_ms += ms;
  return CXK_SUCCESS;
}

// One pass over Q of a group of streamed quadratic cones: out_r = Q x_r for the R vectors of `x` (partials per
// column split; QuadStreamQx adds them).  Nothing to do where Q is the identity.
template <int R>
hipError_t LaunchQuadStreamQmv(const QuadStreamGroup& d, const QuadStreamVecs& x, hipStream_t st) {
  if (!d.Q) return hipSuccess;
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

// The Schur complement of a group of streamed quadratic cones: Q w1, the scalars, the columns, the block.
hipError_t LaunchQuadStreamSchur(Group& g, const Arena& ar, hipStream_t st) {
  const QuadStreamGroup d = MakeQuadStream(g);
  const int cnt = d.count, m = d.m;
  hipError_t e = LaunchQuadStreamQmv<1>(d, QuadStreamOne(d.W + 1, (size_t)d.n + 1), st);
  if (e != hipSuccess) return e;
  quad_stream_schur_vectors<<<cnt, kQuadStreamBlock, 0, st>>>(d);
  if (m > 0) quad_stream_schur_columns<<<(unsigned)((size_t)cnt * m), kQuadStreamBlock, 0, st>>>(d);
  const int blocks = (int)std::max<size_t>(1, ((size_t)m * m + kQuadStreamBlock - 1) / kQuadStreamBlock);
  quad_stream_schur_finish<<<(unsigned)((size_t)cnt * blocks), kQuadStreamBlock, 0, st>>>(d, ar, blocks);
  return hipGetLastError();
}

// The constants of a group of streamed quadratic cones, once at cxk_finalize, on the device: Qc1 = Q c1 and
// c1' Q c1 by the pass kernel, A_gram = A1' (Q A1) as two batched GEMMs (A1 = A + 1 with leading dimension
// n + 1; T = Q A1 in a buffer that lives for this call only).
int QuadStreamConstants(cxk_context* ctx, Group& g) {
  const QuadStreamGroup d = MakeQuadStream(g);
  const int cnt = d.count, n = d.n, m = d.m, len = n + 1;
  CXK_TRY(LaunchQuadStreamQmv<1>(d, QuadStreamOne(d.c + 1, (size_t)len), ctx->stream));
  quad_stream_constants<<<cnt, kQuadStreamBlock, 0, ctx->stream>>>(d);
  CXK_TRY(hipGetLastError());
  DevBuf<double> T;
  if (g.has_q && m > 0) CXK_TRY(T.alloc((size_t)cnt * n * m));
  constexpr int kMaxBatch = 65535;  // gridDim.z
  for (int b0 = 0; b0 < cnt && m > 0; b0 += kMaxBatch) {
    const int nb = std::min(kMaxBatch, cnt - b0);
    const double* A1 = g.A.p + (size_t)b0 * len * m + 1;
    GemmArgs a{};
    a.inner = 1;
    a.alpha = 1.0;
    a.beta = 0.0;
    a.splits = 1;
    if (g.has_q) {  // T = Q A1
      a.M = n;
      a.N = m;
      a.K = n;
      a.A = g.qQ.p + (size_t)b0 * n * n;
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
    a.B = g.has_q ? T.p + (size_t)b0 * n * m : A1;
    a.ldb = g.has_q ? n : len;
    a.sB1 = g.has_q ? (int64_t)n * m : (int64_t)len * m;
    a.C = g.qGram.p + (size_t)b0 * m * m;
    a.ldc = m;
    a.sC1 = (int64_t)m * m;
    CXK_TRY(LaunchGemm(a, true, false, nb, ctx->stream));
  }
  CXK_TRY(hipStreamSynchronize(ctx->stream));  // (T is released on return)
  return CXK_SUCCESS;
}

// A hipEvent pair for this launch of a clock slot's kernels, when it is one of the sampled ones.
bool ClockSample(cxk_context* ctx, int slot, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!ctx->timing || (ctx->timing_tick[slot]++ % ctx->timing_period) != 0) return false;
  if (ctx->ev_used == ctx->ev_pool.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return false;
    if (hipEventCreate(&b) != hipSuccess) {
      (void)hipEventDestroy(a);
      return false;
    }
    ctx->ev_pool.emplace_back(a, b);
    ctx->ev_slot.push_back(slot);
  }
  *e0 = ctx->ev_pool[ctx->ev_used].first;
  *e1 = ctx->ev_pool[ctx->ev_used].second;
  ctx->ev_slot[ctx->ev_used] = slot;
  ctx->ev_used++;
  return true;
}

namespace {
// Kernel clocks (CXK_CLOCK_*): a slot whose launches are ONE register kernel carries the event pair on that
// dispatch; anything else is bracketed by event records around its launches.
struct StepClock {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool sample = false, on_dispatch = false;
};
StepClock BeginStepClock(cxk_context* ctx, int slot, bool one_register_kernel) {
  StepClock c;
  c.sample = ClockSample(ctx, slot, &c.e0, &c.e1);
  c.on_dispatch = c.sample && one_register_kernel;
  if (c.sample && !c.on_dispatch) (void)hipEventRecord(c.e0, ctx->stream);
  return c;
}
void EndStepClock(cxk_context* ctx, const StepClock& c) {
  if (c.sample && !c.on_dispatch) (void)hipEventRecord(c.e1, ctx->stream);
}
// The assembly clock around the launches of one group, for the scope it is declared in.
struct AssemblyClock {
  cxk_context* ctx;
  StepClock clk;
  explicit AssemblyClock(cxk_context* c, bool on_dispatch = false) : ctx(c), clk(BeginStepClock(c, CXK_CLOCK_ASSEMBLY, on_dispatch)) {}
  ~AssemblyClock() { EndStepClock(ctx, clk); }
};
}  // namespace

// The Schur complement of a group of dense LMIs, on the instance LmiSchurKernel names.
static int LaunchLmiDenseSchur(cxk_context* ctx, Group& g, const Arena& ar) {
  const LmiKernel kern = LmiSchurKernel(g);
  // (lmi_schur_mfma carries the pair on its dispatch instead: no marker packets)
  const AssemblyClock clock(ctx, IsSchurMfma(kern));
  if (IsSchurGemm(kern)) {
    CXK_TRY(LmiLargeSchur(MakeLmi(g), ar, MakeLargeWs(g), ctx->stream));
  } else if (IsSchurMfma(kern)) {
    LmiGroup lg = MakeLmi(g);
    if (g.Apad.p) {  // the order runs on the next instance up (masked W loads in the kernel)
      const int np = LmiMfmaPaddedOrder(g.n);
      lg.A = g.Apad.p;
      lg.a_stride = (long long)(g.m + 1) * np * np;
    }
    // every other launch of the group last to first: a launch then starts on the operands the previous one
    // ended with, which shortens its fill (the results are the same bits either way)
    const int rev = ctx->lmi_order_forward ? 0 : (int)(g.schur_launches & 1);
    g.schur_launches++;
    CXK_TRY(LaunchLmiSchurMfma(lg, ar, ctx->cus, rev, ctx->stream, clock.clk.e0, clock.clk.e1));
  } else {
    lmi_schur_generic<<<(int)g.ids.size(), 256, LmiGenericLds(g.n), ctx->stream>>>(MakeLmi(g), ar);
  }
  return CXK_SUCCESS;
}

// The Schur complement of a group of second-order cones on the LDS route: one wavefront per cone, up to four cones per
// workgroup; the cone's data staged in LDS when four staged images fit, read in place otherwise.
static void LaunchSocLdsSchur(cxk_context* ctx, Group& g, const Arena& ar) {
  const int count = (int)g.ids.size();
  const size_t staged = SocSchurLds(g.n, g.m, true), plain = SocSchurLds(g.n, g.m, false);
  if (4 * staged <= kLdsLimit) {
    soc_schur<true><<<(count + 3) / 4, 256, 4 * staged, ctx->stream>>>(MakeVec(g), ar);
  } else {
    const int w = (int)std::max<size_t>(1, std::min<size_t>(4, kLdsLimit / plain));
    soc_schur<false><<<(count + w - 1) / w, 64 * w, w * plain, ctx->stream>>>(MakeVec(g), ar);
  }
}

// The routes of more than one launch, and both quadratic ones (tools/quad_stream_speed.py compares them), carry the
// assembly clock when timing is on.
int LaunchSchur(cxk_context* ctx) {
  Arena ar = MakeArena(ctx);
  hipStream_t st = ctx->stream;
  for (Group& g : ctx->groups) {
    const int count = (int)g.ids.size();
    if (count == 0) continue;
    switch (g.route) {
      case ConeRoute::kLmiDense: if (LaunchLmiDenseSchur(ctx, g, ar)) return CXK_FAILURE; break;
      case ConeRoute::kLmiSparse: { const AssemblyClock clock(ctx); CXK_TRY(LaunchLmiSchurSparse(g, LmiSchurKernel(g), ar, st)); break; }
      case ConeRoute::kLmiFactored: { const AssemblyClock clock(ctx); CXK_TRY(LmiFactoredSchur(MakeLmi(g), MakeLmiFactored(g), ar, MakeLargeWs(g), st)); break; }
      case ConeRoute::kLinearLds: linear_schur<<<count, 256, 0, st>>>(MakeVec(g), ar); break;
      case ConeRoute::kLinearTiled: { const AssemblyClock clock(ctx); CXK_TRY(LaunchLinearTiledSchur(g, ar, st)); break; }
      case ConeRoute::kLinearSparse: { const AssemblyClock clock(ctx); CXK_TRY(LaunchLinearSparseSchur(g, ar, st)); break; }
      case ConeRoute::kSocLds: LaunchSocLdsSchur(ctx, g, ar); break;
      case ConeRoute::kSocStreamed: { const AssemblyClock clock(ctx); CXK_TRY(LaunchSocStreamSchur(g, ar, st)); break; }
      case ConeRoute::kSocSparse: { const AssemblyClock clock(ctx); CXK_TRY(LaunchSocSparseSchur(g, ar, st)); break; }
      case ConeRoute::kQuadLds: { const AssemblyClock clock(ctx); quad_schur<<<count, 64, QuadSchurLds(g.n, g.m), st>>>(MakeQuad(g), ar); break; }
      case ConeRoute::kQuadStreamed: { const AssemblyClock clock(ctx); CXK_TRY(LaunchQuadStreamSchur(g, ar, st)); break; }
      case ConeRoute::kStatic: static_schur<<<count, 64, 0, st>>>(MakeStatic(g), ar); break;
      case ConeRoute::kOct: oct_schur<<<count, 64, 0, st>>>(MakeOct(g), ar); break;
    }
  }
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// The nonzeros (v != 0.0) of a dense-added linear block (rows = n) or second-order cone (rows = n + 1), by rows,
// columns ascending.
static void LinearNonzeros(ConstraintRec* c) {
  const size_t rows = (size_t)c->n + (c->type == CXK_SOC ? 1 : 0);
  c->sp_rowptr.assign(rows + 1, 0);
  for (int j = 0; j < c->m; j++)
    for (size_t r = 0; r < rows; r++) c->sp_rowptr[r + 1] += c->A[r + (size_t)j * rows] != 0.0;
  for (size_t r = 0; r < rows; r++) c->sp_rowptr[r + 1] += c->sp_rowptr[r];
  c->sp_col.resize((size_t)c->sp_rowptr[rows]);
  c->sp_val.resize((size_t)c->sp_rowptr[rows]);
  std::vector<int> next(c->sp_rowptr.begin(), c->sp_rowptr.end() - 1);
  for (int j = 0; j < c->m; j++)
    for (size_t r = 0; r < rows; r++) {
      const double v = c->A[r + (size_t)j * rows];
      if (v != 0.0) {
        c->sp_col[(size_t)next[r]] = j;
        c->sp_val[(size_t)next[r]++] = v;
      }
    }
}

// The device copy of a group of linear blocks (rows = n) or second-order cones (rows = n + 1) on the sparse route:
// every member's nonzeros by rows and by columns.
static int UploadSparseNonzeros(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), rows = (size_t)g.n + (g.type == CXK_SOC ? 1 : 0), m = (size_t)g.m;
  size_t total = 0;
  for (size_t k = 0; k < cnt; k++) total += ctx->cons[g.ids[k]].sp_col.size();
  CXK_DEMAND(total <= (size_t)INT_MAX, g.type == CXK_SOC
                                           ? "a group of sparse second-order cones with more than 2^31 nonzeros is not supported"
                                           : "a group of sparse linear blocks with more than 2^31 nonzeros is not supported");
  std::vector<int> eptr(cnt + 1, 0), rowptr(cnt * (rows + 1)), colptr(cnt * (m + 1), 0), col(total), crow(total);
  std::vector<double> val(total), cval(total);
  for (size_t k = 0; k < cnt; k++) {
    const ConstraintRec& c = ctx->cons[g.ids[k]];
    const size_t base = (size_t)eptr[k];
    eptr[k + 1] = (int)(base + c.sp_col.size());
    std::copy(c.sp_rowptr.begin(), c.sp_rowptr.end(), rowptr.begin() + k * (rows + 1));
    std::copy(c.sp_col.begin(), c.sp_col.end(), col.begin() + base);
    std::copy(c.sp_val.begin(), c.sp_val.end(), val.begin() + base);
    int* cp = colptr.data() + k * (m + 1);
    for (int v : c.sp_col) cp[v + 1]++;
    for (size_t j = 0; j < m; j++) cp[j + 1] += cp[j];
    std::vector<int> next(cp, cp + m);
    for (size_t r = 0; r < rows; r++)  // (rows in order: every column's rows come out ascending)
      for (int s = c.sp_rowptr[r]; s < c.sp_rowptr[r + 1]; s++) {
        const size_t at = base + (size_t)next[(size_t)c.sp_col[(size_t)s]]++;
        crow[at] = (int)r;
        cval[at] = c.sp_val[(size_t)s];
      }
  }
  CXK_TRY(g.ls_eptr.upload(eptr));
  CXK_TRY(g.ls_rowptr.upload(rowptr));
  CXK_TRY(g.ls_col.upload(col));
  CXK_TRY(g.ls_val.upload(val));
  CXK_TRY(g.ls_colptr.upload(colptr));
  CXK_TRY(g.ls_crow.upload(crow));
  CXK_TRY(g.ls_cval.upload(cval));
  return CXK_SUCCESS;
}

// The nonzero statistics Choose asks for, of a dense-added linear block (rows = n) or second-order cone (rows = n + 1)
// whose sparse mode is not 0; and the nonzeros themselves (LinearNonzeros) when ints can point at them.
static void MeasureNonzeros(ConstraintRec* c, ConeShape* s) {
  if (c->sp_rowptr.empty()) {
    size_t nnz = 0;
    for (double v : c->A) nnz += v != 0.0;
    s->nnz = (double)nnz;
    s->nnz_fits_int = nnz <= (size_t)INT_MAX;
    if (!s->nnz_fits_int) return;
    LinearNonzeros(c);
  }
  s->nnz = (double)c->sp_col.size();
  for (size_t r = 0; r + 1 < c->sp_rowptr.size(); r++) {
    const double nz = c->sp_rowptr[r + 1] - c->sp_rowptr[r];
    s->sum_nnz_sq += nz * nz;
  }
  std::vector<int> per_col((size_t)c->m, 0);
  for (int v : c->sp_col) per_col[(size_t)v]++;
  s->longest_column = c->m ? *std::max_element(per_col.begin(), per_col.end()) : 0;
}

// cxk_finalize, per-group stages.  Every owned constraint gets its route (cone_route.h: Choose, or the refusal
// cxk_finalize fails with); constraints of one shape on one route form a group, numbered by first appearance.
int GroupConstraints(cxk_context* ctx, const FinalizeSwitches& sw) {
  const int K = (int)ctx->cons.size();
  std::map<std::tuple<int, int, int, int, ConeRoute, bool, bool, int>, int> gmap;
  ctx->groups.clear();
  ctx->sparse_soc_setup_ms = 0;
  // what the context was told (-1 / -2: nothing) goes in front of the environment's word
  RouteModes modes = sw.modes;
  if (ctx->streamed_cones >= 0) modes.streamed_cones = ctx->streamed_cones != 0;
  if (ctx->tiled_linear >= 0) modes.tiled_linear = ctx->tiled_linear;
  if (ctx->streamed_quadratic != -2) modes.streamed_quadratic = ctx->streamed_quadratic;
  if (ctx->sparse_linear != -2) modes.sparse_linear = ctx->sparse_linear;
  if (ctx->sparse_soc != -2) modes.sparse_soc = ctx->sparse_soc;
  for (int i = 0; i < K; i++) {
    ConstraintRec& c = ctx->cons[i];
    c.route = ConeRoute::kStatic;
    if (!ctx->owned[i]) continue;
    ConeShape s{c.type, c.n, c.m, c.herm_d, c.symmetric, c.csr_only, c.factored, c.type == CXK_QUAD && !c.Q.empty()};
    const int sparse_mode = c.type == CXK_LINEAR ? modes.sparse_linear : c.type == CXK_SOC ? modes.sparse_soc : 0;
    if (sparse_mode != 0 && !c.csr_only) MeasureNonzeros(&c, &s);
    if (c.type == CXK_LMI && !c.factored) {
      double nnz = 0;
      for (double v : c.A) nnz += (v != 0.0);
      s.mfma_supports = LmiMfmaSupports(c.n, c.m, c.herm_d);
      s.sparse_pays = LmiSparsePays(c.n, c.m, nnz, LmiLdsResident(c.n, c.m), s.mfma_supports);
    }
    const RouteChoice choice = Choose(s, modes);
    CXK_DEMAND(!choice.refusal, choice.refusal);
    c.route = choice.route;
    const bool literal = c.type == CXK_LMI && !c.symmetric;
    const int f_R = c.factored ? c.f_R : 0;
    const auto key = std::make_tuple(c.type, c.n, c.m, c.herm_d, c.route, literal, s.has_q, f_R);
    auto it = gmap.find(key);
    if (it == gmap.end()) {
      it = gmap.emplace(key, (int)ctx->groups.size()).first;
      Group& g = ctx->groups.emplace_back();
      g.type = c.type;
      g.n = c.n;
      g.m = c.m;
      g.herm_d = c.herm_d;
      g.route = c.route;
      g.literal = literal;
      g.has_q = s.has_q;
      g.f_R = f_R;
    }
    c.group = it->second;
    c.member = (int)ctx->groups[it->second].ids.size();
    ctx->groups[it->second].ids.push_back(i);
  }
  return CXK_SUCCESS;
}

// The device copy of one group's data in the layout its kernels read, and its work space: what every route shares,
// then the route's own stage (each beside the view of what it allocates, above).
int UploadGroup(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size();
  const GroupSizes sz = SizesOf(g);
  if (g.type == CXK_LMI) {
    const LmiAssemblyChoice a = ChooseLmiAssembly(g.route, g.n, g.m, cnt, g.literal, LmiMfmaSupports(g.n, g.m, g.herm_d),
                                                  sw.schur_generic, sw.gemm_min_n);
    g.large = a.large;
    g.assembly = a.assembly;
    const int wide = WideSpectrumMode(ctx, sw);
    if (g.large && (wide == 1 || (wide == -1 && g.n > LmiLargeSpectrumMaxOrder())))
      CXK_TRY(g.ws_wide.alloc(cnt * LmiWideDoubles(g.n, g.herm_d)));
    g.wide_reduce = g.n >= (sw.wide_reduce_min_order >= 0 ? sw.wide_reduce_min_order : kWideReduceMinOrder);
  }
  // the routes that hold their data as nonzeros or factors keep no dense copy of A on the device
  const bool dense_a = g.route != ConeRoute::kLmiSparse && g.route != ConeRoute::kLmiFactored &&
                       g.route != ConeRoute::kLinearSparse && g.route != ConeRoute::kSocSparse;
  if (UploadDenseData(ctx, g, dense_a ? sz.a : 0, sz.c)) return CXK_FAILURE;
  CXK_TRY(g.W.alloc(sz.w * cnt));
  CXK_TRY(g.T1.alloc(sz.w * cnt));
  CXK_TRY(g.T2.alloc(g.type == CXK_LINEAR ? sz.w * cnt : 0));
  CXK_TRY(g.dids.upload(g.ids));
  switch (g.route) {
    case ConeRoute::kLinearLds: case ConeRoute::kSocLds: case ConeRoute::kStatic: case ConeRoute::kOct:
      return CXK_SUCCESS;  // (the dense copy is all their kernels read)
    case ConeRoute::kLinearTiled: return UploadLinearTiled(ctx, g, sw);
    case ConeRoute::kLinearSparse: return UploadLinearSparse(ctx, g);
    case ConeRoute::kSocStreamed: return UploadSocStream(ctx, g, sw);
    case ConeRoute::kSocSparse: return UploadSocSparse(ctx, g);
    case ConeRoute::kQuadLds: return UploadQuadGram(ctx, g);
    case ConeRoute::kQuadStreamed: return UploadQuadStream(ctx, g, sw);
    case ConeRoute::kLmiDense: return UploadLmiDense(ctx, g, sw);
    case ConeRoute::kLmiSparse: return UploadLmiSparse(ctx, g);
    case ConeRoute::kLmiFactored: return UploadLmiFactored(ctx, g);
  }
  return CXK_SUCCESS;
}

int LaunchSetIdentity(cxk_context* ctx) {
  for (Group& g : ctx->groups) {
    const size_t cnt = g.ids.size();
    if (cnt == 0) continue;
    switch (g.route) {
      case ConeRoute::kLmiDense: case ConeRoute::kLmiSparse: case ConeRoute::kLmiFactored:
        lmi_set_identity<<<GridFor(cnt * g.n * g.n, 256), 256, 0, ctx->stream>>>(MakeLmi(g));
        break;
      case ConeRoute::kLinearLds: case ConeRoute::kLinearTiled: case ConeRoute::kLinearSparse:
        vec_set_identity<<<GridFor(cnt * (g.n + 1), 256), 256, 0, ctx->stream>>>(MakeVec(g), false);
        break;
      case ConeRoute::kSocLds: case ConeRoute::kSocStreamed: case ConeRoute::kSocSparse:
      case ConeRoute::kQuadLds: case ConeRoute::kQuadStreamed:
        vec_set_identity<<<GridFor(cnt * (g.n + 1), 256), 256, 0, ctx->stream>>>(MakeVec(g), true);
        break;
      case ConeRoute::kStatic: break;  // (no scaling point)
      case ConeRoute::kOct:
        oct_set_identity<<<GridFor(cnt * 8 * g.n * g.n, 256), 256, 0, ctx->stream>>>(MakeOct(g));
        break;
    }
  }
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

int LaunchLinearLineSearch(cxk_context* ctx, double dinf_upper_bound, double c_scaling) {
  LineSearchArgs a;
  a.y0 = ctx->y2.p;
  a.y1 = ctx->y.p;
  a.cl_ptr = ctx->cl_ptr.p;
  a.cl_perm = ctx->cl_perm.p;
  a.c0_weight = c_scaling * 0;
  a.c1_weight = c_scaling * 1;
  a.dinfmax = dinf_upper_bound;
  a.out = ctx->info2.p;
  for (Group& g : ctx->groups) {
    const int cnt = (int)g.ids.size();
    if (cnt == 0) continue;
    const int tiles = (g.n + kLinTiledRowTile - 1) / kLinTiledRowTile;
    switch (g.route) {
      case ConeRoute::kLinearLds:
        linear_line_search<<<cnt, 256, sizeof(double) * 2 * g.m, ctx->stream>>>(MakeVec(g), a);
        break;
      case ConeRoute::kLinearTiled: {
        const LinTiledGroup d = MakeLinTiled(g);
        linear_tiled_line_search<<<(unsigned)((size_t)cnt * tiles), kLinTiledBlock, 0, ctx->stream>>>(d, a, tiles);
        linear_tiled_line_finish<<<cnt, kLinTiledBlock, 0, ctx->stream>>>(d, a, tiles);
        break;
      }
      case ConeRoute::kLinearSparse: {
        const LinSparseGroup d = MakeLinSparse(g);
        linear_sparse_line_search<<<(unsigned)((size_t)cnt * tiles), kLinTiledBlock, 0, ctx->stream>>>(d, a, tiles);
        linear_tiled_line_finish<<<cnt, kLinTiledBlock, 0, ctx->stream>>>(d.t, a, tiles);
        break;
      }
      // the line search bounds the step by the linear constraints only
      case ConeRoute::kSocLds: case ConeRoute::kSocStreamed: case ConeRoute::kSocSparse:
      case ConeRoute::kQuadLds: case ConeRoute::kQuadStreamed:
      case ConeRoute::kLmiDense: case ConeRoute::kLmiSparse: case ConeRoute::kLmiFactored:
      case ConeRoute::kStatic: case ConeRoute::kOct:
        break;
    }
  }
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// The Newton direction from the three solutions of cxk_factor_solve_triple_async and the barrier parameter the
// device selected (cone_program.cc:409-411 by linearity).  YFromThree (lmi_types.h) is the one expression for it.
__global__ void newton_from_three(int n, const double* __restrict__ y3, long long st, const double* __restrict__ k_from,
                                  double* __restrict__ y) {
  const double k = k_from[0];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = YFromThree(y3, st, k, i);
}
int FlushDirection(cxk_context* ctx) {
  if (!ctx->y_deferred) return CXK_SUCCESS;
  ctx->y_deferred = false;
  const int N = ctx->md.N;
  newton_from_three<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, ctx->y3.p, (long long)N, ctx->mu_dev.p, ctx->y.p);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

}  // namespace cxk_host

// The mailbox helpers and ReduceStepInfoAndSync have C linkage, and libconex.so has always exported them under these
// names: they stay here, between the two halves of namespace cxk_host, so that the library's dynamic symbols do not
// change.  Do not fold them into the namespace.
extern "C" {

__global__ void mailbox_pack(MailboxArgs m) { MailboxPack(m); }

// The mailbox write of the next host round trip: as arguments of the kernel that produces the
// last results (reduce_step_info), or of mailbox_pack.
int NextMailbox(cxk_context* ctx, MailboxArgs* m) {
  if (!ctx->mb) {
    CXK_TRY(hipHostMalloc(reinterpret_cast<void**>(&ctx->mb), 16 * sizeof(double), hipHostMallocDefault));
    for (int i = 0; i < 16; i++) ctx->mb[i] = 0.0;
    ctx->mb[11] = -1.0;
  }
  m->red = ctx->red_out.p;
  m->scal = ctx->scal_out.p;
  m->fail = ctx->d_fail.p;
  m->tag = ctx->fail_tag;
  m->seq = (double)(++ctx->seq);
  m->mb = ctx->mb;
  m->mu = ctx->mu_dev.p;  // (null until the device has selected a barrier parameter)
  return CXK_SUCCESS;
}

// Waits until the mailbox carries sequence number `want`.
int WaitMailbox(cxk_context* ctx, long long want) {
  // spin on the sequence number (a stream synchronisation costs tens of microseconds of driver
  // wake-up); the stream is polled now and then so that a failed launch cannot hang the host.
  // The data slots are accepted only with a matching checksum (MailboxWrite): the bytes cross PCIe
  // as posted writes whose order of arrival is not relied upon.
  volatile double* flag = ctx->mb + 11;
  volatile unsigned long long* raw = reinterpret_cast<volatile unsigned long long*>(ctx->mb);
  static const bool no_spin = getenv("CXK_NO_SPIN") != nullptr;
  if (no_spin) CXK_TRY(hipStreamSynchronize(ctx->stream));
  double dw = (double)want;
  unsigned long long wbits;
  memcpy(&wbits, &dw, sizeof(wbits));
  bool synced = no_spin;
  for (unsigned spins = 1;; spins++) {
    if (*flag == dw) {
      unsigned long long snap[14], x = wbits;
      for (int i = 0; i <= 13; i++) {
        snap[i] = raw[i];
        if (i == 11 || i == 12) continue;  // sequence number, checksum
        const int r = MailboxRot(i);
        x ^= r ? (snap[i] << r) | (snap[i] >> (64 - r)) : snap[i];
      }
      if (x == snap[12] || synced) {
        memcpy(ctx->mbv, snap, sizeof(double) * 14);
        break;
      }
    }
    // (rarely: a stream query enqueues a marker behind the last command, and the next launch then
    // starts ~5.7 us late -- with a query every few thousand spins every iteration of conex::Solve paid that)
    if ((spins & 0xfffff) == 0 && hipStreamQuery(ctx->stream) != hipErrorNotReady) {
      CXK_TRY(hipStreamSynchronize(ctx->stream));  // everything has run: whatever is there now is final
      synced = true;
      if (*flag != dw) {  // (a launch failed: report what the mailbox holds)
        for (int i = 0; i <= 13; i++) ctx->mbv[i] = ctx->mb[i];
        break;
      }
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  ctx->mb_seen = want;
  return CXK_SUCCESS;
}

// Waits until everything enqueued so far has run and the mailbox carries its results.
int SyncMailbox(cxk_context* ctx) {
  MailboxArgs m;
  if (NextMailbox(ctx, &m)) return CXK_FAILURE;
  mailbox_pack<<<1, 64, 0, ctx->stream>>>(m);
  CXK_TRY(hipGetLastError());
  return WaitMailbox(ctx, ctx->seq);
}

// Whether TakeStep can read its step length from the device (every kernel of this program does).
bool TakeStepFromDeviceOk(const cxk_context* ctx) {
  if (ctx->world > 1 || ctx->use_ldlt) return false;
  for (const Group& g : ctx->groups)
    if (g.type == CXK_LMI && g.large && !g.ids.empty()) return false;  // its step argument kernel takes the value
  return true;
}

// reduce_step_info, then the host round trip: one launch on a single GPU (the results go to the
// mailbox from the reduction itself), reduction + all-reduces + mailbox_pack when sharded.
// take_e_weight != nullptr (mode 0): TakeStep with the step length of cone_program.cc:417-418 taken
// from the reduced norms ON THE DEVICE is enqueued before the host waits, *took reports it.
int ReduceStepInfoAndSync(cxk_context* ctx, int mode, const double* info, const double* take_e_weight = nullptr,
                          int* took = nullptr, bool tail_done = false, bool skip_on_fail = false, bool wait = true,
                          const MuRuleArgs* rule = nullptr) {
  MailboxArgs m;
  m.mb = nullptr;
  const bool fold = ctx->world <= 1;
  if (fold && !tail_done && NextMailbox(ctx, &m)) return CXK_FAILURE;
  const long long want = ctx->seq;
  if (!tail_done) {  // (else the launch's tail workgroup has reduced and written the mailbox: StepTail)
    MuRuleArgs r;
    r.on = 0;
    if (rule && mode == 1) r = *rule;  // (the selection of the barrier parameter rides in the reduction)
    reduce_step_info<<<1, 256, 0, ctx->stream>>>((int)ctx->cons.size(), mode, info, ctx->d_mask.p, ctx->red_out.p, m, r);
    CXK_TRY(hipGetLastError());
  }
  if (fold && take_e_weight && TakeStepFromDeviceOk(ctx)) {
    if (LaunchTakeStep(ctx, *take_e_weight, 1.0, ctx->red_out.p, skip_on_fail)) return CXK_FAILURE;
    if (took) *took = 1;
  }
  if (fold && !wait) return CXK_SUCCESS;  // (the results come back with a later mailbox)
  if (fold) return WaitMailbox(ctx, want);
  // sharded: every rank reduced its own constraints; ONE sum all-reduce of a (world x 4)-slot buffer
  // brings all partial results to every rank, which combines them in rank order (kernels_cone.hip.h:
  // sum / max for mode 0, min / max / sum / sum for mode 1 -- two or three collectives before)
  // (+ the time-out mark of the latest whole-tree launch: ShardMark)
  const size_t nslots = (size_t)4 * ctx->world + 1;
  if (ctx->step_slots.n != nslots) CXK_TRY(ctx->step_slots.alloc(nslots));
  step_slots_fill<<<1, 64, 0, ctx->stream>>>(ctx->rank, ctx->world, ctx->red_out.p, ctx->step_slots.p, ctx->d_fail.p,
                                             ctx->fx_flag ? ctx->shard_fused_tag : 0, ctx->fx_flag);
  CXK_TRY(hipGetLastError());
  if (ShardAllReduce(ctx, ctx->step_slots.p, nslots, kOpSum)) return CXK_FAILURE;
  step_slots_reduce<<<1, 64, 0, ctx->stream>>>(mode, ctx->world, ctx->step_slots.p, ctx->red_out.p, ctx->d_fail.p,
                                               ctx->shard_fused_tag);
  CXK_TRY(hipGetLastError());
  ctx->seq++;
  return SyncMailbox(ctx);
}

int cxk_lmi_kernels(const cxk_context* ctx, int constraint, int out[5]) {
  if (!ctx || !ctx->device_ready || !out || constraint < 0 || constraint >= (int)ctx->cons.size()) return CXK_FAILURE;
  const ConstraintRec& c = ctx->cons[constraint];
  if (c.type != CXK_LMI || c.factored || !ctx->owned[constraint]) return CXK_FAILURE;
  const Group& g = ctx->groups[c.group];
  out[CXK_LMI_STAGE_SCHUR] = LmiSchurKernel(g);
  out[CXK_LMI_STAGE_PREPARE] = LmiPrepareKernel(ctx, g, 0);
  out[CXK_LMI_STAGE_QUERY] = LmiPrepareKernel(ctx, g, 1);
  out[CXK_LMI_STAGE_TAKE] = LmiTakeKernel(g);
  out[CXK_LMI_STAGE_AFFINE] = LmiPrepareKernel(ctx, g, 2);
  return CXK_SUCCESS;
}

const char* cxk_lmi_kernel_name(int code) {
  return code >= 0 && code < kLmiKernelCount ? kLmiKernelNames[code] : nullptr;
}

int cxk_lmi_kernel_count(void) { return kLmiKernelCount; }

#ifdef CXK_DEBUG_STAMPS
int cxk_debug_sparse_stamps(long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sparse_stamp), 8 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
#endif

}  // extern "C"

namespace cxk_host {

// The tail workgroup (StepTail) serves a PrepareStep / eigenvalue query whose constraints ALL go
// through lmi_prepare_rows on one GPU: then the reduction, the step scalars and the mailbox write
// ride in that launch.  CXK_NO_STEP_TAIL=1 keeps the separate launches (tests compare both).
bool StepTailOk(const cxk_context* ctx, int affine) {
  if (ctx->no_step_tail || affine || ctx->world > 1 || ctx->use_ldlt) return false;
  const Group* only = nullptr;
  for (const Group& g : ctx->groups) {
    if (g.ids.empty()) continue;
    if (only) return false;
    only = &g;
  }
  return only && only->type == CXK_LMI && !only->large && !only->literal && only->ids.size() == ctx->cons.size() &&
         LmiPrepareRowsSupports(only->n, only->m, only->herm_d, only->route == ConeRoute::kLmiSparse);
}
namespace {
int MakeStepTail(cxk_context* ctx, int mode, StepTail* t) {
  const size_t K = ctx->cons.size();
  if (ctx->tail_slots.n != 8 * K) {  // two sets, used in turn
    double armed;
    const unsigned long long bits = kTailSentinel;
    memcpy(&armed, &bits, sizeof(armed));
    CXK_TRY(ctx->tail_slots.upload(std::vector<double>(8 * K, armed)));
    ctx->tail_parity = 0;
  }
  t->slots = ctx->tail_slots.p + (size_t)ctx->tail_parity * 4 * K;
  t->rearm = ctx->tail_slots.p + (size_t)(ctx->tail_parity ^ 1) * 4 * K;
  ctx->tail_parity ^= 1;
  t->K = (int)K;
  t->mode = mode;
  t->mask = ctx->d_mask.p;
  t->red_out = ctx->red_out.p;
  t->scal = (mode == 0 && ctx->scal_deferred) ? 1 : 0;
  t->N = ctx->md.N;
  t->b = ctx->b.p;
  t->AQc = ctx->AQc.p;
  t->y = ctx->y.p;
  t->ny = 0;
  t->y_out = nullptr;
  t->y_done = nullptr;
  t->y_target = 0;
  t->sys_sc = ctx->sys_sc.p;
  t->scal_out = ctx->scal_out.p;
  t->rule.on = 0;
  if (NextMailbox(ctx, &t->mbx)) return CXK_FAILURE;
  if (t->scal) {  // the scalars travel in this launch's mailbox
    ctx->scal_deferred = false;
    ctx->scal_seq = ctx->seq;
  }
  return CXK_SUCCESS;
}

int NonEmptyGroups(const cxk_context* ctx) {
  int n = 0;
  for (const Group& g : ctx->groups) n += !g.ids.empty();
  return n;
}
#define CXK_LAUNCH_CLOCKED(clk, kernel, grid, block, ...)                                                        \
  do {                                                                                                           \
    if ((clk).on_dispatch)                                                                                       \
      hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, ctx->stream, (clk).e0, (clk).e1, 0, __VA_ARGS__); \
    else                                                                                                         \
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, ctx->stream, __VA_ARGS__);                          \
  } while (0)
// The same instance of a stage whatever it serves: the query's and the affine update's codes as PrepareStep's.
LmiKernel AsPrepareKernel(LmiKernel k) {
  if (k >= kQueryRowsPacked && k <= kQueryLarge) return (LmiKernel)(k - kQueryRowsPacked + kPrepareRowsPacked);
  if (k >= kAffineGeneric20 && k <= kAffineLarge) return (LmiKernel)(k - kAffineGeneric20 + kPrepareGeneric20);
  return k;
}

// PrepareStep (MODE 0; pmode 0, or 2 for the affine update) or the eigenvalue query (MODE 1; pmode 1) of every
// group.  tail_blocks: what the tail workgroup adds to the grid of lmi_prepare_rows.
template <int MODE>
int LaunchPrepareGroups(cxk_context* ctx, int pmode, const StepArgs& sa, const StepTail& tail, int tail_blocks, int clock_slot) {
  bool rows_only = NonEmptyGroups(ctx) == 1;
  for (const Group& g : ctx->groups)
    if (!g.ids.empty())
      rows_only = rows_only && g.type == CXK_LMI && IsPrepareRows(LmiPrepareKernel(ctx, g, pmode));
  const StepClock clk = BeginStepClock(ctx, clock_slot, rows_only);
  for (Group& g : ctx->groups) {
    const int cnt = (int)g.ids.size();
    if (cnt == 0) continue;
    switch (g.route) {
      case ConeRoute::kLmiFactored:  // (`large`: the factored slack in front of the large-order kernels)
        CXK_TRY(LmiFactoredSlack(MakeLmi(g), MakeLmiFactored(g), sa, MakeLargeWs(g), ctx->stream));
        CXK_TRY(LmiLargeAfterSlack(MakeLmi(g), sa, MakeLargeWs(g), MODE, ctx->stream));
        break;
      case ConeRoute::kLmiDense: case ConeRoute::kLmiSparse:
        switch (AsPrepareKernel(LmiPrepareKernel(ctx, g, pmode))) {
          case kPrepareLarge:
            CXK_TRY(LmiLargePrepare(MakeLmi(g), sa, MakeLargeWs(g), MODE, ctx->stream));
            break;
          case kPrepareRowsPacked:
          case kPrepareRowsExact:  // (the instance reads g.Apk when there is one)
            CXK_LAUNCH_CLOCKED(clk, (lmi_prepare_rows<MODE, 20, true>), (cnt + 3) / 4 + tail_blocks, 256, MakeLmi(g), sa, tail);
            break;
          case kPrepareRowsOdd:
          case kPrepareRowsEven:  // (an order below 20 on the same instance)
            CXK_LAUNCH_CLOCKED(clk, (lmi_prepare_rows<MODE, 20, false>), (cnt + 3) / 4 + tail_blocks, 256, MakeLmi(g), sa, tail);
            break;
          case kPrepareGeneric20:
            lmi_prepare_generic<MODE, 20><<<cnt, 256, LmiPrepareLds(g.n, g.m), ctx->stream>>>(MakeLmi(g), sa);
            break;
          default:  // kPrepareGeneric
            lmi_prepare_generic<MODE, 0><<<cnt, 256, LmiPrepareLds(g.n, g.m), ctx->stream>>>(MakeLmi(g), sa);
            break;
        }
        break;
      case ConeRoute::kLinearLds: linear_prepare<MODE><<<cnt, 256, sizeof(double) * g.m, ctx->stream>>>(MakeVec(g), sa); break;
      case ConeRoute::kLinearTiled: {
        const LinTiledGroup d = MakeLinTiled(g);
        const int tiles = (g.n + kLinTiledRowTile - 1) / kLinTiledRowTile;
        linear_tiled_slack<MODE><<<(unsigned)((size_t)cnt * tiles), kLinTiledBlock, 0, ctx->stream>>>(d, sa, tiles);
        if (MODE == 1 || !sa.affine)  // (the affine update has no reduction)
          linear_tiled_finish<MODE><<<cnt, kLinTiledBlock, 0, ctx->stream>>>(d, sa, tiles);
        break;
      }
      case ConeRoute::kLinearSparse: {
        const LinSparseGroup d = MakeLinSparse(g);
        const int tiles = (g.n + kLinTiledRowTile - 1) / kLinTiledRowTile;
        linear_sparse_slack<MODE><<<(unsigned)((size_t)cnt * tiles), kLinTiledBlock, 0, ctx->stream>>>(d, sa, tiles);
        if (MODE == 1 || !sa.affine)  // (the affine update has no reduction)
          linear_tiled_finish<MODE><<<cnt, kLinTiledBlock, 0, ctx->stream>>>(d.t, sa, tiles);
        break;
      }
      case ConeRoute::kSocLds: soc_prepare<MODE><<<cnt, 64, SocPrepareLds(g.n, g.m), ctx->stream>>>(MakeVec(g), sa); break;
      case ConeRoute::kSocStreamed: {
        const SocStreamGroup d = MakeSocStream(g);
        const int tiles = (g.n + 1 + kSocStreamRowTile - 1) / kSocStreamRowTile;
        soc_stream_slack<<<(unsigned)((size_t)cnt * tiles), kSocStreamBlock, 0, ctx->stream>>>(d, sa, tiles);
        soc_stream_prepare<MODE><<<cnt, kSocStreamBlock, 0, ctx->stream>>>(d, sa);
        break;
      }
      case ConeRoute::kSocSparse: {
        const SocSparseGroup d = MakeSocSparse(g);
        const int tiles = (g.n + 1 + kSocStreamRowTile - 1) / kSocStreamRowTile;
        soc_sparse_slack<<<(unsigned)((size_t)cnt * tiles), kSocStreamBlock, 0, ctx->stream>>>(d, sa, tiles);
        soc_stream_prepare<MODE><<<cnt, kSocStreamBlock, 0, ctx->stream>>>(d.st, sa);
        break;
      }
      case ConeRoute::kQuadLds: quad_prepare<MODE><<<cnt, 64, QuadPrepareLds(g.n, g.m), ctx->stream>>>(MakeQuad(g), sa); break;
      case ConeRoute::kQuadStreamed: {
        const QuadStreamGroup d = MakeQuadStream(g);
        const int tiles = (g.n + 1 + kSocStreamRowTile - 1) / kSocStreamRowTile;
        soc_stream_slack<<<(unsigned)((size_t)cnt * tiles), kSocStreamBlock, 0, ctx->stream>>>(QuadStreamSlackView(g, d), sa, tiles);
        QuadStreamVecs x;  // Q [w1, ms1] in one pass
        x.p[0] = d.W + 1;
        x.p[1] = d.ms + 1;
        x.stride[0] = x.stride[1] = (size_t)g.n + 1;
        CXK_TRY(LaunchQuadStreamQmv<2>(d, x, ctx->stream));
        quad_stream_prepare_mid<MODE><<<cnt, kQuadStreamBlock, 0, ctx->stream>>>(d, sa);
        CXK_TRY(LaunchQuadStreamQmv<1>(d, QuadStreamOne(d.dv, (size_t)g.n), ctx->stream));
        quad_stream_prepare_finish<MODE><<<cnt, kQuadStreamBlock, 0, ctx->stream>>>(d, sa);
        break;
      }
      case ConeRoute::kStatic: break;  // (no cone: nothing to prepare)
      case ConeRoute::kOct: oct_prepare<MODE><<<cnt, 64, sizeof(double) * (size_t)g.m, ctx->stream>>>(MakeOct(g), sa); break;
    }
  }
  EndStepClock(ctx, clk);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}
}  // namespace

int PrepareStepImpl(cxk_context* ctx, int affine, double c_weight, double e_weight, double* info, bool take,
                           int* took, const double* cw_from, double cw_scale) {
  CXK_ENTER_KEEP(ctx);
  const bool with_tail = StepTailOk(ctx, affine);
  // A direction still in its three parts is combined inside this launch: the constraints' wavefronts form the
  // entries they read, a few workgroups more write y out, and the tail workgroup -- which needs all of y for the
  // step scalars -- waits for their count (newton_from_three, 5 us and a kernel boundary, rides along)
  const bool y_here = with_tail && ctx->y_deferred && !ctx->prepare_lds;
  if (FlushDeferred(ctx, with_tail, y_here)) return CXK_FAILURE;
  StepArgs sa = MakeStep(ctx, ctx->info2.p, affine, c_weight, e_weight, 1.0);
  if (y_here) {
    sa.y3 = ctx->y3.p;
    sa.y3_stride = ctx->md.N;
    sa.y3_k = ctx->mu_dev.p;
  }
  sa.cw_from = cw_from;  // (CWeightOf in every PrepareStep kernel)
  sa.cw_scale = cw_scale;

  // PrepareStep may be enqueued before the host has seen the factorization's outcome: the cones whose
  // PrepareStep changes the scaling point itself (second-order and quadratic cones leave w^{1/2} in W)
  // look at the flag and leave W as the reference does when Factor() failed
  sa.skip_if = ctx->d_fail.p;
  sa.skip_tag = ctx->fail_tag;
  StepTail tail;
  tail.slots = nullptr;
  if (with_tail && MakeStepTail(ctx, 0, &tail)) return CXK_FAILURE;
  if (y_here) {
    CXK_DEMAND(tail.slots, "internal error: no tail workgroup in the launch that combines the direction");
    if (ctx->y_done.n != 1) {
      CXK_TRY(ctx->y_done.alloc(1, true));
      ctx->y_done_target = 0;
    }
    tail.ny = (ctx->md.N + 255) / 256;
    tail.y_out = ctx->y.p;
    tail.y_done = ctx->y_done.p;
    ctx->y_done_target += (unsigned long long)tail.ny;
    tail.y_target = ctx->y_done_target;
    ctx->y_deferred = false;
  }
  ctx->lanczos_calls++;
  // (CXK_PREPARE_LDS at cxk_create, an A/B switch for tests and timing, keeps every group off the rows kernel)
  if (LaunchPrepareGroups<0>(ctx, affine ? 2 : 0, sa, tail, tail.slots ? 1 + tail.ny : 0, CXK_CLOCK_PREPARE)) return CXK_FAILURE;
  if (ctx->use_ldlt) {  // lambda_ = y.tail(rows) (equality_constraint.cc:32-37)
    ctx->y_at_prepare.resize(ctx->md.N);
    CXK_TRY(hipStreamSynchronize(ctx->stream));
    CXK_TRY(hipMemcpy(ctx->y_at_prepare.data(), ctx->y.p, sizeof(double) * ctx->md.N, hipMemcpyDeviceToHost));
  }
  if (affine) return CXK_SUCCESS;
  if (ReduceStepInfoAndSync(ctx, 0, ctx->info2.p, take ? &e_weight : nullptr, took, with_tail, cw_from != nullptr))
    return CXK_FAILURE;
  info[0] = ctx->mbv[0];
  info[1] = ctx->mbv[1];
  return CXK_SUCCESS;
}

int LaunchTakeStep(cxk_context* ctx, double e_weight, double step_size, const double* step_from,
                          bool skip_on_fail) {
  StepArgs sa = MakeStep(ctx, ctx->info2.p, 0, 0.0, e_weight, step_size);
  sa.step_from = step_from;
  if (skip_on_fail) {  // (TakeStep enqueued before the host has seen the factorization's outcome)
    sa.skip_if = ctx->d_fail.p;
    sa.skip_tag = ctx->fail_tag;
  }
  bool rows_only = NonEmptyGroups(ctx) == 1;
  for (const Group& g : ctx->groups)
    if (!g.ids.empty()) {
      const LmiKernel k = g.type == CXK_LMI ? LmiTakeKernel(g) : kTakeGeneric;
      rows_only = rows_only && IsTakeRows(k);
    }
  const StepClock clk = BeginStepClock(ctx, CXK_CLOCK_TAKE, rows_only);
  for (Group& g : ctx->groups) {
    const int cnt = (int)g.ids.size();
    if (cnt == 0) continue;
    const int blocks = (cnt + 3) / 4;
    switch (g.route) {
      case ConeRoute::kLmiDense: case ConeRoute::kLmiSparse: case ConeRoute::kLmiFactored:
        switch (LmiTakeKernel(g)) {
          case kTakeLargePade:
          case kTakeLargeTaylor:  // (Pade or Taylor by g.herm_d inside)
            CXK_TRY(LmiLargeTakeStep(MakeLmi(g), sa, MakeLargeWs(g), ctx->stream));
            break;
          case kTakeRows20:
          case kTakeRows20Pad:
            CXK_LAUNCH_CLOCKED(clk, (lmi_take_step_rows<20>), blocks, 256, MakeLmi(g), sa);
            break;
          case kTakeRows32:
          case kTakeRows32Pad:
            CXK_LAUNCH_CLOCKED(clk, (lmi_take_step_rows<32>), blocks, 256, MakeLmi(g), sa);
            break;
          case kTakeTaylor24:
          case kTakeTaylor24Pad:
            CXK_LAUNCH_CLOCKED(clk, (lmi_take_step_rows_taylor<24>), blocks, 256, MakeLmi(g), sa);
            break;
          case kTakeTaylor32:
          case kTakeTaylor32Pad:
            CXK_LAUNCH_CLOCKED(clk, (lmi_take_step_rows_taylor<32>), blocks, 256, MakeLmi(g), sa);
            break;
          case kTakeGeneric20:
            lmi_take_step_generic<20><<<cnt, 256, LmiTakeLds(g.n), ctx->stream>>>(MakeLmi(g), sa);
            break;
          default:  // kTakeGeneric
            lmi_take_step_generic<0><<<cnt, 256, LmiTakeLds(g.n), ctx->stream>>>(MakeLmi(g), sa);
            break;
        }
        break;
      case ConeRoute::kLinearLds: case ConeRoute::kLinearTiled: case ConeRoute::kLinearSparse:  // (W is a dense vector on each)
        linear_take_step<<<GridFor((size_t)cnt * g.n, 256), 256, 0, ctx->stream>>>(MakeVec(g), sa);
        break;
      case ConeRoute::kSocLds: soc_take_step<<<cnt, 64, SocTakeLds(g.n), ctx->stream>>>(MakeVec(g), sa); break;
      case ConeRoute::kSocStreamed: soc_stream_take_step<<<cnt, kSocStreamBlock, 0, ctx->stream>>>(MakeSocStream(g), sa); break;
      case ConeRoute::kSocSparse: soc_stream_take_step<<<cnt, kSocStreamBlock, 0, ctx->stream>>>(MakeSocSparse(g).st, sa); break;
      case ConeRoute::kQuadLds: quad_take_step<<<cnt, 64, QuadTakeLds(g.n), ctx->stream>>>(MakeQuad(g), sa); break;
      case ConeRoute::kQuadStreamed: quad_stream_take_step<<<cnt, kQuadStreamBlock, 0, ctx->stream>>>(MakeQuadStream(g), sa); break;
      case ConeRoute::kStatic: break;  // (no cone: no step)
      case ConeRoute::kOct: oct_take_step<<<cnt, 64, 0, ctx->stream>>>(MakeOct(g), sa); break;
    }
  }
  EndStepClock(ctx, clk);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// rule != nullptr: the selection of the barrier parameter rides in the launch's tail workgroup and
// nobody waits (cxk_select_mu_async)
int SlackEigenvaluesImpl(cxk_context* ctx, double c_weight, double* out, const MuRuleArgs* rule) {
  CXK_ENTER(ctx);
  StepArgs sa = MakeStep(ctx, ctx->info4.p, 0, c_weight, 0.0, 1.0);
  const bool with_tail = StepTailOk(ctx, 0);
  StepTail tail;
  tail.slots = nullptr;
  tail.rule.on = 0;
  if (with_tail && MakeStepTail(ctx, 1, &tail)) return CXK_FAILURE;
  if (rule) tail.rule = *rule;
  ctx->lanczos_calls++;
  if (LaunchPrepareGroups<1>(ctx, 1, sa, tail, tail.slots ? 1 : 0, CXK_CLOCK_QUERY)) return CXK_FAILURE;
  if (ReduceStepInfoAndSync(ctx, 1, ctx->info4.p, nullptr, nullptr, with_tail, false, rule == nullptr, rule))
    return CXK_FAILURE;
  if (out && !rule)
    for (int i = 0; i < 4; i++) out[i] = ctx->mbv[i];
  return CXK_SUCCESS;
}

int SelectMuAsync(cxk_context* ctx, double c_weight, double divergence_upper_bound, int rank, double prev, double lb,
                  double ub) {
  MuRuleArgs r;
  r.on = 1;
  r.u.divergence_upper_bound = divergence_upper_bound;
  r.u.rankK = rank;
  r.u.prev = prev;
  r.u.lb = lb;
  r.u.ub = ub;
  r.out = ctx->mu_dev.p;
  return SlackEigenvaluesImpl(ctx, c_weight, nullptr, &r);
}

}  // namespace cxk_host
