// Linear-inequality blocks on their three routes (kLinearLds, kLinearTiled, kLinearSparse): the views, the stages of
// cxk_finalize and every launch.  Owns the kernels of kernels_linear / _linear_tiled / _linear_sparse; the other
// vector cones reach vec_set_identity, the Gram product and the nonzero lists through the host functions here, which
// work on the GramWs / NonzeroLists they are handed.  The family's state is Group::lin (cone_state.h).
#include "cone_units.h"
#include "kernels_gemm.hip.h"
#include "kernels_linear.hip.h"
#include "kernels_linear_tiled.hip.h"
#include "kernels_linear_sparse.hip.h"

namespace cxk_host {

// ---- The views the kernels take of a group, each beside the stage of cxk_finalize that allocates what it lays out,
// so that a layout and its size are read together.  MakeVec is every vector cone's (len = n + 1 with a scalar part).
VecGroup MakeVec(Group& g) {
  VecGroup d;
  d.len = (g.type == CXK_SOC || g.type == CXK_QUAD) ? g.n + 1 : g.n;
  d.m = g.m;
  d.count = static_cast<int>(g.ids.size());
  d.A = g.A.p;
  d.c = g.C.p;
  d.W = g.W.p;
  d.T1 = g.T1.p;
  d.T2 = g.lin.T2.p;
  d.ids = g.dids.p;
  return d;
}
// The second temporary of the linear blocks' kernels, for every CXK_LINEAR group whatever its route (any other group
// keeps the one element of an empty buffer: MakeVec hands the pointer on).
int AllocLinearT2(cxk_context* ctx, Group& g) {
  CXK_TRY(g.lin.T2.alloc(g.type == CXK_LINEAR ? (size_t)g.n * g.ids.size() : 0));
  return CXK_SUCCESS;
}
// The work space of the Gram product of LaunchGramLower, for `cnt` streamed second-order cones (len = n + 1) or tiled
// linear blocks (len = n) alike: the scaled copy of A, the products, the split partials.
int AllocGramWorkspace(cxk_context* ctx, GramWs& w, size_t cnt, size_t len, size_t m, const FinalizeSwitches& sw) {
  w.splits = SocStreamSplits((int)len, (int)m, (long long)cnt);
  if (sw.gram_splits > 0) w.splits = sw.gram_splits;  // (comparison runs)
  CXK_TRY(w.WA.alloc(cnt * len * m));
  CXK_TRY(w.Gf.alloc(cnt * m * m));
  CXK_TRY(w.part.alloc(w.splits > 1 ? (size_t)w.splits * std::min<size_t>(cnt, 65535) * m * m : 0));
  return CXK_SUCCESS;
}
LinTiledGroup MakeLinTiled(Group& g) {
  LinTiledGroup d;
  d.v = MakeVec(g);
  d.WA = g.lin.gram.WA.p;
  d.Gf = g.lin.gram.Gf.p;
  d.part = g.lin.tile_part.p;
  return d;
}
int UploadLinearTiled(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size(), len = (size_t)g.n, m = (size_t)g.m, tiles = (len + kLinTiledRowTile - 1) / kLinTiledRowTile;
  CXK_DEMAND(cnt * std::max(m, tiles) <= (size_t)INT_MAX,
             "a group of tiled linear blocks with more than 2^31 columns or row tiles is not supported");
  if (AllocGramWorkspace(ctx, g.lin.gram, cnt, len, m, sw)) return CXK_FAILURE;
  CXK_TRY(g.lin.tile_part.alloc(cnt * tiles * 4));
  return CXK_SUCCESS;
}
LinSparseGroup MakeLinSparse(Group& g) {
  LinSparseGroup d;
  d.t = MakeLinTiled(g);  // (A is null, WA and Gf unused: the scalars and finish kernels read v and part only)
  const NonzeroLists& nz = g.lin.nz;
  d.eptr = nz.eptr.p;
  d.rowptr = nz.rowptr.p;
  d.col = nz.col.p;
  d.val = nz.val.p;
  d.colptr = nz.colptr.p;
  d.crow = nz.crow.p;
  d.cval = nz.cval.p;
  return d;
}
int UploadLinearSparse(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), len = (size_t)g.n, m = (size_t)g.m, tiles = (len + kLinTiledRowTile - 1) / kLinTiledRowTile;
  const size_t chunks = m <= (size_t)kLinSparseWaveCols ? 1 : (m + kLinSparseColChunk - 1) / kLinSparseColChunk;
  if (UploadSparseNonzeros(ctx, g, g.lin.nz)) return CXK_FAILURE;
  CXK_DEMAND(cnt * std::max(m * chunks, tiles) <= (size_t)INT_MAX,
             "a group of sparse linear blocks with more than 2^31 column chunks or row tiles is not supported");
  CXK_TRY(g.lin.tile_part.alloc(cnt * tiles * 4));
  return CXK_SUCCESS;
}

// The nonzeros (v != 0.0) of a dense-added linear block (rows = n) or second-order cone (rows = n + 1), by rows,
// columns ascending.
void LinearNonzeros(ConstraintRec* c) {
  const size_t rows = (size_t)c->n + (c->type == CXK_SOC ? 1 : 0);
  ConstraintRec::RowNonzeros& nz = c->rows;
  nz.ptr.assign(rows + 1, 0);
  for (int j = 0; j < c->m; j++)
    for (size_t r = 0; r < rows; r++) nz.ptr[r + 1] += c->A[r + (size_t)j * rows] != 0.0;
  for (size_t r = 0; r < rows; r++) nz.ptr[r + 1] += nz.ptr[r];
  nz.col.resize((size_t)nz.ptr[rows]);
  nz.val.resize((size_t)nz.ptr[rows]);
  std::vector<int> next(nz.ptr.begin(), nz.ptr.end() - 1);
  for (int j = 0; j < c->m; j++)
    for (size_t r = 0; r < rows; r++) {
      const double v = c->A[r + (size_t)j * rows];
      if (v != 0.0) {
        nz.col[(size_t)next[r]] = j;
        nz.val[(size_t)next[r]++] = v;
      }
    }
}

// The device copy of a group of linear blocks (rows = n), second-order cones on the sparse route or quadratic cones added
// by their nonzeros (rows = n + 1): every member's nonzeros by rows and by columns, into its family's lists.
int UploadSparseNonzeros(cxk_context* ctx, const Group& g, NonzeroLists& nz) {
  const size_t cnt = g.ids.size(), rows = (size_t)g.n + (g.type == CXK_LINEAR ? 0 : 1), m = (size_t)g.m;
  size_t total = 0;
  for (size_t k = 0; k < cnt; k++) total += ctx->cons[g.ids[k]].rows.col.size();
  CXK_DEMAND(total <= (size_t)INT_MAX, g.type == CXK_QUAD ? "a group of quadratic cones added by cxk_add_quadratic_csr with more than 2^31 nonzeros is not supported"
                                       : g.type == CXK_SOC ? "a group of sparse second-order cones with more than 2^31 nonzeros is not supported"
                                                           : "a group of sparse linear blocks with more than 2^31 nonzeros is not supported");
  std::vector<int> eptr(cnt + 1, 0), rowptr(cnt * (rows + 1)), colptr(cnt * (m + 1), 0), col(total), crow(total);
  std::vector<double> val(total), cval(total);
  for (size_t k = 0; k < cnt; k++) {
    const ConstraintRec::RowNonzeros& c = ctx->cons[g.ids[k]].rows;
    const size_t base = (size_t)eptr[k];
    eptr[k + 1] = (int)(base + c.col.size());
    std::copy(c.ptr.begin(), c.ptr.end(), rowptr.begin() + k * (rows + 1));
    std::copy(c.col.begin(), c.col.end(), col.begin() + base);
    std::copy(c.val.begin(), c.val.end(), val.begin() + base);
    int* cp = colptr.data() + k * (m + 1);
    for (int v : c.col) cp[v + 1]++;
    for (size_t j = 0; j < m; j++) cp[j + 1] += cp[j];
    std::vector<int> next(cp, cp + m);
    for (size_t r = 0; r < rows; r++)  // (rows in order: every column's rows come out ascending)
      for (int s = c.ptr[r]; s < c.ptr[r + 1]; s++) {
        const size_t at = base + (size_t)next[(size_t)c.col[(size_t)s]]++;
        crow[at] = (int)r;
        cval[at] = c.val[(size_t)s];
      }
  }
  CXK_TRY(nz.eptr.upload(eptr));
  CXK_TRY(nz.rowptr.upload(rowptr));
  CXK_TRY(nz.col.upload(col));
  CXK_TRY(nz.val.upload(val));
  CXK_TRY(nz.colptr.upload(colptr));
  CXK_TRY(nz.crow.upload(crow));
  CXK_TRY(nz.cval.upload(cval));
  return CXK_SUCCESS;
}

// Gf = alpha WA' WA of every member of a group (WA: len x m per member), lower triangles only: the batched GEMM with
// SYRK-shaped output, split along len when that is long (the work space of AllocGramWorkspace).
hipError_t LaunchGramLower(const GramWs& w, const double* WA, double* Gf, int cnt, int len, int m, double alpha, hipStream_t st) {
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
    a.splits = w.splits;
    a.sCs = (int64_t)std::min(cnt, kMaxBatch) * mm;
    const hipError_t e = LaunchGemmSplitK(a, true, false, nb, w.part.p, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The Schur complement of a group of linear blocks on the LDS route: one workgroup per block.
void LaunchLinearLdsSchur(Group& g, const Arena& ar, hipStream_t st) {
  linear_schur<<<(int)g.ids.size(), 256, 0, st>>>(MakeVec(g), ar);
}

// The Schur complement of a group of linear blocks on the tiled route: scalars, apply, Gram (LaunchGramLower,
// alpha = 1), mirror.  Stream order is the only dependency.
hipError_t LaunchLinearTiledSchur(Group& g, const Arena& ar, hipStream_t st) {
  const LinTiledGroup d = MakeLinTiled(g);
  const int cnt = d.v.count, len = d.v.len, m = d.v.m;
  linear_tiled_scalars<<<cnt, kLinTiledBlock, 0, st>>>(d, ar);
  if (m == 0) return hipGetLastError();
  linear_tiled_apply<<<(unsigned)((size_t)cnt * m), kLinTiledBlock, 0, st>>>(d, ar);
  const hipError_t e = LaunchGramLower(g.lin.gram, d.WA, d.Gf, cnt, len, m, 1.0, st);
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

// PrepareStep (MODE 0, with the affine update) or the eigenvalue query (MODE 1) of one group.
namespace {
template <int MODE>
int LinearPrepare(cxk_context* ctx, Group& g, const StepArgs& sa) {
  const int cnt = (int)g.ids.size();
  switch (g.route) {
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
    default: CXK_DEMAND(false, "internal error: not a route of the linear blocks");
  }
  return CXK_SUCCESS;
}
}  // namespace

int LaunchLinearPrepare(cxk_context* ctx, Group& g, int mode, const StepArgs& sa) {
  return mode == 0 ? LinearPrepare<0>(ctx, g, sa) : LinearPrepare<1>(ctx, g, sa);
}

void LaunchLinearTakeStep(Group& g, const StepArgs& sa, hipStream_t st) {  // (W is a dense vector on each route)
  linear_take_step<<<GridFor(g.ids.size() * g.n, 256), 256, 0, st>>>(MakeVec(g), sa);
}

// The bounds of one group's blocks on the line search's step (LaunchLinearLineSearch).
int LaunchLinearGroupLineSearch(cxk_context* ctx, Group& g, const LineSearchArgs& a) {
  const int cnt = (int)g.ids.size();
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
    default: CXK_DEMAND(false, "internal error: not a route of the linear blocks");
  }
  return CXK_SUCCESS;
}

// W = e of a group of vector cones; soc: second-order and quadratic cones, e = (1, 0, ..., 0).
void LaunchVecSetIdentity(Group& g, bool soc, hipStream_t st) {
  vec_set_identity<<<GridFor(g.ids.size() * (g.n + 1), 256), 256, 0, st>>>(MakeVec(g), soc);
}

}  // namespace cxk_host
