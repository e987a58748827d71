// Second-order cones on their three routes (kSocLds, kSocStreamed, kSocSparse): the views, the stages of cxk_finalize
// and every launch.  Owns the kernels of kernels_soc / _soc_stream / _soc_sparse; the streamed quadratic cones reach
// soc_stream_slack through LaunchSocStreamSlack, soc_sparse_slack through LaunchSocSparseSlack.  The family's state is Group::soc (cone_state.h).
#include "cone_units.h"
#include "kernels_soc.hip.h"
#include "kernels_soc_stream.hip.h"
#include "kernels_soc_sparse.hip.h"

namespace cxk_host {

// ---- The views the kernels take of a group, each beside the stage of cxk_finalize that allocates what it lays out,
// so that a layout and its size are read together.  What those stages call further down:
int SocSparseConstants(cxk_context* ctx, Group& g);
static int SocSparseGramChunks(int m);
static int SocSparseCombineTiles(int m);

SocStreamGroup MakeSocStream(Group& g) {
  SocStreamGroup d;
  const size_t per = g.ids.size() * ((size_t)g.n + 1);
  d.v = MakeVec(g);
  d.WA = g.soc.gram.WA.p;
  d.s = g.soc.vec.p;
  d.wc = g.soc.vec.p + per;
  d.ms = g.soc.vec.p + 2 * per;
  d.dets = g.soc.det.p;
  d.Gf = g.soc.gram.Gf.p;
  return d;
}
int UploadSocStream(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size(), len = (size_t)g.n + 1, m = (size_t)g.m;
  CXK_DEMAND(cnt * std::max<size_t>(m, (len + kSocStreamRowTile - 1) / kSocStreamRowTile) <= (size_t)INT_MAX,
             "a group of streamed second-order cones with more than 2^31 columns or row tiles is not supported");
  g.soc.stages = sw.soc_stream_stages;
  if (AllocGramWorkspace(ctx, g.soc.gram, cnt, len, m, sw)) return CXK_FAILURE;
  CXK_TRY(g.soc.vec.alloc(3 * cnt * len));
  CXK_TRY(g.soc.det.alloc(cnt));
  return CXK_SUCCESS;
}
SocSparseGroup MakeSocSparse(Group& g) {
  SocSparseGroup d{};
  const size_t cnt = g.ids.size(), len = (size_t)g.n + 1, m = (size_t)g.m;
  d.st.v = MakeVec(g);  // (A is null; WA, wc, dets and Gf stay null: the step kernels read v, s and ms only)
  double* p = g.soc.vec.p;  // (the layouts UploadSocSparse sizes: SocSparseVecDoubles, SocSparseConstDoubles)
  d.st.s = p;
  d.st.ms = (p += cnt * len);
  d.u = (p += cnt * len);
  d.scal = (p += cnt * m);
  p = g.soc.consts.p;
  d.H = p;
  d.h = (p += cnt * m * m);
  d.z = (p += cnt * m);
  const NonzeroLists& nz = g.soc.nz;
  d.eptr = nz.eptr.p;
  d.rowptr = nz.rowptr.p;
  d.col = nz.col.p;
  d.val = nz.val.p;
  d.colptr = nz.colptr.p;
  d.crow = nz.crow.p;
  d.cval = nz.cval.p;
  return d;
}
size_t SocSparseVecDoubles(size_t cnt, size_t len, size_t m) { return cnt * (2 * len + m + 2); }
size_t SocSparseConstDoubles(size_t cnt, size_t m) { return cnt * (m * m + m + 1); }
// A group of sparse second-order cones: the nonzeros, the work space, and the constants on the device (SocSparseConstants).
int UploadSocSparse(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), len = (size_t)g.n + 1, m = (size_t)g.m, tiles = (len + kSocStreamRowTile - 1) / kSocStreamRowTile;
  if (UploadSparseNonzeros(ctx, g, g.soc.nz)) return CXK_FAILURE;
  CXK_DEMAND(cnt * std::max(std::max(m * (size_t)SocSparseGramChunks(g.m), tiles), (size_t)SocSparseCombineTiles(g.m)) <=
                 (size_t)INT_MAX,
             "a group of sparse second-order cones with more than 2^31 column chunks, row tiles or tiles of the Schur "
             "block is not supported");
  CXK_TRY(g.soc.vec.alloc(SocSparseVecDoubles(cnt, len, m)));
  CXK_TRY(g.soc.consts.alloc(SocSparseConstDoubles(cnt, m)));
  return SocSparseConstants(ctx, g);
}

// Kernels of this unit that may be launched with more than the default 64 KB of dynamic LDS.
hipError_t RaiseSocLdsLimits() {
  return RaiseDynamicLds({
    reinterpret_cast<const void*>(&soc_schur<true>),
    reinterpret_cast<const void*>(&soc_schur<false>),
    // a long thin cone ((n + 1) x (m + 2) within LDS, n in the thousands) passes 64 KB in its step kernels too
    reinterpret_cast<const void*>(&soc_prepare<0>),
    reinterpret_cast<const void*>(&soc_prepare<1>),
    reinterpret_cast<const void*>(&soc_take_step),
  });
}

// The Schur complement of a group of second-order cones on the LDS route: one wavefront per cone, up to four cones per
// workgroup; the cone's data staged in LDS when four staged images fit, read in place otherwise.
void LaunchSocLdsSchur(cxk_context* ctx, Group& g, const Arena& ar) {
  const int count = (int)g.ids.size();
  const size_t staged = SocSchurLds(g.n, g.m, true), plain = SocSchurLds(g.n, g.m, false);
  if (4 * staged <= kLdsLimit) {
    soc_schur<true><<<(count + 3) / 4, 256, 4 * staged, ctx->stream>>>(MakeVec(g), ar);
  } else {
    const int w = (int)std::max<size_t>(1, std::min<size_t>(4, kLdsLimit / plain));
    soc_schur<false><<<(count + w - 1) / w, 64 * w, w * plain, ctx->stream>>>(MakeVec(g), ar);
  }
}

// The Schur complement of a group of streamed second-order cones: vectors, apply, Gram (LaunchGramLower, alpha = 2),
// mirror.  Stream order is the only dependency.
hipError_t LaunchSocStreamSchur(Group& g, const Arena& ar, hipStream_t st) {
  const SocStreamGroup d = MakeSocStream(g);
  const int cnt = d.v.count, len = d.v.len, m = d.v.m;
  soc_stream_vectors<<<cnt, kSocStreamBlock, 0, st>>>(d, ar);
  if (m == 0 || g.soc.stages == 1) return hipGetLastError();
  soc_stream_apply<<<(unsigned)((size_t)cnt * m), kSocStreamBlock, 0, st>>>(d, ar);
  if (g.soc.stages == 2) return hipGetLastError();
  const hipError_t e = LaunchGramLower(g.soc.gram, d.WA, d.Gf, cnt, len, m, 2.0, st);
  if (e != hipSuccess) return e;
  soc_stream_mirror<<<GridFor((size_t)cnt * m * m, kSocStreamBlock), kSocStreamBlock, 0, st>>>(d, ar);
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

// The slack of d.v's rows into d.ms, for the unit of the streamed quadratic cones (same layout, same formula).
void LaunchSocStreamSlack(const SocStreamGroup& d, const StepArgs& sa, hipStream_t st) {
  const int tiles = (d.v.len + kSocStreamRowTile - 1) / kSocStreamRowTile;
  soc_stream_slack<<<(unsigned)((size_t)d.v.count * tiles), kSocStreamBlock, 0, st>>>(d, sa, tiles);
}

// soc_sparse_slack serves a quadratic cone held by the nonzeros of A as it is (same rows, same formula): the view of
// such a group it reads, v and the lists by rows, and where the slack goes.
void LaunchSocSparseSlack(const VecGroup& v, double* ms, const NonzeroLists& nz, const StepArgs& sa, hipStream_t st) {
  SocSparseGroup d{};
  d.st.v = v;
  d.st.ms = ms;
  d.eptr = nz.eptr.p;
  d.rowptr = nz.rowptr.p;
  d.col = nz.col.p;
  d.val = nz.val.p;
  const int tiles = (v.len + kSocStreamRowTile - 1) / kSocStreamRowTile;
  soc_sparse_slack<<<(unsigned)((size_t)v.count * tiles), kSocStreamBlock, 0, st>>>(d, sa, tiles);
}

// PrepareStep (MODE 0) or the eigenvalue query (MODE 1) of one group.
namespace {
template <int MODE>
int SocPrepare(cxk_context* ctx, Group& g, const StepArgs& sa) {
  const int cnt = (int)g.ids.size();
  switch (g.route) {
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
    default: CXK_DEMAND(false, "internal error: not a route of the second-order cones");
  }
  return CXK_SUCCESS;
}
}  // namespace

int LaunchSocPrepare(cxk_context* ctx, Group& g, int mode, const StepArgs& sa) {
  return mode == 0 ? SocPrepare<0>(ctx, g, sa) : SocPrepare<1>(ctx, g, sa);
}

int LaunchSocTakeStep(cxk_context* ctx, Group& g, const StepArgs& sa) {
  const int cnt = (int)g.ids.size();
  switch (g.route) {
    case ConeRoute::kSocLds: soc_take_step<<<cnt, 64, SocTakeLds(g.n), ctx->stream>>>(MakeVec(g), sa); break;
    case ConeRoute::kSocStreamed: soc_stream_take_step<<<cnt, kSocStreamBlock, 0, ctx->stream>>>(MakeSocStream(g), sa); break;
    case ConeRoute::kSocSparse: soc_stream_take_step<<<cnt, kSocStreamBlock, 0, ctx->stream>>>(MakeSocSparse(g).st, sa); break;
    default: CXK_DEMAND(false, "internal error: not a route of the second-order cones");
  }
  return CXK_SUCCESS;
}

}  // namespace cxk_host
