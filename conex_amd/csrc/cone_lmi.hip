// Matrix inequalities on their three routes (kLmiDense, kLmiSparse, kLmiFactored): the views, the stages of
// cxk_finalize, the choosers that name the kernel instance of each stage, and every launch.  Owns the kernels of
// kernels_lmi / _lmi_sparse / _lmi_rows / _lmi_large / _lmi_wide / _lmi_factored.  The family's state is Group::lmi
// (cone_state.h).
#include "cone_units.h"
#include "kernels_gemm.hip.h"
#include "kernels_lmi.hip.h"
#include "lmi_fused_mfma.h"
#include "kernels_lmi_sparse.hip.h"
#include "kernels_lmi_rows.hip.h"
#include "kernels_lmi_large.hip.h"
#include "kernels_lmi_factored.hip.h"

namespace cxk_host {

// ---- The views the kernels take of a group, each beside the stage of cxk_finalize that allocates what it lays out,
// so that a layout and its size are read together.  What those stages call further down:
int UploadSparseLmi(cxk_context* ctx, Group& g);

LmiGroup MakeLmi(Group& g) {
  LmiGroup d;
  d.n = g.n;
  d.m = g.m;
  d.count = static_cast<int>(g.ids.size());
  d.A = g.A.p;
  d.a_stride = (long long)(g.lmi.assembly != LmiAssembly::kGeneric ? g.m + 1 : g.m) * g.n * g.n;
  d.C = g.C.p;
  d.W = g.W.p;
  d.T1 = g.T1.p;
  d.ids = g.dids.p;
  d.Apk = g.lmi.Apk.n ? g.lmi.Apk.p : nullptr;
  d.herm_d = g.herm_d;
  const bool sparse = g.route == ConeRoute::kLmiSparse;
  d.sp_eptr = sparse ? g.lmi.sp.eptr.p : nullptr;
  d.sp_erc = sparse ? g.lmi.sp.erc.p : nullptr;
  d.sp_pairs = sparse ? g.lmi.sp.pairs.p : nullptr;
  d.sp_eval = sparse ? g.lmi.sp.eval.p : nullptr;
  d.sp_pptr = sparse ? g.lmi.sp.pptr.p : nullptr;
  d.sp_pvar = sparse ? g.lmi.sp.pvar.p : nullptr;
  d.sp_pval = sparse ? g.lmi.sp.pval.p : nullptr;
  return d;
}
static int AllocGemmAssembly(cxk_context* ctx, Group& g, const FinalizeSwitches& sw);
// The three side copies of a dense LMI group's matrices: Apad (lmi_schur_mfma at a padded order), Aleft (the folded
// form of a Hermitian group on the GEMM assembly), Apk (the packed lower triangles of the slack pass); then the work
// space of the GEMM assembly (beside MakeLargeWs).
int UploadLmiDense(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size();
  if (g.lmi.assembly == LmiAssembly::kMfma && LmiMfmaPaddedOrder(g.n) != g.n && !(g.herm_d == 2 && g.n == 24)) {
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
    CXK_TRY(g.lmi.Apad.upload(hp));
  }
  if (g.herm_d > 1 && g.lmi.assembly == LmiAssembly::kGemm && !g.lmi.literal && !sw.no_herm_fold) {
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
    CXK_TRY(g.lmi.Aleft.upload(hl));
  }
  if (!g.lmi.literal && !sw.no_packed_slack && g.n == 20 && LmiPrepareRowsSupports(g.n, g.m, g.herm_d, false)) {
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
    CXK_TRY(g.lmi.Apk.upload(hp));
  }
  return g.lmi.assembly == LmiAssembly::kGemm ? AllocGemmAssembly(ctx, g, sw) : CXK_SUCCESS;
}
// A sparse LMI group: its entry lists, and beyond the LDS-resident shapes the large-order work space.
int UploadLmiSparse(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), nn = (size_t)g.n * g.n;
  if (UploadSparseLmi(ctx, g)) return CXK_FAILURE;
  if (g.lmi.large || !g.lmi.sp.small) {
    CXK_TRY(g.lmi.ws_main.alloc(cnt * 8 * nn));  // step temporaries; C W and W C W during assembly
    CXK_TRY(g.lmi.ws_part.alloc(cnt * 2 * kSparseCParts));
    CXK_TRY(g.lmi.ws_piv.alloc(cnt * (size_t)g.n));
  }
  return CXK_SUCCESS;
}
// Where a folded sparse group beyond the LDS-resident shapes keeps the projection of W onto the real representations
// during an assembly (lmi_fold_project): the last of the eight squares of ws_main, which the assembly leaves alone.
// (An LDS-resident group projects on its way into LDS.)
static double* FoldedW(Group& g) { return g.lmi.ws_main.p + g.ids.size() * 7 * (size_t)g.n * g.n; }

LmiLargeWs MakeLargeWs(Group& g) {
  LmiLargeWs w;
  const size_t cnt = g.ids.size(), nn = (size_t)g.n * g.n, m1 = (size_t)g.m + 1;
  w.P = g.lmi.ws_main.p;
  w.PT = g.lmi.ws_main.p + cnt * m1 * nn;
  w.tmp = g.lmi.ws_main.p;
  w.Gf = g.lmi.ws_gf.p;
  w.part = g.lmi.ws_part.p;
  w.piv = g.lmi.ws_piv.p;
  w.splits = g.lmi.splits;
  w.fold = g.lmi.Aleft.n ? g.n / g.herm_d : 0;
  w.Aleft = g.lmi.Aleft.p;
  w.wide = g.lmi.ws_wide.n ? g.lmi.ws_wide.p : nullptr;
  w.wide_reduce = g.lmi.wide_reduce;
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
  g.lmi.splits = std::max(1, std::min(std::max(1, ksteps / 4), (int)((512 + cnt * tiles - 1) / (cnt * tiles))));
  if (sw.gram_splits > 0) g.lmi.splits = sw.gram_splits;  // (comparison runs)
  CXK_TRY(g.lmi.ws_main.alloc(cnt * std::max(2 * m1 * nn, 8 * nn)));
  CXK_TRY(g.lmi.ws_gf.alloc(cnt * m1 * m1));
  CXK_TRY(g.lmi.ws_piv.alloc(cnt * (size_t)g.n));
  CXK_TRY(g.lmi.ws_part.alloc(g.lmi.splits > 1 ? (size_t)g.lmi.splits * cnt * m1 * m1 : 0));
  return CXK_SUCCESS;
}

int LmiLargeSpectrumMaxOrder() {
  int n = 1;
  while (LmiLargeSpectrumLds(n + 1) <= kLdsLimit) n++;
  return n;
}

LmiFactoredGroup MakeLmiFactored(Group& g) {
  LmiFactoredGroup f{};
  const size_t cnt = g.ids.size(), nr = (size_t)g.n * g.lmi.f.R;
  f.R = g.lmi.f.R;
  f.d = g.herm_d > 1 ? g.herm_d : 1;
  f.rank_one = g.lmi.f.rank_one;
  f.F = g.lmi.f.F.p;
  f.sigma = g.lmi.f.sigma.p;
  f.ptr = g.lmi.f.ptr.p;
  f.var = g.lmi.f.var.p;
  f.Z = g.lmi.f.ws.p;  // (the layout UploadLmiFactored sizes: LmiFactoredWsDoubles)
  f.Y = f.Z + cnt * nr;
  f.Fs = f.Y + cnt * nr;
  f.P = f.Fs + cnt * nr * f.d;
  f.part = g.lmi.ws_part.p;
  f.npart = kSparseCParts;
  return f;
}
// (d: the column blocks of a Hermitian member's L(F); Z and Y keep R columns, Fs and P have d R)
size_t LmiFactoredWsDoubles(size_t cnt, size_t n, size_t R, size_t d) { return cnt * ((2 + d) * n * R + d * R * R); }

// A group of LMIs given by factors: every member's F, sigma, column pointers and column -> variable map, the work
// space of the factored kernels and of the large-order step kernels behind them.
int UploadLmiFactored(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), n = (size_t)g.n, R = (size_t)g.lmi.f.R, m = (size_t)g.m;
  const size_t d = g.herm_d > 1 ? (size_t)g.herm_d : 1;  // (a Hermitian member's factors.F is L(F): n x dR)
  CXK_DEMAND(cnt <= 65535, "a group of more than 65535 equal-shaped factored LMIs is not supported");
  std::vector<double> hF(cnt * n * R * d), hs(cnt * R);
  std::vector<int> hp(cnt * (m + 1)), hv(cnt * R);
  g.lmi.f.rank_one = true;
  for (size_t k = 0; k < cnt; k++) {
    const ConstraintRec& c = ctx->cons[g.ids[k]];
    std::copy(c.factors.F.begin(), c.factors.F.end(), hF.begin() + k * n * R * d);
    std::copy(c.factors.sigma.begin(), c.factors.sigma.end(), hs.begin() + k * R);
    std::copy(c.factors.ptr.begin(), c.factors.ptr.end(), hp.begin() + k * (m + 1));
    for (size_t i = 0; i < m; i++) {
      g.lmi.f.rank_one = g.lmi.f.rank_one && c.factors.ptr[i + 1] - c.factors.ptr[i] == 1;
      for (int q = c.factors.ptr[i]; q < c.factors.ptr[i + 1]; q++) hv[k * R + (size_t)q] = (int)i;
    }
  }
  CXK_TRY(g.lmi.f.F.upload(hF));
  CXK_TRY(g.lmi.f.sigma.upload(hs));
  CXK_TRY(g.lmi.f.ptr.upload(hp));
  CXK_TRY(g.lmi.f.var.upload(hv));
  CXK_TRY(g.lmi.f.ws.alloc(LmiFactoredWsDoubles(cnt, n, R, d)));
  CXK_TRY(g.lmi.ws_main.alloc(cnt * 8 * n * n));  // step temporaries; C W and W C W during assembly
  CXK_TRY(g.lmi.ws_part.alloc(cnt * 2 * kSparseCParts));
  CXK_TRY(g.lmi.ws_piv.alloc(cnt * n));
  return CXK_SUCCESS;
}

// What Choose (cone_route.h) asks about an LMI added with its dense matrices.
void MeasureLmi(const ConstraintRec& c, ConeShape* s) {
  double nnz = c.csr_only ? (double)c.entries.ptr[c.m] : 0;  // (held by its nonzeros: A is empty)
  for (double v : c.A) nnz += (v != 0.0);
  s->mfma_supports = LmiMfmaSupports(c.n, c.m, c.herm_d);
  s->sparse_pays = LmiSparsePays(c.n, c.m, nnz, LmiLdsResident(c.n, c.m), s->mfma_supports);
}

// UploadGroup, ahead of the uploads: how the group's Schur complement is assembled (cone_route.h: ChooseLmiAssembly),
// whether it is `large`, and for a large group the work space of the chip-wide Lanczos run.
int PlanLmiGroup(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size();
  const LmiAssemblyChoice a = ChooseLmiAssembly(g.route, g.n, g.m, cnt, g.lmi.literal, LmiMfmaSupports(g.n, g.m, g.herm_d),
                                                sw.schur_generic, sw.gemm_min_n);
  g.lmi.large = a.large;
  g.lmi.assembly = a.assembly;
  const int wide = WideSpectrumMode(ctx, sw);
  if (g.lmi.large && (wide == 1 || (wide == -1 && g.n > LmiLargeSpectrumMaxOrder())))
    CXK_TRY(g.lmi.ws_wide.alloc(cnt * LmiWideDoubles(g.n, g.herm_d)));
  g.lmi.wide_reduce = g.n >= (sw.wide_reduce_min_order >= 0 ? sw.wide_reduce_min_order : kWideReduceMinOrder);
  return CXK_SUCCESS;
}

// What the C-ABI unit counts (cxk_count_lmi_kernel, cxk_count_wide_spectrum).
LmiAssembly LmiAssemblyOf(const Group& g) { return g.lmi.assembly; }
bool LmiOnWideSpectrum(const Group& g) { return g.lmi.ws_wide.n != 0; }

// StepTailOk: lmi_prepare_rows, the kernel that carries the tail workgroup, has an instance for the group's shape.
bool LmiRowsServePrepare(const Group& g) {
  return LmiPrepareRowsSupports(g.n, g.m, g.herm_d, g.route == ConeRoute::kLmiSparse);
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

// An instance that runs only where it was asked for (cxk_set_sparse_affine, cxk_add_lmi_coo) and is no row of the
// kernel matrix that [0, cxk_lmi_kernel_count()) lists: its code lies behind that range (kLmiKernelCount itself stays
// "not an instance"), and cxk_lmi_kernel_name knows it.  lmi_schur_sparse behind lmi_affine_wc / _x / _scalars.
constexpr LmiKernel kSchurSparseAffine = (LmiKernel)(kLmiKernelCount + 1);
constexpr const char* kSchurSparseAffineName = "lmi_schur_sparse hbm sparse-C";
// Likewise the folded forms of the five sparse instances (cxk_set_sparse_fold, cxk_add_hermitian_coo): the four listed
// ones in their order, then the one above.
constexpr LmiKernel kSchurSparseFolded = (LmiKernel)(kLmiKernelCount + 2);
constexpr int kSchurSparseFoldedCount = 5;
constexpr const char* kSchurSparseFoldedNames[kSchurSparseFoldedCount] = {
    "lmi_schur_sparse small folded", "lmi_schur_sparse small dense-C folded", "lmi_schur_sparse hbm folded",
    "lmi_schur_sparse hbm dense-C folded", "lmi_schur_sparse hbm sparse-C folded"};

bool IsSchurMfma(LmiKernel k) { return k >= kSchurMfma8 && k <= kSchurMfma24FoldedSingle; }
bool IsSchurGemm(LmiKernel k) { return k >= kSchurGemm && k <= kSchurGemmFoldedLargeSplit; }
bool IsSchurSparseFolded(LmiKernel k) { return k >= kSchurSparseFolded && k < kSchurSparseFolded + kSchurSparseFoldedCount; }
bool IsSchurSparse(LmiKernel k) {
  return (k >= kSchurSparseSmall && k <= kSchurSparseDenseC) || k == kSchurSparseAffine || IsSchurSparseFolded(k);
}
// the instance a folded one is the form of
LmiKernel UnfoldedSchurSparse(LmiKernel k) {
  if (!IsSchurSparseFolded(k)) return k;
  return k - kSchurSparseFolded == 4 ? kSchurSparseAffine : (LmiKernel)(kSchurSparseSmall + (k - kSchurSparseFolded));
}
bool IsPrepareRows(LmiKernel k) {
  return (k >= kPrepareRowsPacked && k <= kPrepareRowsEven) || (k >= kQueryRowsPacked && k <= kQueryRowsEven);
}
bool IsTakeRows(LmiKernel k) { return k >= kTakeRows20 && k <= kTakeTaylor32Pad; }

LmiKernel LmiSchurKernel(const Group& g) {
  // not one of the instances: a code outside the reported range, which no Is*() test accepts and
  // cxk_lmi_kernel_name has no name for (LaunchSchur switches on the route first, cxk_lmi_kernels refuses the constraint)
  if (g.route == ConeRoute::kLmiFactored) return kLmiKernelCount;
  if (g.route == ConeRoute::kLmiSparse && g.lmi.sp.fold)
    return (LmiKernel)(kSchurSparseFolded + (g.lmi.sa.on ? 4 : (g.lmi.sp.small ? 0 : 2) + (g.lmi.sp.cdense ? 1 : 0)));
  if (g.route == ConeRoute::kLmiSparse && g.lmi.sa.on) return kSchurSparseAffine;
  if (g.route == ConeRoute::kLmiSparse) return (LmiKernel)((g.lmi.sp.small ? kSchurSparseSmall : kSchurSparse) + (g.lmi.sp.cdense ? 1 : 0));
  if (g.lmi.assembly == LmiAssembly::kGemm) {  // (fold and split counts as LmiLargeSchur reads them: MakeLargeWs, LmiFoldedSplits)
    const bool fold = g.lmi.Aleft.n != 0;
    const int splits = fold ? LmiFoldedSplits(g.lmi.splits, g.n, g.n / g.herm_d) : g.lmi.splits;
    return (LmiKernel)(kSchurGemm + (fold ? 4 : 0) + (g.lmi.large ? 2 : 0) + (splits > 1 ? 1 : 0));
  }
  if (g.lmi.assembly == LmiAssembly::kMfma) {
    const LmiMfmaInstance inst = LmiMfmaChoose(g.n, g.m, g.herm_d);
    if (inst.folded) return inst.single ? kSchurMfma24FoldedSingle : kSchurMfma24Folded;
    const bool pad = g.lmi.Apad.p != nullptr;
    switch (inst.order) {
      case 8: return pad ? kSchurMfma8Pad : kSchurMfma8;
      case 12: return pad ? kSchurMfma12Pad : kSchurMfma12;
      case 16: return (LmiKernel)(kSchurMfma16 + (pad ? 2 : 0) + (inst.single ? 1 : 0));
      case 20: return (LmiKernel)(kSchurMfma20 + (pad ? 2 : 0) + (inst.single ? 1 : 0));
      default: return (LmiKernel)(kSchurMfma24 + (pad ? 2 : 0) + (inst.single ? 1 : 0));
    }
  }
  return g.lmi.literal ? kSchurGenericLiteral : kSchurGenericSym;
}

// mode 0 PrepareStep, 1 the eigenvalue query, 2 the affine update
LmiKernel LmiPrepareKernel(const cxk_context* ctx, const Group& g, int mode) {
  const int base = mode == 0 ? kPrepareRowsPacked : kQueryRowsPacked;
  if (g.lmi.large) return mode == 2 ? kAffineLarge : (LmiKernel)(base + 6);
  if (mode != 2 && !ctx->prepare_lds && !g.lmi.literal && LmiPrepareRowsSupports(g.n, g.m, g.herm_d, g.route == ConeRoute::kLmiSparse)) {
    if (g.n == 20) return (LmiKernel)(base + (g.lmi.Apk.p ? 0 : 1));
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
  if (g.lmi.large) return g.herm_d ? kTakeLargeTaylor : kTakeLargePade;
  if (LmiTakeStepRowsSupports(g.n) && !TakeStepLdsSwitch() && !g.lmi.literal) {
    if (g.herm_d == 0) return g.n <= 20 ? (g.n == 20 ? kTakeRows20 : kTakeRows20Pad) : (g.n == 32 ? kTakeRows32 : kTakeRows32Pad);
    return g.n <= 24 ? (g.n == 24 ? kTakeTaylor24 : kTakeTaylor24Pad) : (g.n == 32 ? kTakeTaylor32 : kTakeTaylor32Pad);
  }
  return g.n == 20 ? kTakeGeneric20 : kTakeGeneric;
}

bool LmiPrepareOnRows(const cxk_context* ctx, const Group& g, int pmode) { return IsPrepareRows(LmiPrepareKernel(ctx, g, pmode)); }
bool LmiTakeOnRows(const Group& g) { return IsTakeRows(LmiTakeKernel(g)); }

// Kernels of this unit that may be launched with more than the default 64 KB of dynamic LDS.
hipError_t RaiseLmiLdsLimits() {
  return RaiseDynamicLds({
    reinterpret_cast<const void*>(&lmi_schur_generic),
    reinterpret_cast<const void*>(&lmi_prepare_generic<0, 0>),
    reinterpret_cast<const void*>(&lmi_prepare_generic<1, 0>),
    reinterpret_cast<const void*>(&lmi_take_step_generic<0>),
  });
}

// The m + 1 entry lists of a constraint on the sparse route, both triangles, by column then row: as cxk_add_lmi_coo
// left them, or read off the dense matrices in that order (list m is C; ptr has m + 2 entries).
struct LmiLists {
  const int *ptr = nullptr, *rc = nullptr;
  const double* val = nullptr;
  std::vector<int> own_ptr, own_rc;
  std::vector<double> own_val;
  bool too_many = false;  // 2^31 nonzeros and more: no int points at them
};
static void ReadLmiLists(const ConstraintRec& c, LmiLists* L) {
  if (c.csr_only) {
    L->ptr = c.entries.ptr.data(), L->rc = c.entries.rc.data(), L->val = c.entries.val.data();
    return;
  }
  const int n = c.n, m = c.m;
  const size_t nn = (size_t)n * n;
  L->own_ptr.assign((size_t)m + 2, 0);
  for (int i = 0; i <= m; i++) {
    const double* M = i < m ? c.A.data() + (size_t)i * nn : c.C.data();
    for (int col = 0; col < n; col++)
      for (int row = 0; row < n; row++) {
        const double v = M[row + (size_t)col * n];
        if (v != 0.0) {
          L->own_rc.push_back(row | (col << 16));
          L->own_val.push_back(v);
        }
      }
    L->too_many = L->too_many || L->own_val.size() > (size_t)INT_MAX;
    L->own_ptr[(size_t)i + 1] = L->too_many ? L->own_ptr[i] : (int)L->own_val.size();
  }
  L->ptr = L->own_ptr.data(), L->rc = L->own_rc.data(), L->val = L->own_val.data();
}

// GroupConstraints: a constraint on kLmiSparse takes its affine term by C's nonzeros -- beyond the LDS-resident orders,
// with more than 64 of them (fewer ride in the pair sums as list m), when the mode says so.
bool LmiTakesSparseAffine(const ConstraintRec& c, int mode, double min_ratio) {
  if (mode == 0 || LmiLdsResident(c.n, c.m)) return false;
  size_t nnz_c = 0;
  if (c.csr_only)
    nnz_c = (size_t)(c.entries.ptr[c.m + 1] - c.entries.ptr[c.m]);
  else
    for (double v : c.C) nnz_c += (v != 0.0);
  if (nnz_c <= (size_t)kSparseAffineMinNnz) return false;
  if (mode == 1) return true;
  LmiLists L;
  ReadLmiLists(c, &L);
  if (L.too_many) return false;
  std::vector<int> pos(L.rc, L.rc + L.ptr[c.m + 1]);
  std::sort(pos.begin(), pos.end());
  const size_t npos = (size_t)(std::unique(pos.begin(), pos.end()) - pos.begin());
  return LmiSparseAffinePays(c.n, (double)nnz_c, (double)npos, min_ratio);
}

// What the kernels of the affine term by its nonzeros read (kernels_lmi_sparse.hip.h: SparseAffine): every member's C
// by columns, the positions P, and the slot there of every entry of the A_i and of C.  `erc` holds the group's A lists.
static int UploadSparseAffine(cxk_context* ctx, Group& g, const std::vector<LmiLists>& lists, const std::vector<int>& eptr) {
  const size_t cnt = g.ids.size();
  const int n = g.n, m = g.m, m1 = m + 1;
  CXK_DEMAND(cnt <= 65535, "a group of more than 65535 equal-shaped sparse LMIs with an affine term by its nonzeros is not supported");
  std::vector<int> cptr(cnt * ((size_t)n + 1), 0), crc, cslot, pptr(cnt + 1, 0), prc, eslot((size_t)eptr[cnt * m1], 0);
  std::vector<double> cval;
  g.lmi.sa.pmax = 0;
  for (size_t k = 0; k < cnt; k++) {
    const LmiLists& L = lists[k];
    std::vector<int> pos(L.rc, L.rc + L.ptr[m1]);
    std::sort(pos.begin(), pos.end());
    pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
    auto slot = [&pos](int rc) { return (int)(std::lower_bound(pos.begin(), pos.end(), rc) - pos.begin()); };
    for (int e = 0; e < L.ptr[m]; e++) eslot[(size_t)eptr[k * m1] + e] = slot(L.rc[e]);
    int* cp = cptr.data() + k * ((size_t)n + 1);
    int col = 0;
    cp[0] = (int)crc.size();
    for (int e = L.ptr[m]; e < L.ptr[m1]; e++) {  // (by column then row already)
      for (; col < (L.rc[e] >> 16); col++) cp[col + 1] = (int)crc.size();
      crc.push_back(L.rc[e]);
      cval.push_back(L.val[e]);
      cslot.push_back(slot(L.rc[e]));
    }
    for (; col < n; col++) cp[col + 1] = (int)crc.size();
    prc.insert(prc.end(), pos.begin(), pos.end());
    CXK_DEMAND(prc.size() < ((size_t)1 << 31) && crc.size() < ((size_t)1 << 31), "sparse LMI group: too many nonzeros");
    pptr[k + 1] = (int)prc.size();
    g.lmi.sa.pmax = std::max(g.lmi.sa.pmax, (int)pos.size());
  }
  CXK_TRY(g.lmi.sa.cptr.upload(cptr));
  CXK_TRY(g.lmi.sa.crc.upload(crc));
  CXK_TRY(g.lmi.sa.cslot.upload(cslot));
  CXK_TRY(g.lmi.sa.cval.upload(cval));
  CXK_TRY(g.lmi.sa.pptr.upload(pptr));
  CXK_TRY(g.lmi.sa.prc.upload(prc));
  CXK_TRY(g.lmi.sa.eslot.upload(eslot));
  return CXK_SUCCESS;
}

// Entry lists of a sparse LMI group (kernels_lmi_sparse.hip.h): matrix-major for the sums, position-major for the slack.
int UploadSparseLmi(cxk_context* ctx, Group& g) {
  const size_t cnt = g.ids.size(), nn = (size_t)g.n * g.n;
  const int n = g.n, m = g.m, m1 = m + 1;
  std::vector<LmiLists> lists(cnt);
  for (size_t k = 0; k < cnt; k++) {
    ReadLmiLists(ctx->cons[g.ids[k]], &lists[k]);
    CXK_DEMAND(!lists[k].too_many, "sparse LMI group: too many nonzeros");
  }
  // a dense affine term stays out of the pair sums (X = W C W is formed instead)
  g.lmi.sp.cdense = false;
  for (size_t k = 0; k < cnt; k++)
    if (lists[k].ptr[m1] - lists[k].ptr[m] > 64) g.lmi.sp.cdense = true;  // (C, C) alone would be nz^2 terms on one wavefront
  // a folded group (kernels_lmi_sparse.hip.h, "The folded sums"): within every list that joins the sums the entries of
  // the top block row, rows below n / herm_d, go first; both parts keep their order by column then row.  A dense C
  // stays as it is (its list is read by columns: UploadSparseAffine).  Everything below reads the reordered lists.
  std::vector<int> etop;
  if (g.lmi.sp.fold) {
    CXK_DEMAND(g.herm_d > 1, "internal error: only a Hermitian group over C or H folds its sums");
    const int n0 = n / g.herm_d;
    etop.assign(cnt * m1, 0);
    for (size_t k = 0; k < cnt; k++) {
      LmiLists& L = lists[k];
      std::vector<int> rc(L.rc, L.rc + L.ptr[m1]);
      std::vector<double> val(L.val, L.val + L.ptr[m1]);
      const std::vector<int> ptr(L.ptr, L.ptr + m1 + 1);
      for (int i = 0; i < (g.lmi.sp.cdense ? m : m1); i++) {
        int at = ptr[i];
        for (int pass = 0; pass < 2; pass++) {
          for (int e = ptr[i]; e < ptr[i + 1]; e++)
            if (((L.rc[e] & 0xffff) < n0) == (pass == 0)) rc[at] = L.rc[e], val[at++] = L.val[e];
          if (pass == 0) etop[k * m1 + i] = at - ptr[i];
        }
      }
      L.own_rc = std::move(rc), L.own_val = std::move(val), L.own_ptr = ptr;
      L.ptr = L.own_ptr.data(), L.rc = L.own_rc.data(), L.val = L.own_val.data();
    }
  }
  std::vector<int> eptr(cnt * m1 + 1, 0), erc, pptr(cnt * nn + 1, 0), pvar;
  std::vector<double> eval, pval;
  g.lmi.sp.emax = 0;
  for (size_t k = 0; k < cnt; k++) {
    const LmiLists& L = lists[k];
    for (int i = 0; i < m1; i++) {
      if (i < m || !g.lmi.sp.cdense) {
        erc.insert(erc.end(), L.rc + L.ptr[i], L.rc + L.ptr[i + 1]);
        eval.insert(eval.end(), L.val + L.ptr[i], L.val + L.ptr[i + 1]);
      }
      CXK_DEMAND(eval.size() < ((size_t)1 << 31), "sparse LMI group: too many nonzeros");
      eptr[k * m1 + i + 1] = (int)eval.size();
    }
    g.lmi.sp.emax = std::max(g.lmi.sp.emax, eptr[k * m1 + m1] - eptr[k * m1]);
    // position-major: the variables of a position in ascending order (the reference's order of i in sum_i y_i A_i)
    int* pp = pptr.data() + k * nn;
    const int base = (int)pval.size();
    for (int e = 0; e < L.ptr[m]; e++) pp[(size_t)(L.rc[e] & 0xffff) + (size_t)(L.rc[e] >> 16) * n + 1]++;
    pp[0] = base;
    for (size_t q = 0; q < nn; q++) pp[q + 1] += pp[q];
    pvar.resize(pval.size() + (size_t)L.ptr[m]);
    pval.resize(pvar.size());
    std::vector<int> fill(pp, pp + nn);
    for (int i = 0; i < m; i++)
      for (int e = L.ptr[i]; e < L.ptr[i + 1]; e++) {
        const int at = fill[(size_t)(L.rc[e] & 0xffff) + (size_t)(L.rc[e] >> 16) * n]++;
        pvar[at] = i;
        pval[at] = L.val[e];
      }
  }
  g.lmi.sp.small = !g.lmi.large && LmiSparseLds(n, m, true, g.lmi.sp.cdense, 0, g.lmi.sp.fold) <= kLdsLimit;
  // work split: lanes per pair from the average number of terms of a pair (each lane takes four
  // terms at a time); enough workgroups to fill the chip when the group is small
  // (a folded pair is top x full: 1 / herm_d of the terms)
  const double per_mat = cnt ? (double)eval.size() / (double)(cnt * m1) : 0.0;
  const double avg_terms = g.lmi.sp.fold ? per_mat * per_mat / g.herm_d : per_mat * per_mat;
  g.lmi.sp.lpp = avg_terms <= 8 ? 1 : avg_terms <= 64 ? 4 : avg_terms <= 1024 ? 16 : 64;
  const double pairs = 0.5 * m1 * (m1 + 1.0);
  const double per_block = (256.0 / g.lmi.sp.lpp) * 4.0;  // pairs one workgroup takes in stride
  int chunks = (int)std::ceil(pairs / per_block);
  const int cap = (int)std::max<size_t>(1, 2048 / std::max<size_t>(cnt, 1));
  g.lmi.sp.chunks = std::max(1, std::min(chunks, cap));
  {
    std::vector<int> pr;
    pr.reserve((size_t)m1 * (m1 + 1) / 2);
    for (int i = 0; i < m1; i++)
      for (int j = 0; j <= i; j++) pr.push_back(i | (j << 16));
    CXK_TRY(g.lmi.sp.pairs.upload(pr));
  }
  if (g.lmi.sp.fold) CXK_TRY(g.lmi.sp.etop.upload(etop));
  CXK_TRY(g.lmi.sp.eptr.upload(eptr));
  CXK_TRY(g.lmi.sp.erc.upload(erc));
  CXK_TRY(g.lmi.sp.eval.upload(eval));
  CXK_TRY(g.lmi.sp.pptr.upload(pptr));
  CXK_TRY(g.lmi.sp.pvar.upload(pvar));
  CXK_TRY(g.lmi.sp.pval.upload(pval));
  if (g.lmi.sa.on) {
    CXK_DEMAND(g.lmi.sp.cdense && !g.lmi.sp.small, "internal error: a sparse LMI group takes its affine term by nonzeros only beyond the LDS-resident orders");
    return UploadSparseAffine(ctx, g, lists, eptr);
  }
  return CXK_SUCCESS;
}

// Sparse LMI group: the nonzero sums; a dense C first needs X = W C W (LDS for small orders, two
// GEMMs otherwise).

template <bool SMALL, int LPP, bool AFF, bool FOLD>
hipError_t LaunchLmiSparseKernelL(Group& g, const LmiGroup& d, const Arena& ar, const double* X, hipStream_t st) {
  const dim3 grid(d.count, g.lmi.sp.chunks);
  const int emax = (g.lmi.sp.emax + 1) & ~1;  // keeps the arrays behind it 8-byte aligned
  const bool stage = LmiSparseLds(g.n, g.m, SMALL, g.lmi.sp.cdense, emax, FOLD) <= kLdsLimit;
  const size_t lds = LmiSparseLds(g.n, g.m, SMALL, g.lmi.sp.cdense, stage ? emax : 0, FOLD);
  SparseLaunchOf<AFF, FOLD> L;
  L.Xg = X;
  L.part = g.lmi.ws_part.p;
  L.npart = kSparseCParts;
  L.emax = stage ? emax : 0;
  L.cdense = g.lmi.sp.cdense;
  if constexpr (AFF) {
    L.Xp = g.lmi.ws_main.p + (size_t)d.count * g.n * g.n;
    L.eslot = g.lmi.sa.eslot.p;
    L.ppos = g.lmi.sa.pptr.p;
  }
  if constexpr (FOLD) L.etop = g.lmi.sp.etop.p;
  auto raise = [&](const void* k) -> hipError_t {  // dynamic LDS beyond 64 KB needs the attribute
    return lds > 64 * 1024 ? hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit)
                           : hipSuccess;
  };
  hipError_t e;
  if (stage) {
    if ((e = raise(reinterpret_cast<const void*>(&lmi_schur_sparse<SMALL, LPP, true, AFF, FOLD>))) != hipSuccess) return e;
    lmi_schur_sparse<SMALL, LPP, true, AFF, FOLD><<<grid, 256, lds, st>>>(d, ar, L);
  } else {
    if ((e = raise(reinterpret_cast<const void*>(&lmi_schur_sparse<SMALL, LPP, false, AFF, FOLD>))) != hipSuccess) return e;
    lmi_schur_sparse<SMALL, LPP, false, AFF, FOLD><<<grid, 256, lds, st>>>(d, ar, L);
  }
  return hipGetLastError();
}

template <bool SMALL, bool AFF, bool FOLD>
hipError_t LaunchLmiSparseKernelF(Group& g, const LmiGroup& d, const Arena& ar, const double* X, hipStream_t st) {
  switch (g.lmi.sp.lpp) {
    case 1: return LaunchLmiSparseKernelL<SMALL, 1, AFF, FOLD>(g, d, ar, X, st);
    case 4: return LaunchLmiSparseKernelL<SMALL, 4, AFF, FOLD>(g, d, ar, X, st);
    case 16: return LaunchLmiSparseKernelL<SMALL, 16, AFF, FOLD>(g, d, ar, X, st);
    default: return LaunchLmiSparseKernelL<SMALL, 64, AFF, FOLD>(g, d, ar, X, st);
  }
}

// (the folded form of an instance by the code: LmiSchurKernel)
template <bool SMALL, bool AFF = false>
hipError_t LaunchLmiSparseKernel(Group& g, bool fold, const LmiGroup& d, const Arena& ar, const double* X, hipStream_t st) {
  return fold ? LaunchLmiSparseKernelF<SMALL, AFF, true>(g, d, ar, X, st) : LaunchLmiSparseKernelF<SMALL, AFF, false>(g, d, ar, X, st);
}

hipError_t LaunchLmiSchurSparse(Group& g, LmiKernel code, const Arena& ar, hipStream_t st) {
  LmiGroup d = MakeLmi(g);
  const int n = g.n;
  const bool fold = IsSchurSparseFolded(code);
  const LmiKernel kern = UnfoldedSchurSparse(code);
  if (kern == kSchurSparseSmall || kern == kSchurSparseSmallDenseC) return LaunchLmiSparseKernel<true>(g, fold, d, ar, nullptr, st);
  if (fold) {  // every launch below reads the projection of W onto the real representations (kernels_lmi_sparse.hip.h)
    const int n0 = n / g.herm_d;
    double* Wp = FoldedW(g);
    lmi_fold_project<<<dim3((n0 * n0 + 255) / 256, g.herm_d, d.count), 256, 0, st>>>(d, Wp);
    d.W = Wp;
  }
  double* X = nullptr;
  if (kern == kSchurSparseAffine) {
    SparseAffine a;
    a.cptr = g.lmi.sa.cptr.p;
    a.crc = g.lmi.sa.crc.p;
    a.cslot = g.lmi.sa.cslot.p;
    a.cval = g.lmi.sa.cval.p;
    a.pptr = g.lmi.sa.pptr.p;
    a.prc = g.lmi.sa.prc.p;
    a.U = g.lmi.ws_main.p;                               // count x n^2
    a.Xp = g.lmi.ws_main.p + (size_t)d.count * n * n;    // at most count x n^2 positions
    const int tiles = (n + 63) / 64;
    lmi_affine_wc<<<dim3(tiles, tiles, d.count), 256, 0, st>>>(d, a);
    lmi_affine_x<<<dim3((g.lmi.sa.pmax + 3) / 4, d.count), 256, 0, st>>>(d, a);
    lmi_affine_scalars<<<dim3(kSparseCParts, d.count), 256, 0, st>>>(d, a, g.lmi.ws_part.p);
    return LaunchLmiSparseKernel<false, true>(g, fold, d, ar, nullptr, st);
  } else if (g.lmi.sp.cdense) {
    const int64_t nn = (int64_t)n * n;
    double* CW = g.lmi.ws_main.p;                  // count x nn
    X = g.lmi.ws_main.p + (size_t)d.count * nn;    // count x nn
    hipError_t e;
    GemmArgs a = SquareGemm(n, d.C, nn, d.W, nn, CW, nn);
    if ((e = LaunchGemm(a, false, false, d.count, st)) != hipSuccess) return e;
    a = SquareGemm(n, d.W, nn, CW, nn, X, nn);
    if ((e = LaunchGemm(a, false, false, d.count, st)) != hipSuccess) return e;
    lmi_dense_c_scalars<<<dim3(kSparseCParts, d.count), 256, 0, st>>>(d, X, g.lmi.ws_part.p);
  }
  return LaunchLmiSparseKernel<false>(g, fold, d, ar, X, st);
}

// The Schur complement of a group of dense LMIs, on the instance LmiSchurKernel names.
int LaunchLmiDenseSchur(cxk_context* ctx, Group& g, const Arena& ar) {
  const LmiKernel kern = LmiSchurKernel(g);
  // (lmi_schur_mfma carries the pair on its dispatch instead: no marker packets)
  const AssemblyClock clock(ctx, IsSchurMfma(kern));
  if (IsSchurGemm(kern)) {
    CXK_TRY(LmiLargeSchur(MakeLmi(g), ar, MakeLargeWs(g), ctx->stream));
  } else if (IsSchurMfma(kern)) {
    LmiGroup lg = MakeLmi(g);
    if (g.lmi.Apad.p) {  // the order runs on the next instance up (masked W loads in the kernel)
      const int np = LmiMfmaPaddedOrder(g.n);
      lg.A = g.lmi.Apad.p;
      lg.a_stride = (long long)(g.m + 1) * np * np;
    }
    // every other launch of the group last to first: a launch then starts on the operands the previous one
    // ended with, which shortens its fill (the results are the same bits either way)
    const int rev = ctx->lmi_order_forward ? 0 : (int)(g.lmi.schur_launches & 1);
    g.lmi.schur_launches++;
    CXK_TRY(LaunchLmiSchurMfma(lg, ar, ctx->cus, rev, ctx->stream, clock.clk.e0, clock.clk.e1));
  } else {
    lmi_schur_generic<<<(int)g.ids.size(), 256, LmiGenericLds(g.n), ctx->stream>>>(MakeLmi(g), ar);
  }
  return CXK_SUCCESS;
}

int LaunchLmiSparseSchur(cxk_context* ctx, Group& g, const Arena& ar) {
  CXK_TRY(LaunchLmiSchurSparse(g, LmiSchurKernel(g), ar, ctx->stream));
  return CXK_SUCCESS;
}

int LaunchLmiFactoredSchur(cxk_context* ctx, Group& g, const Arena& ar) {
  CXK_TRY(LmiFactoredSchur(MakeLmi(g), MakeLmiFactored(g), ar, MakeLargeWs(g), ctx->stream));
  return CXK_SUCCESS;
}

void LaunchLmiSetIdentity(Group& g, hipStream_t st) {
  lmi_set_identity<<<GridFor(g.ids.size() * g.n * g.n, 256), 256, 0, st>>>(MakeLmi(g));
}

namespace {
// The same instance of a stage whatever it serves: the query's and the affine update's codes as PrepareStep's.
LmiKernel AsPrepareKernel(LmiKernel k) {
  if (k >= kQueryRowsPacked && k <= kQueryLarge) return (LmiKernel)(k - kQueryRowsPacked + kPrepareRowsPacked);
  if (k >= kAffineGeneric20 && k <= kAffineLarge) return (LmiKernel)(k - kAffineGeneric20 + kPrepareGeneric20);
  return k;
}

template <int MODE>
int LmiPrepare(cxk_context* ctx, Group& g, int pmode, const StepArgs& sa, const StepTail& tail, int tail_blocks, const StepClock& clk) {
  const int cnt = (int)g.ids.size();
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
        case kPrepareRowsExact:  // (the instance reads g.lmi.Apk when there is one)
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
    default: CXK_DEMAND(false, "internal error: not a route of the matrix inequalities");
  }
  return CXK_SUCCESS;
}
}  // namespace

// PrepareStep (mode 0; pmode 0, or 2 for the affine update) or the eigenvalue query (mode 1; pmode 1) of one group.
int LaunchLmiPrepare(cxk_context* ctx, Group& g, int mode, int pmode, const StepArgs& sa, const StepTail& tail,
                     int tail_blocks, const StepClock& clk) {
  return mode == 0 ? LmiPrepare<0>(ctx, g, pmode, sa, tail, tail_blocks, clk) : LmiPrepare<1>(ctx, g, pmode, sa, tail, tail_blocks, clk);
}

int LaunchLmiTakeStep(cxk_context* ctx, Group& g, const StepArgs& sa, const StepClock& clk) {
  const int cnt = (int)g.ids.size();
  const int blocks = (cnt + 3) / 4;
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
  return CXK_SUCCESS;
}

}  // namespace cxk_host

extern "C" {

int cxk_lmi_kernels(const cxk_context* ctx, int constraint, int out[5]) {
  if (!ctx || !ctx->device_ready || !out || constraint < 0 || constraint >= (int)ctx->cons.size()) return CXK_FAILURE;
  const ConstraintRec& c = ctx->cons[constraint];
  if (c.type != CXK_LMI || c.factors.given || !ctx->owned[constraint]) return CXK_FAILURE;
  const Group& g = ctx->groups[c.group];
  out[CXK_LMI_STAGE_SCHUR] = LmiSchurKernel(g);
  out[CXK_LMI_STAGE_PREPARE] = LmiPrepareKernel(ctx, g, 0);
  out[CXK_LMI_STAGE_QUERY] = LmiPrepareKernel(ctx, g, 1);
  out[CXK_LMI_STAGE_TAKE] = LmiTakeKernel(g);
  out[CXK_LMI_STAGE_AFFINE] = LmiPrepareKernel(ctx, g, 2);
  return CXK_SUCCESS;
}

const char* cxk_lmi_kernel_name(int code) {
  if (code == kSchurSparseAffine) return kSchurSparseAffineName;
  if (IsSchurSparseFolded((LmiKernel)code)) return kSchurSparseFoldedNames[code - kSchurSparseFolded];
  return code >= 0 && code < kLmiKernelCount ? kLmiKernelNames[code] : nullptr;
}

int cxk_lmi_kernel_count(void) { return kLmiKernelCount; }

#ifdef CXK_DEBUG_STAMPS
int cxk_debug_sparse_stamps(long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sparse_stamp), 8 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
#endif

}  // extern "C"
