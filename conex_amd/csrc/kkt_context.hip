// cxk_* C-ABI: device-resident Newton-step KKT path (see include/conex_kkt_hip.h).
//
// Host side = structure + launches only.  All fp64 state (A_i, C, W, Schur blocks, the
// supernodal slab, right-hand sides) lives in HBM for the lifetime of the context; per
// Newton step only scalars cross PCIe.
#include <hip/hip_ext.h>
#include "kkt_internal.h"
#include "kernels_cone.hip.h"
#include "kernels_gemm.hip.h"
#include "kernels_kkt_big.hip.h"
#include "kernels_oct.hip.h"
#include "kernels_lmi.hip.h"
#include "lmi_fused_mfma.h"
#include "kernels_lmi_sparse.hip.h"
#include "kernels_lmi_rows.hip.h"
#include "kernels_lmi_large.hip.h"
#include "kernels_quad.hip.h"


namespace cxk_host {

int Fail(cxk_context* ctx, const char* msg) {
  ctx->err = msg;
  fprintf(stderr, "conex_kkt_hip: %s\n", msg);
  return CXK_FAILURE;
}

bool IsUnique(int N, int m, const int* x) {  // constraint_manager.h:11-24
  std::vector<char> seen(N > 0 ? N : 1, 0);
  for (int i = 0; i < m; i++) {
    if (x[i] >= N || x[i] < 0) return false;
    if (seen[x[i]]++) return false;
  }
  return true;
}

int AddConstraint(cxk_context* ctx, ConstraintRec&& rec, const int* vars) {
  if (!ctx || ctx->finalized) return -1;
  if (vars) {
    if (!IsUnique(ctx->num_vars, rec.m, vars)) return -1;
  } else if (rec.m != ctx->num_vars) {
    return -1;
  }
  IntList cl(rec.m);
  for (int i = 0; i < rec.m; i++) cl[i] = vars ? vars[i] : i;
  ctx->cliques.push_back(cl);
  ctx->dual_vars.emplace_back();
  ctx->cons.push_back(std::move(rec));
  return static_cast<int>(ctx->cons.size()) - 1;
}

int GridFor(size_t work, int block) {
  size_t g = (work + block - 1) / block;
  if (g < 1) g = 1;
  if (g > 4096) g = 4096;
  return static_cast<int>(g);
}

// two-shape chains tree_chain_lean is compiled for (LaunchChain): a pair holding <24,0>, or <8,8> with
// <16,8> (second-order cones of dimension 10 with a root of 10 columns: BASELINE config 3)
bool ChainPairCompiled(int sa, int sb) {
  if (sb == 0 || sa == sb) return true;
  if (sa > sb) std::swap(sa, sb);
  return sa == (24 << 8) || sb == (24 << 8) || (sa == (8 << 8 | 8) && sb == (16 << 8 | 8));
}

LmiGroup MakeLmi(Group& g) {
  LmiGroup d;
  d.n = g.n;
  d.m = g.m;
  d.count = static_cast<int>(g.ids.size());
  d.A = g.A.p;
  d.a_stride = (long long)((g.mfma || g.schur_gemm) ? g.m + 1 : g.m) * g.n * g.n;
  d.C = g.C.p;
  d.W = g.W.p;
  d.T1 = g.T1.p;
  d.ids = g.dids.p;
  d.Apk = g.Apk.n ? g.Apk.p : nullptr;
  d.herm_d = g.herm_d;
  d.sp_eptr = g.sparse ? g.sp_eptr.p : nullptr;
  d.sp_erc = g.sparse ? g.sp_erc.p : nullptr;
  d.sp_pairs = g.sparse ? g.sp_pairs.p : nullptr;
  d.sp_eval = g.sparse ? g.sp_eval.p : nullptr;
  d.sp_pptr = g.sparse ? g.sp_pptr.p : nullptr;
  d.sp_pvar = g.sparse ? g.sp_pvar.p : nullptr;
  d.sp_pval = g.sparse ? g.sp_pval.p : nullptr;
  return d;
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
  StepArgs s;
  s.y = ctx->y.p;
  s.y3 = nullptr;
  s.y3_stride = 0;
  s.y3_k = nullptr;
  s.cl_ptr = ctx->cl_ptr.p;
  s.cl_perm = ctx->cl_perm.p;
  s.info = info;
  s.affine = affine;
  s.c_weight = cw;
  s.e_weight = ew;
  s.step_size = ss;
  s.step_from = nullptr;
  s.cw_from = nullptr;
  s.cw_scale = 1.0;
  s.skip_if = nullptr;
  s.skip_tag = 0;
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
  return w;
}

size_t LmiGenericLds(int n) { return sizeof(double) * (size_t)(4 * n * n); }
size_t LmiPrepareLds(int n, int m) {
  return sizeof(double) * (size_t)(3 * n * n + 6 * n + 2 * (n / 2 + 2) + m + 8);
}
size_t LmiTakeLds(int n) { return sizeof(double) * (size_t)(5 * n * n); }

// ---- The kernel instance each per-constraint stage of an LMI group runs.  One chooser per stage: the
// launch sites switch on its answer and cxk_lmi_kernels reports it, so the two cannot disagree.  The
// choosers read only the group's shape and the flags fixed at create / initialize.
enum LmiKernel : int {
  // Schur complement (LaunchSchur)
  kSchurGenericLiteral,
  kSchurGenericSym,
  kSchurMfma8,  // lmi_schur_mfma<N, false> at order N, two P images
  kSchurMfma8Pad,  // ... at a smaller order, zero-padded
  kSchurMfma12,
  kSchurMfma12Pad,
  kSchurMfma16,
  kSchurMfma16Single,  // ... one P image
  kSchurMfma16Pad,
  kSchurMfma16PadSingle,
  kSchurMfma20,
  kSchurMfma20Single,
  kSchurMfma20Pad,
  kSchurMfma20PadSingle,
  kSchurMfma24,
  kSchurMfma24Single,
  kSchurMfma24Pad,
  kSchurMfma24PadSingle,
  kSchurMfma24Folded,
  kSchurMfma24FoldedSingle,
  kSchurGemm,  // batched-GEMM assembly: full form, LDS-resident order, one K split
  kSchurGemmSplit,
  kSchurGemmLarge,
  kSchurGemmLargeSplit,
  kSchurGemmFolded,
  kSchurGemmFoldedSplit,
  kSchurGemmFoldedLarge,
  kSchurGemmFoldedLargeSplit,
  kSchurSparseSmall,
  kSchurSparseSmallDenseC,
  kSchurSparse,
  kSchurSparseDenseC,
  // PrepareStep (MODE 0) and the eigenvalue query (MODE 1): the same order of instances each
  kPrepareRowsPacked,
  kPrepareRowsExact,  // order 20, Apk null
  kPrepareRowsOdd,
  kPrepareRowsEven,
  kPrepareGeneric20,
  kPrepareGeneric,
  kPrepareLarge,
  kQueryRowsPacked,
  kQueryRowsExact,
  kQueryRowsOdd,
  kQueryRowsEven,
  kQueryGeneric20,
  kQueryGeneric,
  kQueryLarge,
  // the affine update (PrepareStep with affine != 0)
  kAffineGeneric20,
  kAffineGeneric,
  kAffineLarge,
  // TakeStep
  kTakeRows20,
  kTakeRows20Pad,
  kTakeRows32,
  kTakeRows32Pad,
  kTakeTaylor24,
  kTakeTaylor24Pad,
  kTakeTaylor32,
  kTakeTaylor32Pad,
  kTakeGeneric20,
  kTakeGeneric,
  kTakeLargePade,
  kTakeLargeTaylor,
  kLmiKernelCount
};

const char* const kLmiKernelNames[kLmiKernelCount] = {
    "lmi_schur_generic literal",
    "lmi_schur_generic symmetric",
    "lmi_schur_mfma<8> exact two-images",
    "lmi_schur_mfma<8> padded two-images",
    "lmi_schur_mfma<12> exact two-images",
    "lmi_schur_mfma<12> padded two-images",
    "lmi_schur_mfma<16> exact two-images",
    "lmi_schur_mfma<16> exact one-image",
    "lmi_schur_mfma<16> padded two-images",
    "lmi_schur_mfma<16> padded one-image",
    "lmi_schur_mfma<20> exact two-images",
    "lmi_schur_mfma<20> exact one-image",
    "lmi_schur_mfma<20> padded two-images",
    "lmi_schur_mfma<20> padded one-image",
    "lmi_schur_mfma<24> exact two-images",
    "lmi_schur_mfma<24> exact one-image",
    "lmi_schur_mfma<24> padded two-images",
    "lmi_schur_mfma<24> padded one-image",
    "lmi_schur_mfma<24,folded> two-images",
    "lmi_schur_mfma<24,folded> one-image",
    "schur_gemm full lds",
    "schur_gemm full lds split",
    "schur_gemm full large",
    "schur_gemm full large split",
    "schur_gemm folded lds",
    "schur_gemm folded lds split",
    "schur_gemm folded large",
    "schur_gemm folded large split",
    "lmi_schur_sparse small",
    "lmi_schur_sparse small dense-C",
    "lmi_schur_sparse hbm",
    "lmi_schur_sparse hbm dense-C",
    "lmi_prepare_rows<0,20,exact> packed",
    "lmi_prepare_rows<0,20,exact> unpacked",
    "lmi_prepare_rows<0,20> odd",
    "lmi_prepare_rows<0,20> even",
    "lmi_prepare_generic<0,20>",
    "lmi_prepare_generic<0,0>",
    "LmiLargePrepare<0>",
    "lmi_prepare_rows<1,20,exact> packed",
    "lmi_prepare_rows<1,20,exact> unpacked",
    "lmi_prepare_rows<1,20> odd",
    "lmi_prepare_rows<1,20> even",
    "lmi_prepare_generic<1,20>",
    "lmi_prepare_generic<1,0>",
    "LmiLargePrepare<1>",
    "lmi_prepare_generic<0,20> affine",
    "lmi_prepare_generic<0,0> affine",
    "LmiLargePrepare<0> affine",
    "lmi_take_step_rows<20> exact",
    "lmi_take_step_rows<20> padded",
    "lmi_take_step_rows<32> exact",
    "lmi_take_step_rows<32> padded",
    "lmi_take_step_rows_taylor<24> exact",
    "lmi_take_step_rows_taylor<24> padded",
    "lmi_take_step_rows_taylor<32> exact",
    "lmi_take_step_rows_taylor<32> padded",
    "lmi_take_step_generic<20>",
    "lmi_take_step_generic<0>",
    "LmiLargeTakeStep pade",
    "LmiLargeTakeStep taylor",
};

bool IsSchurMfma(LmiKernel k) { return k >= kSchurMfma8 && k <= kSchurMfma24FoldedSingle; }
bool IsSchurGemm(LmiKernel k) { return k >= kSchurGemm && k <= kSchurGemmFoldedLargeSplit; }
bool IsSchurSparse(LmiKernel k) { return k >= kSchurSparseSmall && k <= kSchurSparseDenseC; }
bool IsPrepareRows(LmiKernel k) {
  return (k >= kPrepareRowsPacked && k <= kPrepareRowsEven) || (k >= kQueryRowsPacked && k <= kQueryRowsEven);
}
bool IsTakeRows(LmiKernel k) { return k >= kTakeRows20 && k <= kTakeTaylor32Pad; }

LmiKernel LmiSchurKernel(const Group& g) {
  if (g.sparse) return (LmiKernel)((g.sp_small ? kSchurSparseSmall : kSchurSparse) + (g.sp_cdense ? 1 : 0));
  if (g.schur_gemm) {  // (fold and split counts as LmiLargeSchur reads them: MakeLargeWs, LmiFoldedSplits)
    const bool fold = g.Aleft.n != 0;
    const int splits = fold ? LmiFoldedSplits(g.splits, g.n, g.n / g.herm_d) : g.splits;
    return (LmiKernel)(kSchurGemm + (fold ? 4 : 0) + (g.large ? 2 : 0) + (splits > 1 ? 1 : 0));
  }
  if (g.mfma) {
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
  if (mode != 2 && !ctx->prepare_lds && !g.literal && LmiPrepareRowsSupports(g.n, g.m, g.herm_d, g.sparse)) {
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


hipError_t RaiseTopDenseLimits() {
  for (const void* kf : {reinterpret_cast<const void*>(&tree_top_dense<32>), reinterpret_cast<const void*>(&tree_top_dense<40>),
                         reinterpret_cast<const void*>(&tree_top_dense<48>), reinterpret_cast<const void*>(&tree_top_dense<56>),
                         reinterpret_cast<const void*>(&tree_top_dense<64>)}) {
    const hipError_t e = hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTopDenseLds);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Kernels that may be launched with more than the default 64 KB of dynamic LDS.
hipError_t RaiseLdsLimits() {
  static PerDeviceOnce once;  // function attributes are per device: every device a context is built on
  return once.run([] {
    const int lim = (int)kLdsLimit;
    const void* ks[] = {
        reinterpret_cast<const void*>(&lmi_schur_generic),
        reinterpret_cast<const void*>(&lmi_prepare_generic<0, 0>),
        reinterpret_cast<const void*>(&lmi_prepare_generic<1, 0>),
        reinterpret_cast<const void*>(&lmi_take_step_generic<0>),
#define CXK_PAIR_K(NA_, SA_, NB_, SB_)                                              \
  reinterpret_cast<const void*>(&tree_factor_level2<NA_, SA_, NB_, SB_, true>),      \
      reinterpret_cast<const void*>(&tree_factor_level2<NA_, SA_, NB_, SB_, false>),
        CXK_PAIR_K(8, 8, 16, 8) CXK_PAIR_K(8, 8, 24, 0) CXK_PAIR_K(8, 8, 24, 8) CXK_PAIR_K(8, 8, 32, 16)
        CXK_PAIR_K(16, 8, 24, 0) CXK_PAIR_K(16, 8, 24, 8) CXK_PAIR_K(16, 8, 32, 16)
        CXK_PAIR_K(24, 0, 24, 8) CXK_PAIR_K(24, 0, 32, 16) CXK_PAIR_K(24, 8, 32, 16)
#undef CXK_PAIR_K
        reinterpret_cast<const void*>(&tree_chain_lean<0, 32, 16, 32, 16>),
        reinterpret_cast<const void*>(&tree_chain_lean<0, 24, 0, 32, 16>),
        reinterpret_cast<const void*>(&tree_factor_level<8, 8, true>),
        reinterpret_cast<const void*>(&tree_factor_level<8, 8, false>),
        reinterpret_cast<const void*>(&tree_factor_level<16, 8, true>),
        reinterpret_cast<const void*>(&tree_factor_level<16, 8, false>),
        reinterpret_cast<const void*>(&tree_factor_level<24, 0, true>),
        reinterpret_cast<const void*>(&tree_factor_level<24, 0, false>),
        reinterpret_cast<const void*>(&tree_factor_level<24, 8, true>),
        reinterpret_cast<const void*>(&tree_factor_level<24, 8, false>),
        reinterpret_cast<const void*>(&tree_factor_level<32, 16, true>),
        reinterpret_cast<const void*>(&tree_factor_level<32, 16, false>),
        reinterpret_cast<const void*>(&tree_sweep<0, false>),
        reinterpret_cast<const void*>(&tree_sweep<0, true>),
        reinterpret_cast<const void*>(&tree_sweep<1, false>),
        reinterpret_cast<const void*>(&tree_sweep<1, true>),
        reinterpret_cast<const void*>(&tree_sweep<2, false>),
        reinterpret_cast<const void*>(&tree_sweep<2, true>),
        reinterpret_cast<const void*>(&tree_sweep_block<0>),
        reinterpret_cast<const void*>(&tree_sweep_block<1>),
        reinterpret_cast<const void*>(&tree_sweep_block<2>),
        reinterpret_cast<const void*>(&tree_sweep_block_ldlt<0>),
        reinterpret_cast<const void*>(&tree_sweep_block_ldlt<1>),
        reinterpret_cast<const void*>(&tree_sweep_block_ldlt<2>),
        reinterpret_cast<const void*>(&soc_schur<true>),
        reinterpret_cast<const void*>(&soc_schur<false>),
    };
    for (const void* k : ks) {
      hipFuncAttributes attr;
      hipError_t e = hipFuncGetAttributes(&attr, k);
      if (e != hipSuccess) return e;
      // static + dynamic LDS must stay within the 160 KB of a CU
      const int dyn = std::min(lim, 160 * 1024 - (int)attr.sharedSizeBytes);
      e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  });
}

ExchangeArgs MakeExchange(cxk_context* ctx, double k, double bs, double cs) {
  ExchangeArgs a;
  a.n_xs = ctx->n_xs;
  a.n_xv = ctx->n_xv;
  a.xs_off = ctx->xs_off.p;
  a.xs_pt = ctx->xs_pt.p;
  a.xv_idx = ctx->xv_idx.p;
  a.pt_T = (int64_t)(ctx->pt_ptr.n > 0 ? ctx->pt_ptr.n - 1 : 0);
  a.pt_dst = ctx->pt_dst.p;
  a.pt_ptr = ctx->pt_ptr.p;
  a.pt_src = ctx->pt_src.p;
  a.pf_ptr = ctx->pf_ptr.p;
  a.pf_src = ctx->pf_src.p;
  a.upd = ctx->upd.p;
  a.updb = ctx->updb.p;
  a.slab = ctx->slab.p;
  a.AW = ctx->AW.p;
  a.AQc = ctx->AQc.p;
  a.b = ctx->b.p;
  a.y = ctx->y.p;
  a.sys_sc = ctx->sys_sc.p;
  a.fail = ctx->d_fail.p;
  a.host_flag = ctx->fx_flag;
  a.tag = ctx->fail_tag;
  a.x = ctx->xbuf.p;
  a.cb = k * bs;
  a.cq = k * cs;
  a.cw = -2.0;
  return a;
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
constexpr int kSparseCParts = 64;  // slices of the <w,c>, <c,Qc> sums of a dense C beyond LDS orders

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

int LaunchSchur(cxk_context* ctx) {
  Arena ar = MakeArena(ctx);
  for (Group& g : ctx->groups) {
    const int count = (int)g.ids.size();
    if (count == 0) continue;
    switch (g.type) {
      case CXK_LMI: {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        const bool sample = ClockSample(ctx, CXK_CLOCK_ASSEMBLY, &e0, &e1);
        const LmiKernel kern = LmiSchurKernel(g);
        // (lmi_schur_mfma carries the pair on its dispatch instead: no marker packets)
        if (sample && !IsSchurMfma(kern)) CXK_TRY(hipEventRecord(e0, ctx->stream));
        if (IsSchurSparse(kern)) {
          CXK_TRY(LaunchLmiSchurSparse(g, kern, ar, ctx->stream));
        } else if (IsSchurGemm(kern)) {
          CXK_TRY(LmiLargeSchur(MakeLmi(g), ar, MakeLargeWs(g), ctx->stream));
        } else if (IsSchurMfma(kern)) {
          LmiGroup lg = MakeLmi(g);
          if (g.Apad.p) {  // the order runs on the next instance up (masked W loads in the kernel)
            const int np = LmiMfmaPaddedOrder(g.n);
            lg.A = g.Apad.p;
            lg.a_stride = (long long)(g.m + 1) * np * np;
          }
          CXK_TRY(LaunchLmiSchurMfma(lg, ar, ctx->cus, ctx->stream, e0, e1));
        } else {
          lmi_schur_generic<<<count, 256, LmiGenericLds(g.n), ctx->stream>>>(MakeLmi(g), ar);
        }
        if (sample && !IsSchurMfma(kern)) CXK_TRY(hipEventRecord(e1, ctx->stream));
        break;
      }
      case CXK_LINEAR:
        linear_schur<<<count, 256, 0, ctx->stream>>>(MakeVec(g), ar);
        break;
      case CXK_SOC:
      {
        // one wavefront per cone, up to four cones per workgroup; the cone's data staged in LDS when
        // four staged images fit, read in place otherwise
        const size_t staged = sizeof(double) * (size_t)(g.n + 1) * (2 * g.m + 4);
        const size_t plain = sizeof(double) * (size_t)(g.n + 1) * (g.m + 2);
        if (4 * staged <= kLdsLimit) {
          soc_schur<true><<<(count + 3) / 4, 256, 4 * staged, ctx->stream>>>(MakeVec(g), ar);
        } else {
          const int w = (int)std::max<size_t>(1, std::min<size_t>(4, kLdsLimit / plain));
          soc_schur<false><<<(count + w - 1) / w, 64 * w, w * plain, ctx->stream>>>(MakeVec(g), ar);
        }
      }
        break;
      case CXK_STATIC:
        static_schur<<<count, 64, 0, ctx->stream>>>(MakeStatic(g), ar);
        break;
      case CXK_QUAD:
        quad_schur<<<count, 64, sizeof(double) * (size_t)(2 * g.n + g.m + 4), ctx->stream>>>(MakeQuad(g), ar);
        break;
      case CXK_OCT:
        oct_schur<<<count, 64, 0, ctx->stream>>>(MakeOct(g), ar);
        break;
    }
  }
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

GatherArgs MakeGather(cxk_context* ctx, int with_rhs, double k, double bs, double cs) {
  GatherArgs a;
  a.T = ctx->as_T;
  a.rec = ctx->as_rec.p;
  a.src = ctx->as_src.p;
  a.G = ctx->G.p;
  a.slab = ctx->slab.p;
  a.N = ctx->md.N;
  a.rrec = ctx->rs_rec.p;
  a.var_idx = nullptr;
  a.rs_src = ctx->rs_src.p;
  a.AWc = ctx->AWc.p;
  a.AQcc = ctx->AQcc.p;
  a.AW = ctx->AW.p;
  a.AQc = ctx->AQc.p;
  a.K = (int)ctx->cons.size();
  a.sc = ctx->sc.p;
  a.sys_sc = ctx->sys_sc.p;
  a.with_rhs = with_rhs;
  a.k = k;
  a.bs = bs;
  a.cs = cs;
  a.cb = a.cq = a.cw = 0;
  a.b = ctx->b.p;
  a.y = ctx->y.p;
  a.fail = ctx->d_fail.p;
  return a;
}

// Arguments of a first factor level with the assembly folded in: the gather of everything its own
// supernodes do not load themselves, and what those need to load it (AsmIn).
void MakeFusedAssembly(cxk_context* ctx, const cxk_context::AsmPending& ap, GatherArgs* gap, AsmIn* aip) {
  GatherArgs ga = MakeGather(ctx, ap.with_rhs, ap.k, ap.bs, ap.cs);
  ga.cb = ap.cb;
  ga.cq = ap.cq;
  ga.cw = ap.cw;
  ga.T = ctx->as_T2;
  ga.rec = ctx->as_rec2.p;
  ga.N = ctx->rs_N2;
  ga.rrec = ctx->rs_rec2.p;
  ga.var_idx = ctx->rs_var2.p;
  AsmIn ai;
  ai.rec = ctx->asm_rec.p;
  ai.G = ctx->G.p;
  ai.AWc = ctx->AWc.p;
  ai.AQcc = ctx->AQcc.p;
  ai.b = ctx->b.p;
  ai.AW = ctx->AW.p;
  ai.AQc = ctx->AQc.p;
  ai.k = ap.k;
  ai.bs = ap.bs;
  ai.cs = ap.cs;
  ai.cb = ap.cb;
  ai.cq = ap.cq;
  ai.cw = ap.cw;
  ai.comb = ap.with_rhs == 2;
  ctx->asm_tag = ctx->asm_tag >= (1 << 30) ? 1 : ctx->asm_tag + 1;
  ai.tag = ctx->fail_tag = ctx->asm_tag;
  *gap = ga;
  *aip = ai;
}

int LaunchGather(cxk_context* ctx, bool with_rhs, double k, double bs, double cs) {
  const GatherArgs a = MakeGather(ctx, with_rhs ? 1 : 0, k, bs, cs);
  assemble_gather<<<GridFor((size_t)std::max<int64_t>(ctx->as_T, ctx->md.N), 256), 256, 0,
                    ctx->stream>>>(a);
  CXK_TRY(hipGetLastError());
  ctx->fail_tag = 0;
  ctx->fail_clean = true;
  return CXK_SUCCESS;
}

// Supernodes of level l whose panel exceeds LDS: blocked HBM path, one at a time.
int LaunchHuge(cxk_context* ctx, int l, int mode, bool with_rhs) {
  const int first = ctx->level_ptr[l] + ctx->level_nh[l], last = ctx->level_ptr[l + 1];
  if (first == last) return CXK_SUCCESS;
  double* rhs = (with_rhs || mode != 0) ? ctx->y.p : nullptr;
  if (ctx->use_ldlt) {
    // the LDLT kernel of the LDS-sized supernodes with its panel image in HBM (same pivot rule, same
    // operations: RLDLT.h:298-431 picks every pivot from the whole trailing diagonal)
    for (int pos = first; pos < last; pos++) {
      if (mode == 0)
        tree_sweep_block_ldlt<0, true><<<1, 1024, 0, ctx->stream>>>(ctx->plan, pos, ctx->slab.p, rhs, ctx->d_tr.p, ctx->d_reg.p, ctx->big_ws.p);
      else if (mode == 1)
        tree_sweep_block_ldlt<1, true><<<1, 1024, 0, ctx->stream>>>(ctx->plan, pos, ctx->slab.p, rhs, ctx->d_tr.p, ctx->d_reg.p, ctx->big_ws.p);
      else
        tree_sweep_block_ldlt<2, true><<<1, 1024, 0, ctx->stream>>>(ctx->plan, pos, ctx->slab.p, rhs, ctx->d_tr.p, ctx->d_reg.p, ctx->big_ws.p);
      CXK_TRY(hipGetLastError());
    }
    return CXK_SUCCESS;
  }
  for (int pos = first; pos < last; pos++)
    CXK_TRY(BigSupernodeSweep(ctx->plan, ctx->h_recs[pos], mode, ctx->slab.p, rhs, ctx->d_fail.p,
                              ctx->big_ws.p, ctx->stream, ctx->big_flags.p, &ctx->big_gen));
  return CXK_SUCCESS;
}

// One sweep launch over levels [lb, le).  mode 0 factor(+forward), 1 forward, 2 backward.
int LaunchSweep(cxk_context* ctx, int lb, int le, int mode, bool then_backward, bool with_rhs) {
  const int per_wave = (int)(ctx->chol_lds / sizeof(double));
  const int wmax = std::max(1, std::min<int>(8, (int)(kLdsLimit / std::max<size_t>(ctx->chol_lds, 8))));
  if (le - lb == 1 && !then_backward && ctx->level_nh[lb] < ctx->level_ptr[lb + 1] - ctx->level_ptr[lb]) {
    if (LaunchHuge(ctx, lb, mode, with_rhs)) return CXK_FAILURE;
    if (ctx->level_nh[lb] == 0) return CXK_SUCCESS;
  }
  int maxcnt = 0;
  for (int l = lb; l < le; l++) maxcnt = std::max(maxcnt, le - lb == 1 ? ctx->level_nh[l] : ctx->level_ptr[l + 1] - ctx->level_ptr[l]);
  if (maxcnt == 0) return CXK_SUCCESS;
  int waves, grid;
  if (le - lb > 1 || then_backward) {
    const int wtop = std::max(1, std::min<int>(8, (int)((kLdsLimit - kRangeMaxRecs * sizeof(SnRec)) / std::max<size_t>(ctx->chol_lds, 8))));
    waves = std::min(wtop, maxcnt);
    grid = 1;
  } else {
    waves = std::max(1, std::min(wmax, (maxcnt + 255) / 256));
    grid = (maxcnt + waves - 1) / waves;
  }
  const bool is_top = le - lb > 1 || then_backward;
  if (ctx->use_ldlt) {
    CXK_DEMAND(!is_top, "internal error: LDLT sweeps are launched level by level");
    double* r = (with_rhs || mode != 0) ? ctx->y.p : nullptr;
    const int base = ctx->level_ptr[lb];
    if (mode == 0)
      tree_sweep_block_ldlt<0><<<maxcnt, 256, ctx->chol_lds, ctx->stream>>>(ctx->plan, base, ctx->slab.p, r, ctx->d_tr.p, ctx->d_reg.p);
    else if (mode == 1)
      tree_sweep_block_ldlt<1><<<maxcnt, 256, ctx->chol_lds, ctx->stream>>>(ctx->plan, base, ctx->slab.p, r, ctx->d_tr.p, ctx->d_reg.p);
    else
      tree_sweep_block_ldlt<2><<<maxcnt, 256, ctx->chol_lds, ctx->stream>>>(ctx->plan, base, ctx->slab.p, r, ctx->d_tr.p, ctx->d_reg.p);
    CXK_TRY(hipGetLastError());
    return CXK_SUCCESS;
  }
  if (!is_top && ctx->level_big[lb]) {  // one workgroup per supernode
    double* r = (with_rhs || mode != 0) ? ctx->y.p : nullptr;
    const int base = ctx->level_ptr[lb];
    if (mode == 0)
      tree_sweep_block<0><<<maxcnt, 256, ctx->chol_lds, ctx->stream>>>(ctx->plan, base, ctx->slab.p, r, ctx->d_fail.p);
    else if (mode == 1)
      tree_sweep_block<1><<<maxcnt, 256, ctx->chol_lds, ctx->stream>>>(ctx->plan, base, ctx->slab.p, r, ctx->d_fail.p);
    else
      tree_sweep_block<2><<<maxcnt, 256, ctx->chol_lds, ctx->stream>>>(ctx->plan, base, ctx->slab.p, r, ctx->d_fail.p);
    CXK_TRY(hipGetLastError());
    return CXK_SUCCESS;
  }
  double* rhs = (with_rhs || mode != 0) ? ctx->y.p : nullptr;
  if (!is_top && !ctx->no_lean) {
    // segment by segment: the kernel compiled for the segment's register shape alone where its
    // supernodes qualify, the generic kernel on the sub-range otherwise
    auto lean = [&](const cxk_context::LevelSeg& sg) { return sg.shape > 0 && (mode == 2 ? sg.inl : sg.fast); };
    bool any = false;
    for (auto& sg : ctx->level_segs[lb]) any = any || lean(sg);
    if (any) {
      const auto& segs = ctx->level_segs[lb];
      for (size_t si = 0; si < segs.size(); si++) {
        const auto& sg = segs[si];
        const int cnt = sg.end - sg.begin;
        if (lean(sg) && si + 1 < segs.size() && lean(segs[si + 1])) {
          // two lean segments: one launch, workgroups [0, gA) on shape A and the rest on shape B
          const auto& sb = segs[si + 1];
          const int cntB = sb.end - sb.begin;
          const int w = std::max(1, std::min(std::min(wmax, 4), (std::max(cnt, cntB) + 255) / 256));
          const int gA = (cnt + w - 1) / w, gB = (cntB + w - 1) / w;
          const size_t lds = (size_t)w * ctx->chol_lds;
          const int sa = sg.shape, sb2 = sb.shape;
          bool done = false;
          if (mode == 0 && lb == 0 && ctx->asm_pending.on && ctx->asm_pending.with_rhs != 0 && segs.size() == 2) {
            // the assembly rides in this launch (see the one-shape case below)
            const cxk_context::AsmPending ap = ctx->asm_pending;
            ctx->asm_pending.on = false;
            GatherArgs ga;
            AsmIn ai;
            MakeFusedAssembly(ctx, ap, &ga, &ai);
            const int w4 = 4, gA4 = (cnt + w4 - 1) / w4, gB4 = (cntB + w4 - 1) / w4;
            const size_t lds4 = (size_t)w4 * ctx->chol_lds;
            const int gg = GridFor((size_t)std::max<int64_t>(std::max<int64_t>(ga.T, ga.N), 1), 256);
#define CXK_PAIR_ASM(NA_, SA_, NB_, SB_)                                                                     \
  if (!done && sa == ((NA_) << 8 | (SA_)) && sb2 == ((NB_) << 8 | (SB_))) {                                  \
    done = true;                                                                                             \
    tree_factor_level2_asm<NA_, SA_, NB_, SB_><<<gA4 + gB4 + gg, w4 * 64, lds4, ctx->stream>>>(              \
        ctx->plan, ctx->p_rec.p, sg.begin, cnt, gA4, sb.begin, cntB, ctx->slab.p, rhs, ctx->d_fail.p,        \
        per_wave, ai, ga, gA4 + gB4);                                                                        \
  }
            CXK_PAIR_ASM(8, 8, 16, 8)
            CXK_PAIR_ASM(8, 8, 24, 0)
            CXK_PAIR_ASM(8, 8, 24, 8)
            CXK_PAIR_ASM(8, 8, 32, 16)
            CXK_PAIR_ASM(16, 8, 24, 0)
            CXK_PAIR_ASM(16, 8, 24, 8)
            CXK_PAIR_ASM(16, 8, 32, 16)
            CXK_PAIR_ASM(24, 0, 24, 8)
            CXK_PAIR_ASM(24, 0, 32, 16)
            CXK_PAIR_ASM(24, 8, 32, 16)
#undef CXK_PAIR_ASM
            CXK_DEMAND(done, "internal error: no tree_factor_level2_asm instance for the first level's shapes");
            si++;
            continue;
          }
#define CXK_PAIR(NA_, SA_, NB_, SB_)                                                                         \
  if (!done && sa == ((NA_) << 8 | (SA_)) && sb2 == ((NB_) << 8 | (SB_))) {                                  \
    done = true;                                                                                             \
    if (mode == 2)                                                                                           \
      tree_backward_level2<NA_, SA_, NB_, SB_><<<gA + gB, w * 64, 0, ctx->stream>>>(                         \
          ctx->p_rec.p, sg.begin, cnt, gA, sb.begin, cntB, ctx->slab.p, rhs);                                \
    else if (mode == 1)                                                                                      \
      tree_forward_level2<NA_, SA_, NB_, SB_><<<gA + gB, w * 64, 0, ctx->stream>>>(                          \
          ctx->plan, ctx->p_rec.p, sg.begin, cnt, gA, sb.begin, cntB, ctx->slab.p, rhs, ctx->rhs_in);        \
    else if (rhs)                                                                                            \
      tree_factor_level2<NA_, SA_, NB_, SB_, true><<<gA + gB, w * 64, lds, ctx->stream>>>(                   \
          ctx->plan, ctx->p_rec.p, sg.begin, cnt, gA, sb.begin, cntB, ctx->slab.p, rhs, ctx->d_fail.p, per_wave); \
    else                                                                                                     \
      tree_factor_level2<NA_, SA_, NB_, SB_, false><<<gA + gB, w * 64, lds, ctx->stream>>>(                  \
          ctx->plan, ctx->p_rec.p, sg.begin, cnt, gA, sb.begin, cntB, ctx->slab.p, rhs, ctx->d_fail.p, per_wave); \
  }
          CXK_PAIR(8, 8, 16, 8)
          CXK_PAIR(8, 8, 24, 0)
          CXK_PAIR(8, 8, 24, 8)
          CXK_PAIR(8, 8, 32, 16)
          CXK_PAIR(16, 8, 24, 0)
          CXK_PAIR(16, 8, 24, 8)
          CXK_PAIR(16, 8, 32, 16)
          CXK_PAIR(24, 0, 24, 8)
          CXK_PAIR(24, 0, 32, 16)
          CXK_PAIR(24, 8, 32, 16)
#undef CXK_PAIR
          if (done) {
            si++;
            continue;
          }
        }
        if (!lean(sg)) {
          const int w = std::max(1, std::min(wmax, (cnt + 255) / 256));
          const int g = (cnt + w - 1) / w;
          if (mode == 0)
            tree_sweep<0, false><<<g, w * 64, (size_t)w * ctx->chol_lds, ctx->stream>>>(
                ctx->plan, ctx->p_rec.p, nullptr, sg.begin, cnt, 1, 0, ctx->slab.p, rhs, ctx->d_fail.p, per_wave);
          else if (mode == 1)
            tree_sweep<1, false><<<g, w * 64, (size_t)w * ctx->chol_lds, ctx->stream>>>(
                ctx->plan, ctx->p_rec.p, nullptr, sg.begin, cnt, 1, 0, ctx->slab.p, rhs, ctx->d_fail.p, per_wave);
          else
            tree_sweep<2, false><<<g, w * 64, (size_t)w * ctx->chol_lds, ctx->stream>>>(
                ctx->plan, ctx->p_rec.p, nullptr, sg.begin, cnt, 1, 0, ctx->slab.p, rhs, ctx->d_fail.p, per_wave);
          continue;
        }
        // the shape-specialised level kernels are compiled for <= 256 threads
        const int w = std::max(1, std::min(std::min(wmax, 4), (cnt + 255) / 256));
        const int g = (cnt + w - 1) / w;
        const size_t lds = (size_t)w * ctx->chol_lds;
        const int sh = sg.shape;
#define CXK_LEVEL(NS_, S_)                                                                              \
  if (sh == ((NS_) << 8 | (S_))) {                                                                      \
    if (mode == 2)                                                                                      \
      tree_backward_level<NS_, S_><<<g, w * 64, 0, ctx->stream>>>(ctx->p_rec.p, sg.begin, cnt,          \
                                                                  ctx->slab.p, rhs);                    \
    else if (mode == 1)                                                                                 \
      tree_forward_level<NS_, S_><<<g, w * 64, 0, ctx->stream>>>(ctx->plan, ctx->p_rec.p, sg.begin,     \
                                                                 cnt, ctx->slab.p, rhs, ctx->rhs_in);   \
    else if (rhs)                                                                                       \
      tree_factor_level<NS_, S_, true><<<g, w * 64, lds, ctx->stream>>>(                                \
          ctx->plan, ctx->p_rec.p, sg.begin, cnt, ctx->slab.p, rhs, ctx->d_fail.p, per_wave);           \
    else                                                                                                \
      tree_factor_level<NS_, S_, false><<<g, w * 64, lds, ctx->stream>>>(                               \
          ctx->plan, ctx->p_rec.p, sg.begin, cnt, ctx->slab.p, rhs, ctx->d_fail.p, per_wave);           \
  }
        if (mode == 0 && lb == 0 && ctx->asm_pending.on) {
          // the assembly rides in this launch: factor workgroups [0, g) read their panels from
          // the Schur blocks, the others gather what the levels above need
          const cxk_context::AsmPending ap = ctx->asm_pending;
          ctx->asm_pending.on = false;
          GatherArgs ga;
          AsmIn ai;
          MakeFusedAssembly(ctx, ap, &ga, &ai);
          // 256 threads per workgroup whatever the level's size: the gather's fixed-order sums
          // (<w,c>, <c,Qc>) are dealt by thread index, and must come out as in assemble_gather
          const int w = 4, g = (cnt + w - 1) / w;
          const size_t lds = (size_t)w * ctx->chol_lds;
          const int gg = GridFor((size_t)std::max<int64_t>(std::max<int64_t>(ga.T, ga.N), 1), 256);
          bool done = false;
#define CXK_LEVEL_ASM(NS_, S_)                                                                          \
  if (sh == ((NS_) << 8 | (S_))) {                                                                      \
    done = true;                                                                                        \
    if (ap.with_rhs != 0)                                                                               \
      tree_factor_level_asm<NS_, S_, true><<<g + gg, w * 64, lds, ctx->stream>>>(                       \
          ctx->plan, ctx->p_rec.p, sg.begin, cnt, ctx->slab.p, rhs, ctx->d_fail.p, per_wave, ai, ga, g); \
    else                                                                                                \
      tree_factor_level_asm<NS_, S_, false><<<g + gg, w * 64, lds, ctx->stream>>>(                      \
          ctx->plan, ctx->p_rec.p, sg.begin, cnt, ctx->slab.p, rhs, ctx->d_fail.p, per_wave, ai, ga, g); \
  }
          CXK_LEVEL_ASM(8, 8)
          CXK_LEVEL_ASM(16, 8)
          CXK_LEVEL_ASM(24, 0)
          CXK_LEVEL_ASM(24, 8)
          CXK_LEVEL_ASM(32, 16)
#undef CXK_LEVEL_ASM
          CXK_DEMAND(done, "internal error: no tree_factor_level_asm instance for the first level's shape");
          continue;
        }
        CXK_LEVEL(8, 8)
        CXK_LEVEL(16, 8)
        CXK_LEVEL(24, 0)
        CXK_LEVEL(24, 8)
        CXK_LEVEL(32, 16)
#undef CXK_LEVEL
      }
      CXK_TRY(hipGetLastError());
      return CXK_SUCCESS;
    }
  }
  const size_t lds = (size_t)waves * ctx->chol_lds;
  // the top [lb, le) is ONE piece: its level table is the level_ptr slice itself (positions into
  // the level-ordered records)
#define CXK_SWEEP(MODE, TOP)                                                                   \
  tree_sweep<MODE, TOP><<<grid, waves * 64, lds, ctx->stream>>>(                               \
      ctx->plan, ctx->p_rec.p, ctx->d_level_ptr.p + lb, ctx->level_ptr[lb],                    \
      is_top ? ctx->level_ptr[lb + 1] - ctx->level_ptr[lb] : maxcnt, le - lb, then_backward ? 1 : 0, \
      ctx->slab.p, rhs, ctx->d_fail.p, per_wave)
  if (mode == 0) {
    if (is_top) CXK_SWEEP(0, true); else CXK_SWEEP(0, false);
  } else if (mode == 1) {
    if (is_top) CXK_SWEEP(1, true); else CXK_SWEEP(1, false);
  } else {
    if (is_top) CXK_SWEEP(2, true); else CXK_SWEEP(2, false);
  }
#undef CXK_SWEEP
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// One launch over a merged level range: one workgroup per connected piece.
int LaunchRange(cxk_context* ctx, cxk_context::SweepRange& r, int mode, bool with_rhs) {
  const int per_wave = (int)(ctx->chol_lds / sizeof(double));
  const int wmax = std::max(1, std::min<int>(8, (int)((kLdsLimit - kRangeMaxRecs * sizeof(SnRec)) / std::max<size_t>(ctx->chol_lds, 8))));
  const int waves = std::max(1, std::min(wmax, r.waves));
  const size_t lds = (size_t)waves * ctx->chol_lds;
  double* rhs = (with_rhs || mode != 0) ? ctx->y.p : nullptr;
#define CXK_RANGE(MODE)                                                                          \
  tree_sweep<MODE, true><<<r.groups, waves * 64, lds, ctx->stream>>>(                            \
      ctx->plan, ctx->rec_r.p, r.wg_lev.p, 0, 0, r.hi - r.lo, 0, ctx->slab.p, rhs, ctx->d_fail.p, per_wave)
  if (mode == 0)
    CXK_RANGE(0);
  else if (mode == 1)
    CXK_RANGE(1);
  else
    CXK_RANGE(2);
#undef CXK_RANGE
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// Bottom-up pass (mode 0 factor or mode 1 forward), optionally continuing straight into the
// top-down backward pass.  The narrow top of the tree is one launch.
int LaunchTreeCore(cxk_context* ctx, int mode, bool with_rhs, bool backward);

// A sweep with the refinement steps the reference's SolveInPlace runs after every solve
// (kkt_solver.cc:233-261); without refinement this is LaunchTreeCore.
int ShardedTree(cxk_context* ctx, int mode, bool with_rhs, bool backward);

int QrFactor(cxk_context* ctx);
int QrSolve(cxk_context* ctx);

int LaunchTreeUntimed(cxk_context* ctx, int mode, bool with_rhs, bool backward);

// (the kernel clocks CXK_CLOCK_TREE / CXK_CLOCK_SOLVE sit here: on the dispatch when the sweep is one
// whole-tree launch, around the launches otherwise)
int LaunchTree(cxk_context* ctx, int mode, bool with_rhs, bool backward) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  const bool solving = backward && (mode != 0 || with_rhs);
  if (!ctx->timing || !solving || !ClockSample(ctx, mode == 0 ? CXK_CLOCK_TREE : CXK_CLOCK_SOLVE, &e0, &e1))
    return LaunchTreeUntimed(ctx, mode, with_rhs, backward);
  const bool one_launch =
      ctx->world == 1 && ctx->refine_iters <= 0 && ctx->solver_mode != 2 && ctx->fused_tree && !ctx->fused_split &&
      (mode == 0 ? (with_rhs && ctx->asm_pending.on && ctx->asm_pending.with_rhs != 0) : ctx->fused_sweep);
  if (one_launch) {
    ctx->clk_e0 = e0;
    ctx->clk_e1 = e1;
  } else {
    CXK_TRY(hipEventRecord(e0, ctx->stream));
  }
  const int rc = LaunchTreeUntimed(ctx, mode, with_rhs, backward);
  if (!one_launch) CXK_TRY(hipEventRecord(e1, ctx->stream));
  ctx->clk_e0 = ctx->clk_e1 = nullptr;
  return rc;
}

int LaunchTreeUntimed(cxk_context* ctx, int mode, bool with_rhs, bool backward) {
  if (mode == 0) ctx->fail_clean = false;  // (whatever this factorization reports stays until the next gather)
  if (ctx->solver_mode == 2) {  // CONEX_QR_FACTORIZATION
    if (mode == 0 && QrFactor(ctx)) return CXK_FAILURE;
    if ((mode != 0 || with_rhs) && backward) return QrSolve(ctx);
    return CXK_SUCCESS;
  }
  if (ctx->world > 1) return ShardedTree(ctx, mode, with_rhs, backward);  // (refinement is single-GPU)
  if (ctx->refine_iters <= 0) return LaunchTreeCore(ctx, mode, with_rhs, backward);
  const int N = ctx->md.N;
  const bool solving = backward && (mode != 0 || with_rhs);
  if (mode == 0) {  // kkt_matrix_ = KKTMatrix() before factoring (kkt_solver.cc:177-179)
    CXK_TRY(hipMemcpyAsync(ctx->slab0.p, ctx->slab.p, sizeof(double) * ctx->slab.n, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->slab0_valid = true;
  }
  if (solving)
    CXK_TRY(hipMemcpyAsync(ctx->rhs0.p, ctx->y.p, sizeof(double) * N, hipMemcpyDeviceToDevice, ctx->stream));
  if (LaunchTreeCore(ctx, mode, with_rhs, backward)) return CXK_FAILURE;
  if (!solving || !ctx->slab0_valid) return CXK_SUCCESS;
  for (int it = 0; it < ctx->refine_iters; it++) {
    kkt_matvec<<<(int)ctx->level_sn.size(), 256, 0, ctx->stream>>>(ctx->plan, ctx->slab0.p, ctx->y.p, ctx->mv_u.p,
                                                                   ctx->mvb.p);
    refine_residual<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, ctx->rhs0.p, ctx->mv_u.p, ctx->fs_ptr.p,
                                                              ctx->fs_src.p, ctx->mvb.p, ctx->y.p, ctx->ysave.p);
    CXK_TRY(hipGetLastError());
    if (LaunchTreeCore(ctx, 1, true, true)) return CXK_FAILURE;
    refine_add<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, ctx->ysave.p, ctx->y.p);
    CXK_TRY(hipGetLastError());
  }
  return CXK_SUCCESS;
}

// The chain at the top of the tree (levels [chain_level, nlev), one supernode each): up and
// straight back down in one launch of one wavefront.  mode 0 factor + forward, mode 1 forward.
int LaunchBackPair(cxk_context* ctx, const cxk_context::BackPair& bp) {
  bool done = false;
#define CXK_BACK_PAIR(NP_, SP_, NC_, SC_)                                                              \
  if (!done && bp.shape_p == ((NP_) << 8 | (SP_)) && bp.shape_c == ((NC_) << 8 | (SC_))) {             \
    done = true;                                                                                       \
    tree_backward_pair<NP_, SP_, NC_, SC_><<<bp.nwg, 576, 0, ctx->stream>>>(ctx->p_rec.p, bp.tab.p,    \
                                                                            ctx->slab.p, ctx->y.p);    \
  }
#define CXK_BACK_PAIR_ROW(NP_, SP_)                                                                    \
  CXK_BACK_PAIR(NP_, SP_, 8, 8)                                                                        \
  CXK_BACK_PAIR(NP_, SP_, 16, 8)                                                                       \
  CXK_BACK_PAIR(NP_, SP_, 24, 0) CXK_BACK_PAIR(NP_, SP_, 24, 8) CXK_BACK_PAIR(NP_, SP_, 32, 16)
  CXK_BACK_PAIR_ROW(8, 8)
  CXK_BACK_PAIR_ROW(16, 8)
  CXK_BACK_PAIR_ROW(24, 0)
  CXK_BACK_PAIR_ROW(24, 8)
  CXK_BACK_PAIR_ROW(32, 16)
#undef CXK_BACK_PAIR_ROW
#undef CXK_BACK_PAIR
  CXK_DEMAND(done, "internal error: no tree_backward_pair instance for the levels' shapes");
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

int LaunchChain(cxk_context* ctx, int mode) {
  const int nlev = (int)ctx->level_ptr.size() - 1;
  // one supernode per chain level: their records are consecutive in level order
  const int pos0 = ctx->level_ptr[ctx->chain_level], nchain = nlev - ctx->chain_level;
    const int sa = ctx->chain_a, sb = ctx->chain_b;
    bool done = false;
#define CXK_CHAIN(NA_, SA_, NB_, SB_)                                                                       \
  if (!done && sa == ((NA_) << 8 | (SA_)) && sb == ((NB_) << 8 | (SB_))) {                                  \
    done = true;                                                                                            \
    const size_t lds = sizeof(double) * 65 * ((NA_) > (NB_) ? (NA_) : (NB_)) + sizeof(SnRec) * (size_t)std::min(nchain, kChainRing); \
    if (mode == 0)                                                                                          \
      tree_chain_lean<0, NA_, SA_, NB_, SB_><<<1, 64, lds, ctx->stream>>>(                                  \
          ctx->plan, ctx->p_rec.p, pos0, nchain, ctx->slab.p, ctx->y.p, ctx->d_fail.p, RhsIn{});            \
    else                                                                                                    \
      tree_chain_lean<1, NA_, SA_, NB_, SB_><<<1, 64, lds, ctx->stream>>>(                                  \
          ctx->plan, ctx->p_rec.p, pos0, nchain, ctx->slab.p, ctx->y.p, ctx->d_fail.p, ctx->rhs_in);        \
  }
    CXK_CHAIN(8, 8, 8, 8)
    CXK_CHAIN(16, 8, 16, 8)
    CXK_CHAIN(24, 0, 24, 0)
    CXK_CHAIN(24, 8, 24, 8)
    CXK_CHAIN(32, 16, 32, 16)
    CXK_CHAIN(8, 8, 24, 0)
    CXK_CHAIN(16, 8, 24, 0)
    CXK_CHAIN(8, 8, 16, 8)
    CXK_CHAIN(24, 0, 24, 8)
    CXK_CHAIN(24, 0, 32, 16)
#undef CXK_CHAIN
    CXK_DEMAND(done, "internal error: no tree_chain_lean instance for the chain's shapes");
    CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// Arguments of a whole-tree launch (tree_fused.hip); rebuilds the hand-off slots first when an
// earlier launch reported that a wait ran out.
int MakeFusedTreeArgs(cxk_context* ctx, FusedTreeArgs* out) {
  if (*ctx->fx_flag != 0.0) {
    // a wait ran out in an earlier launch (reported as a failed factorization): the hand-off slots
    // may hold anything -- rebuild both sets before they are trusted again
    CXK_TRY(hipStreamSynchronize(ctx->stream));
    CXK_TRY(hipMemcpy(ctx->fx_hand.p, ctx->fx_hand_init.data(), sizeof(double) * ctx->fx_hand_init.size(), hipMemcpyHostToDevice));
    unsigned long long bits = kFusedSentinel;
    double sent;
    memcpy(&sent, &bits, sizeof(sent));
    std::vector<double> ys(ctx->fx_ysig.n, sent);
    CXK_TRY(hipMemcpy(ctx->fx_ysig.p, ys.data(), sizeof(double) * ys.size(), hipMemcpyHostToDevice));
    if (ctx->fx_done.p) {
      CXK_TRY(hipMemset(ctx->fx_done.p, 0, sizeof(unsigned long long) * ctx->fx_done.n));
      ctx->fx_done_target = 0;
    }
    *ctx->fx_flag = 0.0;
    ctx->timeout_pending = true;  // (what cxk_sync / cxk_factor_status act on: FusedTimedOut)
  }
  FusedTreeArgs& a = *out;
  a.rec = ctx->fx_rec.p;
  a.count = (int)ctx->level_sn.size();
  a.G = ctx->G.p;
  a.AWc = ctx->AWc.p;
  a.AQcc = ctx->AQcc.p;
  a.b = ctx->b.p;
  a.AW = ctx->AW.p;
  a.AQc = ctx->AQc.p;
  a.slab = ctx->slab.p;
  a.y = ctx->y.p;
  a.pub = ctx->fx_pub.p;
  a.tg_reg = ctx->tg_reg.p;
  a.xreg = ctx->fx_xreg.p;
  a.xsrc = ctx->fx_xsrc.p;
  a.rsrc = ctx->fx_rsrc.p;
  a.hand = ctx->fx_hand.p;
  a.hand_stride = (long long)(ctx->fx_hand.n / 2);
  a.updb_base = ctx->fx_updb_base;
  a.ysig = ctx->fx_ysig.p;
  a.ysig_stride = (long long)(ctx->fx_ysig.n / 2);
  a.gen = (int)(ctx->fused_gen++ & 1u);
  a.tgen = (int)(ctx->fused_tgen & 1u);
  a.fwd_stride = ctx->fx_fwd_stride;
  a.y_stride = ctx->md.N;
  a.y3 = ctx->y3.p;
  a.fail = ctx->d_fail.p;
  a.tag = ctx->fail_tag;
  a.k = a.bs = a.cs = a.cb = a.cq = a.cw = 0;
  a.k_from = nullptr;
  a.comb = 0;
  a.form = 0;
  a.sc = ctx->sc.p;
  a.sys_sc = ctx->sys_sc.p;
  a.K = (int)ctx->cons.size();
  a.host_flag = ctx->fx_flag;
  a.up_sleep = 30;  // units of 64 cycles a level takes at least (tree_fused.h)
  // sharded contexts (kFusedShardUp / kFusedShardTop)
  a.count_up = ctx->fused_shard ? ctx->fused_up : a.count;
  a.x = ctx->xbuf.p;
  a.n_xs = ctx->n_xs;
  a.n_xv = ctx->n_xv;
  a.xg = ctx->fx_xg.p;
  a.as_src = ctx->as_src.p;
  a.xs_pt = ctx->xs_pt.p;
  a.pt_ptr = ctx->pt_ptr.p;
  a.pt_src = ctx->pt_src.p;
  a.xr = ctx->fx_xr.p;
  a.rs_src = ctx->rs_src.p;
  a.pf_ptr = ctx->pf_ptr.p;
  a.pf_src = ctx->pf_src.p;
  a.done = ctx->fx_done.p;
  a.done_target = 0;
  return CXK_SUCCESS;
}

int ShardAllReduce(cxk_context* ctx, double* buf, size_t count, int op);
long ExchangeCount(const cxk_context* ctx);

// Test hook (cxk_debug_fused_timeout_at): behind the launch just enqueued, what a wait of it that ran out
// reports -- d_fail[1] = tag on the device and the pinned host word.  Nothing else.  The host
// word is raised before this returns, or (CXK_DEBUG_FUSED_STREAM_ORDERED) by a host function on the stream,
// as late as a launch that is still running when the host goes on would raise it.
void RaiseHostWord(void* flag) { *static_cast<double*>(flag) = 1.0; }
int DebugReportTimeout(cxk_context* ctx) {
  CXK_TRY(hipMemcpyAsync(ctx->d_fail.p + 1, &ctx->asm_tag, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (ctx->debug_stream_ordered) {
    CXK_TRY(hipLaunchHostFunc(ctx->stream, RaiseHostWord, ctx->fx_flag));
    return CXK_SUCCESS;
  }
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  *ctx->fx_flag = 1.0;
  return CXK_SUCCESS;
}

// The factor-and-solve of a sharded context on the whole-tree kernels: own subtrees up with the pack of
// the exchange buffer behind them (one launch), the sum all-reduce, the replicated top straight from
// the buffer and the way back down the own subtrees (one launch).  Consumes the pending assembly.
int LaunchFusedShard(cxk_context* ctx) {
  const cxk_context::AsmPending ap = ctx->asm_pending;
  ctx->asm_pending.on = false;
  FusedTreeArgs a;
  if (MakeFusedTreeArgs(ctx, &a)) return CXK_FAILURE;
  ctx->asm_tag = ctx->asm_tag >= (1 << 30) ? 1 : ctx->asm_tag + 1;
  a.tag = ctx->fail_tag = ctx->asm_tag;
  a.k = ap.k;
  a.bs = ap.bs;
  a.cs = ap.cs;
  a.cb = ap.cb;
  a.cq = ap.cq;
  a.cw = ap.cw;
  a.comb = ap.with_rhs == 2;
  a.done_target = ++ctx->fx_done_target;  // (up launches so far: kFusedShardUp's counters)
  const bool hook = ctx->debug_timeout_at >= 0 && ctx->fused_launches++ == ctx->debug_timeout_at;
  CXK_TRY(LaunchFusedTree(a, ctx->fused_sa, ctx->fused_sb, kFusedShardUp, ctx->stream));
  if (hook && ctx->debug_timeout_site == CXK_DEBUG_FUSED_SHARD_UP && DebugReportTimeout(ctx)) return CXK_FAILURE;
  if (*ctx->fx_flag != 0.0) {
    // a wait of this launch ran out and the host already sees it: make sure it travels (the launch's
    // tail folds what it sees itself, ShardPackTail) -- failure word and time-out count of the exchange
    static const double kTimedOut[2] = {1.0, 1.0};
    CXK_TRY(hipMemcpyAsync(ctx->xbuf.p + ExchangeCount(ctx) - 2, kTimedOut, sizeof(kTimedOut), hipMemcpyHostToDevice,
                           ctx->stream));
  }
  if (ShardAllReduce(ctx, ctx->xbuf.p, (size_t)ExchangeCount(ctx), 0 /* kOpSum */)) return CXK_FAILURE;
  ctx->shard_fused_tag = ctx->asm_tag;
  ctx->shard_launch_collectives = ctx->collectives;  // (what has gone out behind the launch: ResolveShardTimeout)
  CXK_TRY(LaunchFusedTree(a, ctx->fused_sa, ctx->fused_sb, kFusedShardTop, ctx->stream));
  if (hook && ctx->debug_timeout_site == CXK_DEBUG_FUSED_SHARD_TOP && DebugReportTimeout(ctx)) return CXK_FAILURE;
  return CXK_SUCCESS;
}

// Assembly gather, factorization with the first right-hand side, back substitution: one launch.
// Consumes the pending assembly.
int LaunchFusedTreeSolve(cxk_context* ctx) {
  const cxk_context::AsmPending ap = ctx->asm_pending;
  ctx->asm_pending.on = false;
  FusedTreeArgs a;
  if (MakeFusedTreeArgs(ctx, &a)) return CXK_FAILURE;
  ctx->asm_tag = ctx->asm_tag >= (1 << 30) ? 1 : ctx->asm_tag + 1;
  a.tag = ctx->fail_tag = ctx->asm_tag;
  a.k = ap.k;
  a.bs = ap.bs;
  a.cs = ap.cs;
  a.cb = ap.cb;
  a.cq = ap.cq;
  a.cw = ap.cw;
  a.comb = ap.with_rhs == 2;
  if (ap.with_rhs == 3) {  // (cxk_factor_solve_triple_async: TripleOk has checked that the one-launch sweep applies)
    ctx->fused_tgen++;
    CXK_TRY(LaunchFusedTree(a, ctx->fused_sa, ctx->fused_sb, kFusedTriple, ctx->stream, ctx->clk_e0, ctx->clk_e1));
  } else if (ctx->fused_split) {
    CXK_TRY(LaunchFusedTree(a, ctx->fused_sa, ctx->fused_sb, kFusedUp, ctx->stream));
    CXK_TRY(LaunchFusedTree(a, ctx->fused_sa, ctx->fused_sb, kFusedDown, ctx->stream));
  } else {
    CXK_TRY(LaunchFusedTree(a, ctx->fused_sa, ctx->fused_sb, kFusedFull, ctx->stream, ctx->clk_e0, ctx->clk_e1));
  }
  // test hook (CXK_DEBUG_FUSED_TIMEOUT_AT=k at cxk_create, or cxk_debug_fused_timeout_at): the k-th factor launch
  if (ctx->debug_timeout_at >= 0 && ctx->fused_launches++ == ctx->debug_timeout_at &&
      ctx->debug_timeout_site == CXK_DEBUG_FUSED_FACTOR && DebugReportTimeout(ctx))
    return CXK_FAILURE;
  return CXK_SUCCESS;
}

// A solve-only sweep on the stored factor: forward and back substitution, one launch.  The
// right-hand side is in y, or formed inside the kernel (ctx->rhs_in, SolveWithRhs).
int LaunchFusedTreeSweep(cxk_context* ctx) {
  FusedTreeArgs a;
  if (MakeFusedTreeArgs(ctx, &a)) return CXK_FAILURE;
  const RhsIn& ri = ctx->rhs_in;
  a.form = ri.form;
  a.k = ri.k;
  a.k_from = ri.k_from;
  a.bs = ri.bs;
  a.cs = ri.cs;
  a.cb = ri.cb;
  a.cq = ri.cq;
  a.cw = ri.cw;
  if (ctx->fused_split) {
    CXK_TRY(LaunchFusedTree(a, ctx->fused_sa, ctx->fused_sb, kFusedForward, ctx->stream));
    CXK_TRY(LaunchFusedTree(a, ctx->fused_sa, ctx->fused_sb, kFusedDown, ctx->stream));
  } else {
    CXK_TRY(LaunchFusedTree(a, ctx->fused_sa, ctx->fused_sb, kFusedSolve, ctx->stream, ctx->clk_e0, ctx->clk_e1));
  }
  return CXK_SUCCESS;
}

// A wait of a whole-tree launch ran out (the launch reports it as a failed factorization and through
// the pinned word).  tree_fused is deadlock-free only while its whole grid is resident, i.e. while the
// device is this context's alone; on a device shared with other streams / processes a wavefront can
// wait for one that was never dispatched.  Nothing is wrong with the matrix then: the context gives
// the whole-tree launch up and sweeps its tree level by level from here on (the CXK_NO_FUSED_TREE
// path: kernel boundaries instead of in-kernel waits), and the caller redoes the sweep.
bool FusedTimedOut(const cxk_context* ctx) { return ctx->timeout_pending || (ctx->fx_flag && *ctx->fx_flag != 0.0); }

int DisableFusedTree(cxk_context* ctx) {
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  *ctx->fx_flag = 0.0;
  ctx->timeout_pending = false;
  ctx->fused_tree = false;
  ctx->fused_sweep = false;
  ctx->y3_valid = false;
  ctx->y_deferred = false;  // (its three parts came from the launch that timed out)
  ctx->fused_timeouts++;
  fprintf(stderr, "conex_kkt_hip: a wait inside the whole-tree launch ran out (device shared with other work?); "
                  "this context sweeps its elimination tree level by level from now on\n");
  return CXK_SUCCESS;
}

// ... and the latest factor-and-solve again on the level kernels: the Schur blocks are still in the
// arena, the right-hand side was cb b + cq AQc + cw AW with the coefficients of ctx->rhs_c.
int RedoFactorSolveOnLevels(cxk_context* ctx) {
  if (DisableFusedTree(ctx)) return CXK_FAILURE;
  const int N = ctx->md.N;
  ctx->asm_pending.on = false;
  ctx->asm_deferred = false;
  if (LaunchGather(ctx, false, 0, 0, 0)) return CXK_FAILURE;
  CXK_TRY(hipMemsetAsync(ctx->d_fail.p, 0, 2 * sizeof(int), ctx->stream));
  build_rhs_comb<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, ctx->rhs_c[0], ctx->rhs_c[1], ctx->rhs_c[2], ctx->b.p,
                                                           ctx->AQc.p, ctx->AW.p, ctx->y.p, ctx->d_fail.p);
  CXK_TRY(hipGetLastError());
  if (LaunchTree(ctx, 0, true, true)) return CXK_FAILURE;
  ctx->factor_seq = ++ctx->seq;
  return CXK_SUCCESS;
}

int LaunchTreeCore(cxk_context* ctx, int mode, bool with_rhs, bool backward) {
  if (mode == 0 && with_rhs && backward && ctx->fused_tree && ctx->asm_pending.on && ctx->asm_pending.with_rhs != 0)
    return LaunchFusedTreeSolve(ctx);
  if (mode == 1 && backward && ctx->fused_tree && ctx->fused_sweep) return LaunchFusedTreeSweep(ctx);
  if (ctx->use_ldlt && mode == 0) CXK_TRY(hipMemsetAsync(ctx->d_reg.p, 0, sizeof(int), ctx->stream));
  const int nlev = (int)ctx->level_ptr.size() - 1;
  const int top = ctx->top_level;
  // levels below the top: merged ranges where they exist, single levels otherwise
  auto range_at = [&](int l) -> cxk_context::SweepRange* {
    if (ctx->no_ranges) return nullptr;
    for (auto& r : ctx->ranges)
      if (r->lo == l) return r.get();
    return nullptr;
  };
  std::vector<std::pair<int, cxk_context::SweepRange*>> order;  // (first level, range or null)
  for (int l = 0; l < top;) {
    cxk_context::SweepRange* r = range_at(l);
    order.emplace_back(l, r);
    l = r ? r->hi : l + 1;
  }
  // Bottom-up sweeps stay one launch per level: a factor step is long (thousands of cycles of
  // elimination) and a kernel boundary buys full width for ~2 us; merging levels only pays on the
  // way down, where a level step is a short back-substitution (measured: -30 % on C4).
  // mode 0 with a dense range: levels below it as usual, then ONE dense factorization (+ solves)
  // of everything from dense_level up (kernels_kkt_top.hip.h)
  const bool dense = mode == 0 && ctx->top_dense.on;
  // the chain at the top: up and straight back down in one launch of one wavefront
  const bool chain = !dense && backward && ctx->chain_level < nlev && (mode == 1 || (mode == 0 && with_rhs));
  const int up_end = dense ? ctx->dense_level : (chain ? ctx->chain_level : top);
  for (int l = 0; l < up_end; l++)
    if (LaunchSweep(ctx, l, l + 1, mode, false, with_rhs)) return CXK_FAILURE;
  if (chain && LaunchChain(ctx, mode)) return CXK_FAILURE;
  if (dense) {
    double* rhs = with_rhs ? ctx->y.p : nullptr;
    const int wb = with_rhs && backward;
    const TopDenseArgs& ta = ctx->top_dense.args;
#define CXK_TOP_DENSE(TM) \
  tree_top_dense<TM><<<1, 256, kTopDenseLds, ctx->stream>>>(ctx->plan, ta, ctx->slab.p, rhs, ctx->d_fail.p, with_rhs, wb)
    if (ta.T <= 32)
      CXK_TOP_DENSE(32);
    else if (ta.T <= 40)
      CXK_TOP_DENSE(40);
    else if (ta.T <= 48)
      CXK_TOP_DENSE(48);
    else if (ta.T <= 56)
      CXK_TOP_DENSE(56);
    else
      CXK_TOP_DENSE(64);
#undef CXK_TOP_DENSE
    CXK_TRY(hipGetLastError());
  } else if (top < nlev) {
    if (LaunchSweep(ctx, top, nlev, mode, backward, with_rhs)) return CXK_FAILURE;
  }
  if (backward)
    for (auto it = order.rbegin(); it != order.rend(); ++it) {
      if (dense && it->first >= ctx->dense_level) continue;  // solved inside the dense kernel
      if (chain && it->first >= ctx->chain_level) continue;  // solved inside the chain kernel
      if (!it->second && it->first >= 1 && it->first < (int)ctx->back_pairs.size() && ctx->back_pairs[it->first] &&
          std::next(it) != order.rend() && std::next(it)->first == it->first - 1 && !std::next(it)->second) {
        if (LaunchBackPair(ctx, *ctx->back_pairs[it->first])) return CXK_FAILURE;
        ++it;  // the lower level went with it
        continue;
      }
      if (it->second ? LaunchRange(ctx, *it->second, 2, true) : LaunchSweep(ctx, it->first, it->first + 1, 2, false, true))
        return CXK_FAILURE;
    }
  return CXK_SUCCESS;
}

// ---------------------------------------------------------------- QR solver mode (B10)
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

// ---------------------------------------------------------------- sharded contexts
enum { kOpSum = 0, kOpMax = 1, kOpMin = 2 };

// In-place all-reduce of `count` doubles of device memory across the ranks, ordered on the
// context's stream (RCCL) or complete on return (caller-supplied function).
int ShardAllReduce(cxk_context* ctx, double* buf, size_t count, int op) {
  if (ctx->world <= 1 || count == 0) return CXK_SUCCESS;
  ctx->collectives++;
  if (ctx->coll_fn) {
    CXK_DEMAND(ctx->coll_fn(ctx->coll_user, buf, (long)count, op, ctx->stream) == 0,
               "the caller-supplied all-reduce reported a failure");
    return CXK_SUCCESS;
  }
  CXK_DEMAND(ctx->rccl.comm != nullptr,
             "sharded context without a communicator: call cxk_comm_init_rccl or cxk_comm_set_allreduce first");
  const ncclRedOp_t rop = op == kOpSum ? ncclSum : (op == kOpMax ? ncclMax : ncclMin);
  const ncclResult_t r = ctx->rccl.AllReduce(buf, buf, count, ncclDouble, rop, ctx->rccl.comm, ctx->stream);
  if (r != ncclSuccess) {
    ctx->err = std::string("ncclAllReduce: ") + (ctx->rccl.GetErrorString ? ctx->rccl.GetErrorString(r) : "error");
    fprintf(stderr, "conex_kkt_hip: %s\n", ctx->err.c_str());
    return CXK_FAILURE;
  }
  return CXK_SUCCESS;
}

long ExchangeCount(const cxk_context* ctx) { return (long)(ctx->n_xs + 3 * (int64_t)ctx->n_xv + 4); }

// One sweep of a sharded context.  Bottom-up over this rank's subtrees (mode 0 factor [+ forward
// substitution when with_rhs], mode 1 forward substitution), ONE sum all-reduce of what the
// subtrees contribute to the replicated top of the tree --
//   mode 0: [top slab entries | AW_T | AQc_T | forward values | <w,c> <c,Qc> | failure flag | time-out count]
//           (supernodal_assembler.cc:103-111,162-164 and block_triangular_operations.cc:209-215 are
//            the sums that cross ranks here),
//   mode 1: [forward values | time-out mark]  --
// then the top on every rank (bit-identical: same data, same kernels) and, when `backward`, the
// back-substitution down this rank's subtrees.
int ShardedTop(cxk_context* ctx, int mode, bool rhs, bool backward);
int ShardedTree(cxk_context* ctx, int mode, bool with_rhs, bool backward) {
  if (mode == 0 && with_rhs && backward && ctx->fused_tree && ctx->fused_shard && ctx->asm_pending.on &&
      ctx->asm_pending.with_rhs != 0)
    return LaunchFusedShard(ctx);
  if (ctx->use_ldlt && mode == 0) CXK_TRY(hipMemsetAsync(ctx->d_reg.p, 0, sizeof(int), ctx->stream));
  const int cut = ctx->cut_level;
  const bool rhs = with_rhs || mode != 0;
  for (int l = 0; l < cut; l++)
    if (LaunchSweep(ctx, l, l + 1, mode, false, rhs)) return CXK_FAILURE;
  ExchangeArgs a = MakeExchange(ctx, 0, 0, 0);
  a.cb = ctx->rhs_c[0];
  a.cq = ctx->rhs_c[1];
  a.cw = ctx->rhs_c[2];
  const size_t work = (size_t)std::max<int64_t>(std::max<int64_t>(ctx->n_xs, ctx->n_xv), 1);
  if (mode == 0) {
    exchange_pack<<<GridFor(work, 256), 256, 0, ctx->stream>>>(a);
    CXK_TRY(hipGetLastError());
    if (ShardAllReduce(ctx, ctx->xbuf.p, (size_t)ExchangeCount(ctx), kOpSum)) return CXK_FAILURE;
    if (with_rhs)
      exchange_unpack<<<GridFor(work, 256), 256, 0, ctx->stream>>>(a);
    else
      exchange_unpack_matrix<<<GridFor(work, 256), 256, 0, ctx->stream>>>(a);
  } else if (ctx->n_xv > 0) {
    a.tag = ctx->fx_flag ? ctx->shard_fused_tag : 0;  // (x[n_xv]: the time-out mark, ShardMark)
    a.host_flag = ctx->fx_flag;
    exchange_pack_solve<<<GridFor((size_t)ctx->n_xv, 256), 256, 0, ctx->stream>>>(a);
    CXK_TRY(hipGetLastError());
    if (ShardAllReduce(ctx, ctx->xbuf.p, (size_t)ctx->n_xv + 1, kOpSum)) return CXK_FAILURE;
    exchange_unpack_solve<<<GridFor((size_t)ctx->n_xv, 256), 256, 0, ctx->stream>>>(a);
  }
  CXK_TRY(hipGetLastError());
  return ShardedTop(ctx, mode, rhs, backward);
}

// The part of ShardedTree behind the exchange: the replicated top, levels [cut, nlev), and when
// `backward` the way back down this rank's subtrees.
int ShardedTop(cxk_context* ctx, int mode, bool rhs, bool backward) {
  const int nlev = ctx->nlev, cut = ctx->cut_level, top = ctx->top_level;
  const bool chain = backward && rhs && ctx->chain_level < nlev && ctx->chain_level >= cut;
  const int up_end = chain ? ctx->chain_level : top;
  for (int l = cut; l < up_end; l++)
    if (LaunchSweep(ctx, l, l + 1, mode, false, rhs)) return CXK_FAILURE;
  if (chain) {
    if (LaunchChain(ctx, mode)) return CXK_FAILURE;
  } else if (top < nlev) {
    if (LaunchSweep(ctx, top, nlev, mode, backward, rhs)) return CXK_FAILURE;
  }
  if (backward)
    for (int l = std::min(top, up_end) - 1; l >= 0; l--) {
      if (l >= 1 && l < (int)ctx->back_pairs.size() && ctx->back_pairs[l]) {
        // (a rank's level lists hold its own subtrees and the replicated top: a pair is local either way)
        if (LaunchBackPair(ctx, *ctx->back_pairs[l])) return CXK_FAILURE;
        l--;
        continue;
      }
      if (LaunchSweep(ctx, l, l + 1, 2, false, true)) return CXK_FAILURE;
    }
  return CXK_SUCCESS;
}

// A wait of this rank's kFusedShardTop ran out.  That launch ran behind the exchange, so no other rank
// knows: this rank redoes its part on the level kernels without a collective -- the reduced exchange
// buffer is still there (the top launch only reads it), the factor of its own subtrees is in the slab
// (the top launch only reads that too), and the right-hand side is cb b + cq AQc + cw AW with the
// coefficients of ctx->rhs_c.  Forward substitution down its subtrees again (the top launch may have
// overwritten some of their y), the unpack, the top and the way back down: what ShardedTree does
// around its all-reduce.
int RedoShardTopOnLevels(cxk_context* ctx) {
  if (DisableFusedTree(ctx)) return CXK_FAILURE;
  const int N = ctx->md.N;
  CXK_TRY(hipMemsetAsync(ctx->d_fail.p, 0, 3 * sizeof(int), ctx->stream));  // (the time-out mark with them)
  build_rhs_comb<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, ctx->rhs_c[0], ctx->rhs_c[1], ctx->rhs_c[2], ctx->b.p,
                                                           ctx->AQc.p, ctx->AW.p, ctx->y.p);
  CXK_TRY(hipGetLastError());
  for (int l = 0; l < ctx->cut_level; l++)
    if (LaunchSweep(ctx, l, l + 1, 1, false, true)) return CXK_FAILURE;
  ExchangeArgs a = MakeExchange(ctx, 0, 0, 0);
  a.cb = ctx->rhs_c[0];
  a.cq = ctx->rhs_c[1];
  a.cw = ctx->rhs_c[2];
  const size_t work = (size_t)std::max<int64_t>(std::max<int64_t>(ctx->n_xs, ctx->n_xv), 1);
  exchange_unpack<<<GridFor(work, 256), 256, 0, ctx->stream>>>(a);
  CXK_TRY(hipGetLastError());
  return ShardedTop(ctx, 0, true, true);
}

extern "C" int SyncMailbox(cxk_context* ctx);  // (defined with the mailbox entry points)

// Sharded contexts: what a time-out of a whole-tree launch means, settled once per factorization and the
// same way on every rank.  Called with this rank's host word raised, or with the mailbox of the latest
// factorization read and reporting failure.  Two marks that reach every rank tell the cases apart: the
// exchange buffer's time-out count (ExchangeCount - 1: ShardPackTail, LaunchFusedShard), and d_fail[2] =
// the launch's tag, which the solve exchanges and step reductions behind the launch set on every rank
// when the launch's wait ran out on any (ShardMark).
//   a mark: a wait of some rank's kFusedShardUp ran out (it travelled with the exchange), or one of its
//        kFusedShardTop ran out and a solve sweep or step reduction went out behind it (it travelled with
//        that): every rank's mailbox reports a failed factorization, every rank gives the whole-tree
//        launch up (same collectives on the level kernels) and reports the time-out through
//        cxk_fused_tree_timed_out -- the caller redoes its iteration on every rank.
//   no mark, own word raised, no collective behind the launch: a wait of this rank's kFusedShardTop ran
//        out and nothing has used it yet: RedoShardTopOnLevels, with no collective, and nothing is
//        reported -- the other ranks cannot tell the difference.
//   no mark, own word raised, collectives without a mark behind the launch (the step scalars: cxk_get_y
//        and cxk_line_search settle first, SettleBeforeUnmarked): the same redo, so that the ranks stay
//        in step, and a warning -- what those collectives carried came from the timed-out launch.
int ResolveShardTimeout(cxk_context* ctx) {
  if (ctx->world <= 1 || !ctx->fx_flag || ctx->shard_settled_seq == ctx->factor_seq) return CXK_SUCCESS;
  const bool failed = ctx->mb && ctx->mb_seen >= ctx->factor_seq && ctx->mbv[10] != 0.0;
  if (!failed && !FusedTimedOut(ctx)) return CXK_SUCCESS;  // (the success path: two host reads)
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  const bool own = FusedTimedOut(ctx);
  double up_count = 0;
  int mark = 0;
  CXK_TRY(hipMemcpy(&up_count, ctx->xbuf.p + ExchangeCount(ctx) - 1, sizeof(double), hipMemcpyDeviceToHost));
  CXK_TRY(hipMemcpy(&mark, ctx->d_fail.p + 2, sizeof(int), hipMemcpyDeviceToHost));
  ctx->shard_settled_seq = ctx->factor_seq;
  if (up_count > 0 || (ctx->shard_fused_tag != 0 && mark == ctx->shard_fused_tag)) {
    if (DisableFusedTree(ctx)) return CXK_FAILURE;
    ctx->timeout_unreported = true;
    CXK_TRY(hipMemsetAsync(ctx->d_fail.p + 1, 0, 2 * sizeof(int), ctx->stream));  // (settled: no mark goes out again)
  } else if (own) {
    if (ctx->collectives != ctx->shard_launch_collectives)
      fprintf(stderr, "conex_kkt_hip: collectives without the time-out mark went out behind the timed-out "
                      "whole-tree launch; what they carried from this rank is not trustworthy\n");
    if (RedoShardTopOnLevels(ctx) || SyncMailbox(ctx)) return CXK_FAILURE;
  }
  return CXK_SUCCESS;
}
// Before a collective that carries no time-out mark: a launch still unsettled with nothing behind it yet is
// settled first (the stream is waited for once per factorization, only by these entry points).
int SettleBeforeUnmarked(cxk_context* ctx) {
  if (ctx->world <= 1 || !ctx->fx_flag || ctx->shard_settled_seq == ctx->factor_seq ||
      ctx->shard_fused_tag == 0 || ctx->collectives != ctx->shard_launch_collectives)
    return CXK_SUCCESS;
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  return ResolveShardTimeout(ctx);
}

int CheckReady(cxk_context* ctx) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(ctx->finalized, "context not finalized");
  CXK_DEMAND(ctx->device >= 0,
             "no HIP device bound to this context: the KKT path has no CPU fallback");
  CXK_DEMAND(ctx->device_ready, "device state of this context was not built (cxk_finalize failed)");
  return CXK_SUCCESS;
}

// The current HIP device is per-thread state: every entry point binds the context's device for
// its own duration and restores the caller's (another thread, a second context on another GPU,
// or a host framework that switched devices in between would otherwise launch on the wrong one).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int want) {
    if (want < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != want) switched = hipSetDevice(want) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched && prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
// cxk_kkt_solve_async and the factor-and-solve entry points fold the assembly into the first
// factor level when the tree allows it (BuildPlans) and nothing needs the assembled system as
// such: Cholesky sweeps, no refinement copy (sharded contexts: when the first level lies below the cut).
bool FusedAssembly(const cxk_context* ctx) {
  return (ctx->fused_asm || ctx->fused_tree) && ctx->solver_mode != 2 && ctx->refine_iters <= 0 && !ctx->no_lean;
}
// cxk_assemble leaves the gather to the factorization that normally follows; any other entry point
// that runs first gets the assembled system by the separate launch.
int LaunchStepScalars(cxk_context* ctx) {
  if (ctx->world > 1) {
    // every rank sums over its own share of the variables, the four dot products are then summed
    step_scalars_masked<<<1, 1024, 0, ctx->stream>>>(ctx->md.N, ctx->d_count_mask.p, ctx->b.p, ctx->AQc.p, ctx->y.p,
                                                     ctx->sys_sc.p, ctx->scal_out.p);
    CXK_TRY(hipGetLastError());
    if (ShardAllReduce(ctx, ctx->scal_out.p, 4, kOpSum)) return CXK_FAILURE;
  } else {
    step_scalars<<<1, 1024, 0, ctx->stream>>>(ctx->md.N, ctx->b.p, ctx->AQc.p, ctx->y.p,
                                              ctx->sys_sc.p, ctx->scal_out.p);
  }
  CXK_TRY(hipGetLastError());
  ctx->scal_seq = ++ctx->seq;
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
int FlushDeferred(cxk_context* ctx, bool keep_scalars = false, bool keep_y = false) {
  if (ctx->asm_deferred) {
    ctx->asm_deferred = false;
    if (LaunchGather(ctx, false, 0, 0, 0)) return CXK_FAILURE;
  }
  if (!keep_y && FlushDirection(ctx)) return CXK_FAILURE;  // (before the scalars: they read y)
  if (ctx->scal_deferred && !keep_scalars) {
    ctx->scal_deferred = false;
    if (LaunchStepScalars(ctx)) return CXK_FAILURE;
  }
  return CXK_SUCCESS;
}
// The three solutions of cxk_factor_solve_triple_async hold for the b, the W, the slab and the factor of that
// launch: an entry point that changes one of them drops them (a direction already asked for is formed first).
int DropTriple(cxk_context* ctx) {
  if (FlushDirection(ctx)) return CXK_FAILURE;
  ctx->y3_valid = false;
  return CXK_SUCCESS;
}
#define CXK_ENTER_KEEP(ctx)                     \
  if (CheckReady(ctx)) return CXK_FAILURE;      \
  (ctx)->calls++;                               \
  DeviceGuard cxk_device_guard_((ctx)->device); \
  if (ResolveShardTimeout(ctx)) return CXK_FAILURE
#define CXK_ENTER(ctx)   \
  CXK_ENTER_KEEP(ctx);   \
  if (FlushDeferred(ctx)) return CXK_FAILURE

}  // namespace

// =================================================================== C-ABI
extern "C" {

int cxk_create(int num_vars, int device, void* stream, cxk_context** out) {
  if (!out || num_vars < 0) return CXK_FAILURE;
  cxk_context* ctx = new cxk_context();
  if (const char* v = getenv("CXK_DEBUG_FUSED_TIMEOUT_AT")) ctx->debug_timeout_at = atoi(v);
  ctx->num_vars = num_vars;
  ctx->device = device;
  ctx->stream = static_cast<hipStream_t>(stream);
  ctx->prepare_lds = getenv("CXK_PREPARE_LDS") != nullptr;
  ctx->no_step_tail = getenv("CXK_NO_STEP_TAIL") != nullptr || ctx->prepare_lds;
  ctx->no_triple = getenv("CXK_NO_TRIPLE") != nullptr;
  ctx->no_y_deferral = getenv("CXK_NO_Y_DEFERRAL") != nullptr;
  ctx->no_device_mu = getenv("CXK_NO_DEVICE_MU") != nullptr;
  if (device >= 0) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || device >= count) {
      fprintf(stderr, "conex_kkt_hip: HIP device %d not available (%s)\n", device,
              e == hipSuccess ? "out of range" : hipGetErrorString(e));
      delete ctx;
      return CXK_FAILURE;
    }
    if (hipSetDevice(device) != hipSuccess) {
      delete ctx;
      return CXK_FAILURE;
    }
  }
  *out = ctx;
  return CXK_SUCCESS;
}

void cxk_destroy(cxk_context* ctx) {
  if (!ctx) return;
  for (auto& pr : ctx->ev_pool) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  for (auto& m : ctx->phase_marks) (void)hipEventDestroy(m.first);
  for (hipEvent_t e : ctx->phase_pool) (void)hipEventDestroy(e);
  if (ctx->rccl.comm && ctx->rccl.CommDestroy) ctx->rccl.CommDestroy(ctx->rccl.comm);
  if (ctx->mb) (void)hipHostFree(ctx->mb);
  if (ctx->pin_y) (void)hipHostFree(ctx->pin_y);
  if (ctx->fx_flag) (void)hipHostFree(ctx->fx_flag);
  delete ctx;
}

const char* cxk_last_error(const cxk_context* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int cxk_add_lmi(cxk_context* ctx, int n, int m, const double* A, const double* C, const int* vars) {
  if (!ctx || n < 1 || m < 0 || !A || !C) return -1;
  ConstraintRec r;
  r.type = CXK_LMI;
  r.n = n;
  r.m = m;
  r.A.assign(A, A + (size_t)m * n * n);
  r.C.assign(C, C + (size_t)n * n);
  auto symmetric = [n](const double* X) {
    for (int c = 0; c < n; c++)
      for (int q = c + 1; q < n; q++)
        if (X[q + (size_t)c * n] != X[c + (size_t)q * n]) return false;
    return true;
  };
  r.symmetric = symmetric(C);
  for (int i = 0; i < m && r.symmetric; i++) r.symmetric = symmetric(A + (size_t)i * n * n);
  return AddConstraint(ctx, std::move(r), vars);
}

namespace {
// jordan_matrix_algebra.cc:103-124 (4 x 4 corner): plane i ^ j of X Y receives sign[i][j] X_i Y_j.
// Real representation L(X): block (k, j) = sign[k ^ j][j] X_{k ^ j}; L(XY) = L(X) L(Y),
// L(X^*) = L(X)^T, tr L(X) = d Re tr X.
const int kHcSign[4][4] = {{1, 1, 1, 1}, {1, -1, -1, 1}, {1, 1, -1, -1}, {1, -1, 1, -1}};
void EmbedPlanes(int d, int n, const double* planes, double* out /* (d n)^2 col-major */) {
  const size_t nn = (size_t)n * n, N = (size_t)d * n;
  for (int k = 0; k < d; k++)
    for (int j = 0; j < d; j++) {
      const double* X = planes + (size_t)(k ^ j) * nn;
      const double sg = kHcSign[k ^ j][j];
      for (int c = 0; c < n; c++)
        for (int r = 0; r < n; r++) out[((size_t)j * n + c) * N + (size_t)k * n + r] = sg * X[(size_t)c * n + r];
    }
}
void ExtractPlanes(int d, int n, const double* emb, double* planes) {
  const size_t nn = (size_t)n * n, N = (size_t)d * n;
  for (int k = 0; k < d; k++)  // block (k, 0) = sign[k][0] X_k = X_k
    for (int c = 0; c < n; c++)
      for (int r = 0; r < n; r++) planes[(size_t)k * nn + (size_t)c * n + r] = emb[(size_t)c * N + (size_t)k * n + r];
}
}  // namespace

int cxk_add_hermitian(cxk_context* ctx, int n, int d, int m, const double* A, const double* C,
                      const int* vars) {
  if (!ctx || n < 1 || m < 0 || !A || !C) return -1;
  if (d == 8) {
    // Hermitian matrices over the octonions: no real representation (the algebra is not
    // associative): a cone type of its own, planes as they come (kernels_oct.hip.h)
    if (n > 3) {
      fprintf(stderr, "cxk_add_hermitian: order of octonion algebra cannot be greater than 3 (interfaces/conex.cc:310-311)\n");
      return -1;
    }
    ConstraintRec r;
    r.type = CXK_OCT;
    r.n = n;
    r.m = m;
    const size_t sz = (size_t)8 * n * n;
    r.A.assign(A, A + (size_t)m * sz);
    r.C.assign(C, C + sz);
    return AddConstraint(ctx, std::move(r), vars);
  }
  if (d != 1 && d != 2 && d != 4) {
    fprintf(stderr, "cxk_add_hermitian: hyper-complex dimension %d is not 1, 2, 4 or 8\n", d);
    return -1;
  }
  ConstraintRec r;
  r.type = CXK_LMI;
  r.herm_d = d;
  r.n = d * n;
  r.m = m;
  const size_t nn = (size_t)n * n, NN = (size_t)r.n * r.n;
  r.A.resize((size_t)m * NN);
  r.C.resize(NN);
  for (int i = 0; i < m; i++) EmbedPlanes(d, n, A + (size_t)i * d * nn, r.A.data() + (size_t)i * NN);
  EmbedPlanes(d, n, C, r.C.data());
  return AddConstraint(ctx, std::move(r), vars);
}

int cxk_add_linear(cxk_context* ctx, int rows, int m, const double* A, const double* c,
                   const int* vars) {
  if (!ctx || rows < 1 || m < 0 || !A || !c) return -1;
  ConstraintRec r;
  r.type = CXK_LINEAR;
  r.n = rows;
  r.m = m;
  r.A.assign(A, A + (size_t)rows * m);
  r.C.assign(c, c + rows);
  return AddConstraint(ctx, std::move(r), vars);
}

int cxk_add_soc(cxk_context* ctx, int n, int m, const double* A, const double* c, const int* vars) {
  if (!ctx || n < 1 || m < 0 || !A || !c) return -1;
  ConstraintRec r;
  r.type = CXK_SOC;
  r.n = n;
  r.m = m;
  r.A.assign(A, A + (size_t)(n + 1) * m);
  r.C.assign(c, c + n + 1);
  return AddConstraint(ctx, std::move(r), vars);
}

int cxk_add_quadratic(cxk_context* ctx, int n, int m, const double* Q, const double* A, const double* c, const int* vars) {
  if (!ctx || n < 1 || m < 0 || !A || !c) return -1;
  ConstraintRec r;
  r.type = CXK_QUAD;
  r.n = n;
  r.m = m;
  r.A.assign(A, A + (size_t)(n + 1) * m);
  r.C.assign(c, c + n + 1);
  if (Q) r.Q.assign(Q, Q + (size_t)n * n);
  return AddConstraint(ctx, std::move(r), vars);
}

int cxk_add_static(cxk_context* ctx, int m, const double* G, const int* vars) {
  if (!ctx || m < 1 || !G) return -1;
  ConstraintRec r;
  r.type = CXK_STATIC;
  r.n = 0;
  r.m = m;
  r.A.assign(G, G + (size_t)m * m);
  return AddConstraint(ctx, std::move(r), vars);
}

int cxk_add_equality(cxk_context* ctx, int rows, int m, const double* A, const double* b,
                     const int* vars) {
  if (!ctx || rows < 1 || m < 1 || !A || !b) return -1;
  const int mt = m + rows;
  ConstraintRec r;
  r.type = CXK_STATIC;  // constant Schur block [0 A^T; A 0], constant AQc = [0; b]
  r.n = 0;
  r.m = m;              // AddConstraint validates the user variables; multipliers appended below
  r.eq_rows = rows;
  r.A.assign((size_t)mt * mt, 0.0);
  r.C.assign((size_t)mt, 0.0);
  for (int j = 0; j < m; j++)
    for (int i = 0; i < rows; i++) {
      const double a = A[(size_t)j * rows + i];
      r.A[(size_t)j * mt + (m + i)] = a;
      r.A[(size_t)(m + i) * mt + j] = a;
    }
  for (int i = 0; i < rows; i++) r.C[m + i] = b[i];
  const int id = AddConstraint(ctx, std::move(r), vars);
  if (id < 0) return id;
  if (ctx->dual_start < 0) ctx->dual_start = ctx->num_vars;
  for (int i = 0; i < rows; i++) {  // constraint_manager.h:66-90
    ctx->cliques[id].push_back(ctx->dual_start + i);
    ctx->dual_vars[id].push_back(ctx->dual_start + i);
  }
  ctx->dual_start += rows;
  ctx->cons[id].m = mt;
  return id;
}

int cxk_factor_regularized(cxk_context* ctx, int* flag) {
  if (!ctx || !flag) return CXK_FAILURE;
  *flag = 0;
  if (!ctx->use_ldlt || !ctx->d_reg.p) return CXK_SUCCESS;
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(flag, ctx->d_reg.p, sizeof(int), hipMemcpyDeviceToHost));
  return CXK_SUCCESS;
}

int cxk_num_constraints(const cxk_context* ctx) { return ctx ? (int)ctx->cons.size() : 0; }

int cxk_set_shard(cxk_context* ctx, int rank, int world_size) {
  if (!ctx || ctx->finalized || world_size < 1 || rank < 0 || rank >= world_size) return CXK_FAILURE;
  ctx->rank = rank;
  ctx->world = world_size;
  return CXK_SUCCESS;
}

static int FinalizeImpl(cxk_context* ctx);

int cxk_comm_unique_id(void* out128) {
  if (!out128) return CXK_FAILURE;
  void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) {
    fprintf(stderr, "conex_kkt_hip: librccl.so not found (%s)\n", dlerror());
    return CXK_FAILURE;
  }
  auto get = reinterpret_cast<ncclResult_t (*)(ncclUniqueId*)>(dlsym(lib, "ncclGetUniqueId"));
  if (!get) return CXK_FAILURE;
  static_assert(sizeof(ncclUniqueId) == 128, "cxk_comm_unique_id hands out 128 bytes");
  return get(static_cast<ncclUniqueId*>(out128)) == ncclSuccess ? CXK_SUCCESS : CXK_FAILURE;
}

static int CommInitImpl(cxk_context* ctx, const void* unique_id128, int rank, int world_size, bool solo);
int cxk_comm_init_rccl(cxk_context* ctx, const void* unique_id128, int rank, int world_size) {
  return CommInitImpl(ctx, unique_id128, rank, world_size, false);
}
// Diagnostic: a ONE-rank communicator on a context sharded as rank r of a larger (virtual) world --
// its all-reduces are real ncclAllReduce calls that return their input, so the sharded step can be
// timed on a single GPU (bench.py --shard-path); the results are those of one shard only.
int cxk_comm_init_rccl_solo(cxk_context* ctx) {
  char id[128];
  if (cxk_comm_unique_id(id)) return CXK_FAILURE;
  return CommInitImpl(ctx, id, 0, 1, true);
}
static int CommInitImpl(cxk_context* ctx, const void* unique_id128, int rank, int world_size, bool solo) {
  if (!ctx || !unique_id128 || world_size < 1 || rank < 0 || rank >= world_size) return CXK_FAILURE;
  CXK_DEMAND(ctx->device >= 0, "a communicator needs a HIP device");
  if (!ctx->finalized && !solo) {
    ctx->rank = rank;
    ctx->world = world_size;
  }
  CXK_DEMAND(solo || (ctx->rank == rank && ctx->world == world_size), "communicator rank / size differ from cxk_set_shard");
  DeviceGuard guard(ctx->device);
  auto& R = ctx->rccl;
  if (!R.lib) {
    R.lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!R.lib) R.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    CXK_DEMAND(R.lib != nullptr, "librccl.so not found");
    R.CommInitRank = reinterpret_cast<decltype(R.CommInitRank)>(dlsym(R.lib, "ncclCommInitRank"));
    R.CommDestroy = reinterpret_cast<decltype(R.CommDestroy)>(dlsym(R.lib, "ncclCommDestroy"));
    R.CommCount = reinterpret_cast<decltype(R.CommCount)>(dlsym(R.lib, "ncclCommCount"));
    R.AllReduce = reinterpret_cast<decltype(R.AllReduce)>(dlsym(R.lib, "ncclAllReduce"));
    R.GetErrorString = reinterpret_cast<decltype(R.GetErrorString)>(dlsym(R.lib, "ncclGetErrorString"));
    CXK_DEMAND(R.CommInitRank && R.CommDestroy && R.AllReduce, "librccl.so lacks ncclCommInitRank / ncclAllReduce");
  }
  if (R.comm) {
    R.CommDestroy(R.comm);
    R.comm = nullptr;
  }
  ncclUniqueId id;
  memcpy(&id, unique_id128, sizeof(id));
  const ncclResult_t r = R.CommInitRank(&R.comm, world_size, id, rank);
  if (r != ncclSuccess) {
    ctx->err = std::string("ncclCommInitRank: ") + (R.GetErrorString ? R.GetErrorString(r) : "error");
    fprintf(stderr, "conex_kkt_hip: %s\n", ctx->err.c_str());
    R.comm = nullptr;
    return CXK_FAILURE;
  }
  return CXK_SUCCESS;
}

// Ranks of the attached RCCL communicator as RCCL itself counts them (ncclCommCount); 0 when the
// context has no RCCL communicator (single GPU, or a caller-supplied all-reduce).
int cxk_comm_count(const cxk_context* ctx) {
  if (!ctx || !ctx->rccl.comm || !ctx->rccl.CommCount) return 0;
  int n = 0;
  return ctx->rccl.CommCount(ctx->rccl.comm, &n) == ncclSuccess ? n : 0;
}

__global__ void comm_selftest_fill(int n, double* x) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) x[i] = 0.5 * i - 3.0;
}

// Runs sum, max and min all-reduces of `count` doubles through the attached RCCL communicator on
// the context's stream and checks the result against world_size copies of the same input (every
// rank fills the same values): the RCCL call path, exercised also by a one-rank communicator.
int cxk_comm_selftest(cxk_context* ctx, int count) {
  if (!ctx || count < 1) return CXK_FAILURE;
  CXK_DEMAND(ctx->rccl.comm != nullptr, "no RCCL communicator attached");
  DeviceGuard guard(ctx->device);
  DevBuf<double> buf;
  CXK_TRY(buf.alloc((size_t)count));
  std::vector<double> h((size_t)count);
  const int saved_world = ctx->world;
  for (int op = 0; op < 3; op++) {
    comm_selftest_fill<<<GridFor((size_t)count, 256), 256, 0, ctx->stream>>>(count, buf.p);
    CXK_TRY(hipGetLastError());
    ctx->world = 2;  // ShardAllReduce skips single-rank contexts; the communicator decides the real size
    const int rc = ShardAllReduce(ctx, buf.p, (size_t)count, op);
    ctx->world = saved_world;
    if (rc) return CXK_FAILURE;
    CXK_TRY(hipStreamSynchronize(ctx->stream));
    CXK_TRY(hipMemcpy(h.data(), buf.p, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    for (int i = 0; i < count; i++) {
      const double v = 0.5 * i - 3.0, want = op == kOpSum ? v * saved_world : v;
      CXK_DEMAND(h[i] == want, "RCCL all-reduce returned a wrong value");
    }
  }
  return CXK_SUCCESS;
}

int cxk_comm_set_allreduce(cxk_context* ctx, cxk_allreduce_fn fn, void* user) {
  if (!ctx) return CXK_FAILURE;
  ctx->coll_fn = fn;
  ctx->coll_user = user;
  return CXK_SUCCESS;
}

int cxk_set_chain_segments(cxk_context* ctx, int segments) {
  if (!ctx || ctx->finalized || segments < 0) return CXK_FAILURE;
  ctx->chain_segments = segments;
  return CXK_SUCCESS;
}
int cxk_chain_segments(const cxk_context* ctx) { return ctx && ctx->finalized ? ctx->segments : 0; }

int cxk_set_reference_identity(cxk_context* ctx, int on) {
  if (!ctx || ctx->finalized) return CXK_FAILURE;
  ctx->reference_identity = on != 0;
  return CXK_SUCCESS;
}

int cxk_finalize(cxk_context* ctx) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(!ctx->cons.empty(), "no constraints");
  CXK_DEMAND(!ctx->finalized, "context already finalized");
  DeviceGuard guard(ctx->device);
  const int rc = FinalizeImpl(ctx);
  if (rc != CXK_SUCCESS) {
    // a half-built context must not pass CheckReady, and the caller may change the shard or the
    // constraints and finalize again
    ctx->finalized = false;
    ctx->device_ready = false;
    ctx->groups.clear();
  }
  return rc;
}

static int FinalizeImpl(cxk_context* ctx) {
  if (ctx->reference_identity < 0) {
    // default: the reference as written; CXK_REFERENCE_QUIRKS=0 opts into the two corrections
    const char* quirks_env = getenv("CXK_REFERENCE_QUIRKS");
    ctx->reference_identity = !(quirks_env && atoi(quirks_env) == 0 && quirks_env[0] != '\0');
  }
  try {
    ctx->md = Analyze(ctx->cliques, ctx->dual_vars);
    ctx->lay = BuildLayout(ctx->md);
    // what the library REPORTS (cxk_get_order / _permutation / _list / _block_offsets ...) is always the
    // reference's structure; the factorization of a long chain-shaped tree runs in a segment-parallel
    // order of its own (symbolic.h, SegmentChain): CXK_CHAIN_SEGMENTS=0 keeps the reference's order,
    // =P asks for P segments, unset = automatic for chains of at least kAutoChainSteps steps
    ctx->md_ref = ctx->md;
    ctx->lay_ref = ctx->lay;
    ctx->segments = 0;
    constexpr int kAutoChainSteps = 256;
    int want = ctx->chain_segments;
    if (want < 0)
      if (const char* v = getenv("CXK_CHAIN_SEGMENTS")) want = atoi(v);
    if (want != 0 && ctx->md.K >= (want > 0 ? 4 : kAutoChainSteps) && IsChain(ctx->md)) {
      // depth of the segmented tree = K / P + log2(P) levels: the shortest pieces (two steps each) are
      // the fastest (measured on config 3: 128 / 500 / 1250 / 2500 pieces -> 2300 / 4680 / 6270 / 6600 solves/s)
      int P = want > 1 ? want : ctx->md.K / 2;
      P = std::min(P, ctx->md.K / 2);
      MatrixData seg;
      if (P >= 2 && SegmentChain(ctx->md, ctx->cliques, ctx->dual_vars, P, &seg)) {
        ctx->md = seg;
        ctx->lay = BuildLayout(ctx->md);
        ctx->segments = P;
      }
    }
  } catch (const std::exception& e) {
    return Fail(ctx, e.what());
  }
  const int K = (int)ctx->cons.size();
  ComputeTreeStructure(ctx);
  PartitionTree(ctx);  // world == 1: everything is owned
  ctx->g_off.assign(K, 0);
  ctx->r_off.assign(K, 0);
  int64_t go = 0, ro = 0;
  for (int i = 0; i < K; i++) {
    ctx->g_off[i] = go;
    ctx->r_off[i] = ro;
    go += (int64_t)ctx->cons[i].m * ctx->cons[i].m;
    ro += ctx->cons[i].m;
  }
  ctx->finalized = true;
  if (ctx->device < 0) return CXK_SUCCESS;  // symbolic-only context

  CXK_TRY(RaiseLdsLimits());
  CXK_TRY(hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  // groups of identically shaped constraints (owned ones only carry data)
  std::map<std::tuple<int, int, int, int>, int> gmap;
  ctx->groups.clear();
  for (int i = 0; i < K; i++) {
    ConstraintRec& c = ctx->cons[i];
    if (!ctx->owned[i]) continue;
    if (c.type == CXK_LMI) {
      // sparse evaluation when it pays (CXK_SPARSE_LMI=0 / 1 forces never / always: tests)
      double nnz = 0;
      for (double v : c.A) nnz += (v != 0.0);
      const char* force = getenv("CXK_SPARSE_LMI");
      const bool lds_resident = LmiTakeLds(c.n) <= kLdsLimit && LmiPrepareLds(c.n, c.m) <= kLdsLimit;
      c.sparse = force ? (atoi(force) != 0)
                       : LmiSparsePays(c.n, c.m, nnz, lds_resident, LmiMfmaSupports(c.n, c.m, c.herm_d));
      if (c.n > 65535) c.sparse = false;  // packed row | col << 16
      if (!c.symmetric) {
        // The reference accepts non-symmetric matrices and evaluates <W A_i W, A_j> as written;
        // only the literal LDS kernels do the same.
        c.sparse = false;
        CXK_DEMAND(lds_resident, "non-symmetric LMI data beyond the LDS-resident orders is not supported: "
                                 "the large-order kernels use tr(W A_i W A_j) = tr(P_i P_j), which needs A_i = A_i^T");
      }
    }
    if (c.type == CXK_SOC)
      // soc_schur keeps a cone's (n + 1) x (m + 2) image in LDS (CONEX_NewLorentzConeConstraint makes a
      // cone's matrix as wide as its largest variable index: thousands of columns are possible there)
      CXK_DEMAND(sizeof(double) * (size_t)(c.n + 1) * (size_t)(c.m + 2) <= kLdsLimit,
                 "a second-order cone whose (dimension + 1) x (variables + 2) image exceeds LDS (160 KB) is not supported");
    auto key = std::make_tuple(c.type, c.n, c.m, c.herm_d + (c.sparse ? 16 : 0) + (c.type == CXK_LMI && !c.symmetric ? 32 : 0) +
                                                     (c.type == CXK_QUAD && !c.Q.empty() ? 64 : 0));
    auto it = gmap.find(key);
    if (it == gmap.end()) {
      it = gmap.emplace(key, (int)ctx->groups.size()).first;
      ctx->groups.emplace_back();
      ctx->groups.back().type = c.type;
      ctx->groups.back().n = c.n;
      ctx->groups.back().m = c.m;
      ctx->groups.back().herm_d = c.herm_d;
      ctx->groups.back().sparse = c.sparse;
      ctx->groups.back().literal = c.type == CXK_LMI && !c.symmetric;
      ctx->groups.back().has_q = c.type == CXK_QUAD && !c.Q.empty();
    }
    c.group = it->second;
    c.member = (int)ctx->groups[it->second].ids.size();
    ctx->groups[it->second].ids.push_back(i);
  }
  for (Group& g : ctx->groups) {
    const size_t cnt = g.ids.size();
    size_t a_sz = 0, c_sz = 0, w_sz = 0;
    switch (g.type) {
      case CXK_LMI:
        a_sz = (size_t)g.m * g.n * g.n;
        c_sz = w_sz = (size_t)g.n * g.n;
        g.large = !(LmiTakeLds(g.n) <= kLdsLimit && LmiPrepareLds(g.n, g.m) <= kLdsLimit);
        {
          const int gemm_min_n = getenv("CXK_GEMM_MIN_N") ? atoi(getenv("CXK_GEMM_MIN_N")) : 9;
          // shapes past the register kernels' instances assemble through the batched GEMM (measured
          // 1.5 - 3.3x faster than lmi_schur_generic at 1000 constraints: orders 25 up, and smaller
          // orders with more variables than lmi_schur_mfma's LDS images hold, e.g. order 22, m = 20
          // 285 -> 133 us, order 10, m = 60 496 -> 148 us; CXK_GEMM_MIN_N moves the threshold for
          // comparison runs)
          // CXK_LMI_SCHUR=generic selects the LDS-resident literal kernel (comparison runs, tests)
          const char* pick = getenv("CXK_LMI_SCHUR");
          const bool want_generic = pick && !strcmp(pick, "generic");
          g.mfma = !g.sparse && !g.large && !g.literal && !want_generic && LmiMfmaSupports(g.n, g.m, g.herm_d);
          g.schur_gemm = !g.sparse && !g.literal && (g.large || (!g.mfma && g.n >= gemm_min_n &&
                                     cnt * 2 * ((size_t)g.m + 1) * g.n * g.n * sizeof(double) <= ((size_t)8 << 30)));
        }
        break;
      case CXK_LINEAR:
        a_sz = (size_t)g.n * g.m;
        c_sz = w_sz = (size_t)g.n;
        break;
      case CXK_SOC:
        a_sz = (size_t)(g.n + 1) * g.m;
        c_sz = w_sz = (size_t)(g.n + 1);
        break;
      case CXK_STATIC:
        a_sz = (size_t)g.m * g.m;
        c_sz = (size_t)g.m;  // constant AQc (zeros for a quadratic-cost block)
        break;
      case CXK_QUAD:
        a_sz = (size_t)(g.n + 1) * g.m;
        c_sz = w_sz = (size_t)(g.n + 1);
        break;
      case CXK_OCT:
        a_sz = (size_t)g.m * 8 * g.n * g.n;
        c_sz = w_sz = (size_t)8 * g.n * g.n;
        break;
    }
    if (g.type == CXK_LMI && g.sparse) {
      if (UploadSparseLmi(ctx, g)) return CXK_FAILURE;
      a_sz = 0;  // no dense copy of A on the device
    }
    // lmi_schur_mfma reads [A_1 .. A_m | C] of a constraint as one contiguous array of stacked
    // rows: such groups keep a copy of C right behind the A_i (LmiGroup::a_stride)
    const size_t a_blk = a_sz + (g.type == CXK_LMI && (g.mfma || g.schur_gemm) ? c_sz : 0);
    std::vector<double> hA(a_blk * cnt), hC(c_sz * cnt);
    for (size_t k = 0; k < cnt; k++) {
      const ConstraintRec& c = ctx->cons[g.ids[k]];
      if (a_sz) std::copy(c.A.begin(), c.A.end(), hA.begin() + k * a_blk);
      if (a_blk > a_sz) std::copy(c.C.begin(), c.C.end(), hA.begin() + k * a_blk + a_sz);
      std::copy(c.C.begin(), c.C.end(), hC.begin() + k * c_sz);
    }
    CXK_TRY(g.A.upload(hA));
    CXK_TRY(g.C.upload(hC));
    if (g.type == CXK_LMI && g.mfma && LmiMfmaPaddedOrder(g.n) != g.n && !(g.herm_d == 2 && g.n == 24)) {
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
    if (g.type == CXK_LMI && g.herm_d > 1 && g.schur_gemm && !g.literal && !getenv("CXK_NO_HERM_FOLD")) {
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
    if (g.type == CXK_LMI && !g.literal && !getenv("CXK_NO_PACKED_SLACK") && g.n == 20 &&
        LmiPrepareRowsSupports(g.n, g.m, g.herm_d, g.sparse)) {
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
    if (g.type == CXK_QUAD) {
      // A_gram = A1' (Q A1), made once (QuadraticConstraintBase::Initialize, quadratic_cone_constraint.cc:216-219)
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
      CXK_TRY(g.qS.alloc(w_sz * cnt));
    }
    CXK_TRY(g.W.alloc(w_sz * cnt));
    CXK_TRY(g.T1.alloc(w_sz * cnt));
    CXK_TRY(g.T2.alloc(g.type == CXK_LINEAR ? w_sz * cnt : 0));
    CXK_TRY(g.dids.upload(g.ids));
    if (g.type == CXK_LMI && g.sparse && (g.large || !g.sp_small)) {
      const size_t nn = (size_t)g.n * g.n;
      CXK_TRY(g.ws_main.alloc(cnt * 8 * nn));  // step temporaries; C W and W C W during assembly
      CXK_TRY(g.ws_part.alloc(cnt * 2 * kSparseCParts));
      CXK_TRY(g.ws_piv.alloc(cnt * (size_t)g.n));
    }
    if (g.schur_gemm) {
      const size_t nn = (size_t)g.n * g.n, m1 = (size_t)g.m + 1;
      // split-K of the contraction: enough workgroups to fill the chip, at most one K step each
      const int ksteps = (int)((nn + kGemmBK - 1) / kGemmBK);
      const int tiles = (int)(((m1 + 63) / 64) * ((m1 + 63) / 64));
      // (measured on BASELINE config 2, one constraint, K = 40 000: 39 / 78 / 156 / 312 / 512 / 768 / 1024
      // splits -> 115 / 93 / 82 / 81 / 76 / 80 / 82 us per KKT solve)
      g.splits = std::max(1, std::min(std::max(1, ksteps / 4), (int)((512 + cnt * tiles - 1) / (cnt * tiles))));
      if (getenv("CXK_GRAM_SPLITS")) g.splits = std::max(1, atoi(getenv("CXK_GRAM_SPLITS")));  // (comparison runs)
      CXK_TRY(g.ws_main.alloc(cnt * std::max(2 * m1 * nn, 8 * nn)));
      CXK_TRY(g.ws_gf.alloc(cnt * m1 * m1));
      CXK_TRY(g.ws_piv.alloc(cnt * (size_t)g.n));
      CXK_TRY(g.ws_part.alloc(g.splits > 1 ? (size_t)g.splits * cnt * m1 * m1 : 0));
    }
  }
  CXK_TRY(ctx->G.alloc((size_t)go));
  CXK_TRY(ctx->AWc.alloc((size_t)ro));
  CXK_TRY(ctx->AQcc.alloc((size_t)ro));
  CXK_TRY(ctx->sc.alloc((size_t)2 * K, true));  // entries of constraints owned by other ranks stay 0 (summed by the gather)
  CXK_TRY(ctx->d_g_off.upload(ctx->g_off));
  CXK_TRY(ctx->d_r_off.upload(ctx->r_off));
  CXK_TRY(ctx->slab.alloc((size_t)ctx->lay.slab_size));
  const int N = ctx->md.N;
  CXK_TRY(ctx->y.alloc(N));
  CXK_TRY(ctx->b.alloc(N));
  CXK_TRY(ctx->AW.alloc(N));
  CXK_TRY(ctx->AQc.alloc(N));
  CXK_TRY(ctx->sys_sc.alloc(2));
  CXK_TRY(ctx->red_out.alloc(4));
  CXK_TRY(ctx->scal_out.alloc(8));
  // [flag, tag of a failed fused pivot or time-out, tag of a time-out some rank reported (ShardMark)]
  CXK_TRY(ctx->d_fail.alloc(3, true));
  ctx->use_ldlt = false;
  for (const IntList& dv : ctx->dual_vars)
    if (!dv.empty()) ctx->use_ldlt = true;  // kkt_solver.cc:180-186
  if (ctx->use_ldlt) {
    CXK_TRY(ctx->d_tr.alloc(N));
    CXK_TRY(ctx->d_reg.alloc(1, true));
  }
  {
    // per-constraint step outputs; constraints without a cone (constant blocks) keep the
    // reference's defaults: StepInfo {0,0}; WeightedSlackEigenvalues {min=DBL_MAX,max=-DBL_MAX,0,0}
    std::vector<double> info((size_t)4 * K, 0.0);
    for (int i = 0; i < K; i++)
      if (ctx->cons[i].type == CXK_STATIC) {
        info[4 * i] = DBL_MAX;
        info[4 * i + 1] = -DBL_MAX;
      }
    CXK_TRY(ctx->info4.upload(info));
    CXK_TRY(ctx->info2.alloc((size_t)2 * K, true));  // cone-less constraints keep StepInfo {0, 0}
    CXK_TRY(ctx->d_mask.upload(ctx->owned));
  }
  if (BuildPlans(ctx) != CXK_SUCCESS) return CXK_FAILURE;
  ctx->device_ready = true;
  return cxk_set_identity(ctx);
}

// ------------------------------------------------------------- symbolic getters
int cxk_system_size(const cxk_context* ctx) { return ctx && ctx->finalized ? ctx->md.N : 0; }
int cxk_get_order(const cxk_context* ctx, int* order) {
  if (!ctx || !ctx->finalized) return 0;
  std::copy(ctx->md_ref.clique_order.begin(), ctx->md_ref.clique_order.end(), order);
  return ctx->md_ref.K;
}
int cxk_get_permutation(const cxk_context* ctx, int* perm, int* perm_inv) {
  if (!ctx || !ctx->finalized) return 0;
  std::copy(ctx->md_ref.permutation.begin(), ctx->md_ref.permutation.end(), perm);
  std::copy(ctx->md_ref.permutation_inverse.begin(), ctx->md_ref.permutation_inverse.end(), perm_inv);
  return ctx->md_ref.num_vars;
}
int cxk_get_list(const cxk_context* ctx, int which, int e, int* out) {
  if (!ctx || !ctx->finalized || e < 0 || e >= ctx->md_ref.K) return -1;
  const IntList* v = nullptr;
  switch (which) {
    case 0: v = &ctx->md_ref.cliques[e]; break;
    case 1: v = &ctx->md_ref.supernodes_orig[e]; break;
    case 2: v = &ctx->md_ref.separators_orig[e]; break;
    case 3: v = &ctx->md_ref.supernodes_pos[e]; break;
    case 4: v = &ctx->md_ref.separators_pos[e]; break;
    // (10 ..: the structure the factorization runs on -- the same unless cxk_chain_segments(ctx) != 0;
    // 20 / 21 ignore e: its supernode sizes / its permutation, original variable -> eliminated position)
    case 10: v = &ctx->md.cliques[e]; break;
    case 11: v = &ctx->md.supernodes_orig[e]; break;
    case 12: v = &ctx->md.separators_orig[e]; break;
    case 13: v = &ctx->md.supernodes_pos[e]; break;
    case 14: v = &ctx->md.separators_pos[e]; break;
    case 20: v = &ctx->md.supernode_size; break;
    case 21: v = &ctx->md.permutation; break;
    default: return -1;
  }
  if (out) std::copy(v->begin(), v->end(), out);
  return (int)v->size();
}
int cxk_get_supernode_sizes(const cxk_context* ctx, int* out) {
  if (!ctx || !ctx->finalized) return 0;
  std::copy(ctx->md_ref.supernode_size.begin(), ctx->md_ref.supernode_size.end(), out);
  return ctx->md_ref.K;
}
long cxk_slab_size(const cxk_context* ctx) { return ctx && ctx->finalized ? (long)ctx->lay.slab_size : 0; }
int cxk_get_block_offsets(const cxk_context* ctx, long* diag_off, long* offd_off) {
  if (!ctx || !ctx->finalized) return 0;
  for (int e = 0; e < ctx->md_ref.K; e++) {
    diag_off[e] = (long)ctx->lay_ref.diag_off[e];
    offd_off[e] = (long)ctx->lay_ref.offd_off[e];
  }
  return ctx->md_ref.K;
}
int cxk_get_ss_index(const cxk_context* ctx, int e, long* out) {
  if (!ctx || !ctx->finalized || e < 0 || e >= ctx->md_ref.K) return -1;
  const auto& v = ctx->lay_ref.ss_index[e];
  if (out)
    for (size_t i = 0; i < v.size(); i++) out[i] = (long)v[i];
  return (int)v.size();
}
int cxk_num_levels(const cxk_context* ctx) { return ctx ? (int)ctx->level_ptr.size() - 1 : 0; }

// ------------------------------------------------------------- scaling point
int cxk_dual_size(const cxk_context* ctx, int i) {
  if (!ctx || i < 0 || i >= (int)ctx->cons.size()) return 0;
  const ConstraintRec& c = ctx->cons[i];
  switch (c.type) {
    case CXK_LMI: return c.herm_d ? (c.n / c.herm_d) * (c.n / c.herm_d) * c.herm_d : c.n * c.n;
    case CXK_LINEAR: return c.n;
    case CXK_SOC: return c.n + 1;
    case CXK_QUAD: return c.n + 1;
    case CXK_OCT: return 8 * c.n * c.n;
    case CXK_STATIC: return c.eq_rows;  // lambda_ of an equality block; 0 for a quadratic cost
    default: return 0;
  }
}

int cxk_set_identity(cxk_context* ctx) {
  CXK_ENTER(ctx);
  if (DropTriple(ctx)) return CXK_FAILURE;
  for (Group& g : ctx->groups) {
    const size_t cnt = g.ids.size();
    if (cnt == 0) continue;
    if (g.type == CXK_LMI)
      lmi_set_identity<<<GridFor(cnt * g.n * g.n, 256), 256, 0, ctx->stream>>>(MakeLmi(g));
    else if (g.type == CXK_LINEAR || g.type == CXK_SOC || g.type == CXK_QUAD)
      vec_set_identity<<<GridFor(cnt * (g.n + 1), 256), 256, 0, ctx->stream>>>(MakeVec(g),
                                                                               g.type != CXK_LINEAR);
    else if (g.type == CXK_OCT)
      oct_set_identity<<<GridFor(cnt * 8 * g.n * g.n, 256), 256, 0, ctx->stream>>>(MakeOct(g));
  }
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

int cxk_get_W(cxk_context* ctx, int i, double* out) {
  CXK_ENTER(ctx);
  CXK_DEMAND(i >= 0 && i < (int)ctx->cons.size() && ctx->cons[i].group >= 0, "invalid constraint");
  const ConstraintRec& c = ctx->cons[i];
  const size_t sz = (size_t)cxk_dual_size(ctx, i);
  if (sz == 0) return CXK_SUCCESS;
  if (c.type == CXK_STATIC) {  // multipliers latched by the last PrepareStep (equality_constraint.cc:32-37)
    CXK_DEMAND(!ctx->y_at_prepare.empty(), "no PrepareStep has run yet");
    const IntList& cl = ctx->cliques[i];
    for (int q = 0; q < c.eq_rows; q++)
      out[q] = ctx->y_at_prepare[ctx->md.permutation[cl[cl.size() - c.eq_rows + q]]];
    return CXK_SUCCESS;
  }
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  if (c.herm_d) {  // device holds the real representation; the interface speaks planes
    const size_t NN = (size_t)c.n * c.n;
    std::vector<double> emb(NN);
    CXK_TRY(hipMemcpy(emb.data(), ctx->groups[c.group].W.p + NN * c.member, NN * sizeof(double),
                      hipMemcpyDeviceToHost));
    ExtractPlanes(c.herm_d, c.n / c.herm_d, emb.data(), out);
    return CXK_SUCCESS;
  }
  CXK_TRY(hipMemcpy(out, ctx->groups[c.group].W.p + sz * c.member, sz * sizeof(double),
                    hipMemcpyDeviceToHost));
  return CXK_SUCCESS;
}

int cxk_set_W(cxk_context* ctx, int i, const double* in) {
  CXK_ENTER(ctx);
  if (DropTriple(ctx)) return CXK_FAILURE;
  CXK_DEMAND(i >= 0 && i < (int)ctx->cons.size() && ctx->cons[i].group >= 0, "invalid constraint");
  const ConstraintRec& c = ctx->cons[i];
  const size_t sz = (size_t)cxk_dual_size(ctx, i);
  if (sz == 0 || c.type == CXK_STATIC) return CXK_SUCCESS;  // multipliers are outputs only
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  if (c.herm_d) {
    const size_t NN = (size_t)c.n * c.n;
    std::vector<double> emb(NN);
    EmbedPlanes(c.herm_d, c.n / c.herm_d, in, emb.data());
    CXK_TRY(hipMemcpy(ctx->groups[c.group].W.p + NN * c.member, emb.data(), NN * sizeof(double),
                      hipMemcpyHostToDevice));
    return CXK_SUCCESS;
  }
  CXK_TRY(hipMemcpy(ctx->groups[c.group].W.p + sz * c.member, in, sz * sizeof(double),
                    hipMemcpyHostToDevice));
  return CXK_SUCCESS;
}

// ------------------------------------------------------------- Newton step
int cxk_assemble_local(cxk_context* ctx) {
  CXK_ENTER_KEEP(ctx);
  if (FlushDirection(ctx)) return CXK_FAILURE;  // (a direction nobody has read yet: before its three parts are overwritten)
  ctx->asm_deferred = false;  // a gather still pending would describe the previous Schur blocks
  ctx->y3_valid = false;      // (so would three solutions nobody has combined: a redone iteration)
  if (LaunchSchur(ctx)) return CXK_FAILURE;
  if (FusedAssembly(ctx)) {
    ctx->asm_deferred = true;  // rides in the factorization that follows (or FlushDeferred)
    return CXK_SUCCESS;
  }
  return LaunchGather(ctx, false, 0, 0, 0);
}

int cxk_finish_assemble(cxk_context* ctx) { return CheckReady(ctx); }  // (a deferred gather stays deferred)

int cxk_assemble(cxk_context* ctx) {
  if (cxk_assemble_local(ctx)) return CXK_FAILURE;
  return cxk_finish_assemble(ctx);
}

__global__ void copy_doubles(int n, const double* __restrict__ src, double* __restrict__ dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

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

// TakeStep of every cone; step_from != nullptr: step length from the device (StepArgs::step_from).
extern "C" {
static int LaunchTakeStep(cxk_context* ctx, double e_weight, double step_size, const double* step_from,
                          bool skip_on_fail = false);
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

int cxk_factor_async(cxk_context* ctx) {
  CXK_ENTER(ctx);
  if (DropTriple(ctx)) return CXK_FAILURE;
  // the gather that assembled the system has cleared the failure flag (GatherBody); a factorization
  // of a slab that came another way (cxk_set_slab, a second factorization) clears it here
  if (!ctx->fail_clean) CXK_TRY(hipMemsetAsync(ctx->d_fail.p, 0, sizeof(int), ctx->stream));
  ctx->fail_tag = 0;
  if (LaunchTree(ctx, 0, false, false)) return CXK_FAILURE;
  ctx->factor_seq = ++ctx->seq;
  return CXK_SUCCESS;
}

int cxk_factor_status(cxk_context* ctx, int* ok) {
  CXK_ENTER(ctx);
  if (ctx->mb_seen < ctx->factor_seq && SyncMailbox(ctx)) return CXK_FAILURE;
  if (ResolveShardTimeout(ctx)) return CXK_FAILURE;  // (sharded: settled the same way on every rank)
  if (ok) *ok = (ctx->mb ? (ctx->mbv[10] == 0.0) : 1) && !FusedTimedOut(ctx);
  if (FusedTimedOut(ctx) && ctx->world <= 1) {
    // not a property of the matrix: the caller learns it through cxk_fused_tree_timed_out and redoes
    // its iteration, which then runs on the level kernels
    if (DisableFusedTree(ctx)) return CXK_FAILURE;
    ctx->timeout_unreported = true;
  }
  return CXK_SUCCESS;
}

}  // extern "C"
namespace {
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
         LmiPrepareRowsSupports(only->n, only->m, only->herm_d, only->sparse);
}
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
}  // namespace
extern "C" {

int cxk_step_scalars_async(cxk_context* ctx) {
  CXK_ENTER_KEEP(ctx);
  if (FlushDeferred(ctx, false, StepTailOk(ctx, 0))) return CXK_FAILURE;
  if (StepTailOk(ctx, 0)) {
    ctx->scal_deferred = true;  // normally picked up by the PrepareStep that follows
    return CXK_SUCCESS;
  }
  return LaunchStepScalars(ctx);
}

// Factor and solve in one sweep (the forward substitution rides in the elimination as in
// cxk_kkt_solve_async): y <- K^-1 (cb b + cq AQc + cw AW).  With (k bs, k cs, -2) this is the Newton
// direction, with (-bs, cs, 0) the right-hand side of ComputeMuFromDivergence (cone_program.cc:173-214).
int cxk_factor_solve_async(cxk_context* ctx, double cb, double cq, double cw) {
  CXK_ENTER_KEEP(ctx);
  if (DropTriple(ctx)) return CXK_FAILURE;
  const int N = ctx->md.N;
  if (ctx->asm_deferred && FusedAssembly(ctx)) {  // gather and right-hand side ride in the first factor level
    ctx->asm_deferred = false;
    ctx->asm_pending.on = true;
    ctx->asm_pending.with_rhs = 2;
    ctx->asm_pending.cb = cb;
    ctx->asm_pending.cq = cq;
    ctx->asm_pending.cw = cw;
  } else {
    if (FlushDeferred(ctx)) return CXK_FAILURE;
    build_rhs_comb<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, cb, cq, cw, ctx->b.p, ctx->AQc.p, ctx->AW.p,
                                                             ctx->y.p, ctx->d_fail.p);
    CXK_TRY(hipGetLastError());
    ctx->fail_tag = 0;
  }
  ctx->rhs_c[0] = cb;
  ctx->rhs_c[1] = cq;
  ctx->rhs_c[2] = cw;
  if (LaunchTree(ctx, 0, true, true)) return CXK_FAILURE;
  CXK_DEMAND(!ctx->asm_pending.on, "internal error: the folded assembly was not launched");
  ctx->factor_seq = ++ctx->seq;
  ctx->redo_call = ctx->calls;
  return CXK_SUCCESS;
}

// The factorization with THREE right-hand sides in its one launch (tree_fused.h kFusedTriple): y <- K^-1 (-bs b +
// cs AQc), the solve of the mu selection (cone_program.cc:181), and the three solutions K^-1 (bs b), K^-1 (cs AQc),
// K^-1 AW from which the Newton direction for the mu the device selects is a linear combination -- formed on
// the fly by the PrepareStep that follows (StepArgs::y3): cxk_newton_direction_device_mu then launches nothing,
// the interior-point iteration is five launches instead of six.
// y = k (K^-1 (bs b) + K^-1 (cs AQc)) - 2 K^-1 AW, k = the barrier parameter the device selected

static bool DeviceMuOk(const cxk_context* ctx);
static bool TripleOk(const cxk_context* ctx) {
  return !ctx->no_triple && ctx->fused_tree && !ctx->fused_split && !ctx->fused_shard && ctx->world <= 1 && ctx->refine_iters <= 0 &&
         ctx->solver_mode != 2 && !ctx->use_ldlt && ctx->y3.n == 3 * (size_t)ctx->md.N && StepTailOk(ctx, 0) && DeviceMuOk(ctx) &&
         (ctx->fused_sa >> 8) <= 32 && (ctx->fused_sb >> 8) <= 32 &&
         // (as things stand: the assembly just enqueued is still waiting to ride in the factorization -- not
         // after a call that flushed it, e.g. the step scalars of the first iteration's rescaling)
         ctx->asm_deferred && FusedAssembly(ctx);
}
int cxk_triple_supported(cxk_context* ctx) {
  if (!ctx || CheckReady(ctx)) return 0;
  return TripleOk(ctx) ? 1 : 0;
}
int cxk_factor_solve_triple_async(cxk_context* ctx, double bs, double cs) {
  CXK_ENTER_KEEP(ctx);
  CXK_DEMAND(TripleOk(ctx), "cxk_factor_solve_triple_async: not supported by this program, or not directly behind cxk_assemble (cxk_triple_supported)");
  ctx->asm_deferred = false;
  ctx->asm_pending.on = true;
  ctx->asm_pending.with_rhs = 3;
  ctx->asm_pending.bs = bs;
  ctx->asm_pending.cs = cs;
  ctx->rhs_c[0] = -bs;
  ctx->rhs_c[1] = cs;
  ctx->rhs_c[2] = 0.0;
  if (LaunchTree(ctx, 0, true, true)) return CXK_FAILURE;
  CXK_DEMAND(!ctx->asm_pending.on, "internal error: the folded assembly was not launched");
  ctx->factor_seq = ++ctx->seq;
  ctx->redo_call = ctx->calls;
  ctx->y3_valid = true;
  ctx->y3_bs = bs;
  ctx->y3_cs = cs;
  return CXK_SUCCESS;
}

// cxk_factor_async + cxk_newton_direction in one upward pass: y <- K^-1 (k (b bs + AQc cs) - 2 AW).
int cxk_factor_direction_async(cxk_context* ctx, double k, double bs, double cs) {
  CXK_ENTER_KEEP(ctx);
  if (DropTriple(ctx)) return CXK_FAILURE;
  const int N = ctx->md.N;
  if (ctx->asm_deferred && FusedAssembly(ctx)) {
    ctx->asm_deferred = false;
    ctx->asm_pending.on = true;
    ctx->asm_pending.with_rhs = 1;
    ctx->asm_pending.k = k;
    ctx->asm_pending.bs = bs;
    ctx->asm_pending.cs = cs;
  } else {
    if (FlushDeferred(ctx)) return CXK_FAILURE;
    build_rhs<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, k, bs, cs, ctx->b.p, ctx->AQc.p, ctx->AW.p, ctx->y.p,
                                                        ctx->d_fail.p);
    CXK_TRY(hipGetLastError());
    ctx->fail_tag = 0;
  }
  ctx->rhs_c[0] = k * bs;
  ctx->rhs_c[1] = k * cs;
  ctx->rhs_c[2] = -2.0;
  if (LaunchTree(ctx, 0, true, true)) return CXK_FAILURE;
  CXK_DEMAND(!ctx->asm_pending.on, "internal error: the folded assembly was not launched");
  ctx->factor_seq = ++ctx->seq;
  ctx->redo_call = ctx->calls;
  return CXK_SUCCESS;
}

int cxk_factor(cxk_context* ctx, int* ok) {
  if (cxk_factor_async(ctx)) return CXK_FAILURE;
  return cxk_sync(ctx, ok);
}

int cxk_sync(cxk_context* ctx, int* factor_ok) {
  CXK_ENTER(ctx);
  if (SyncMailbox(ctx)) return CXK_FAILURE;
  CXK_TRY(hipStreamSynchronize(ctx->stream));  // the stream is idle: cheap, and later host-side copies rely on it
  if (ResolveShardTimeout(ctx)) return CXK_FAILURE;  // (sharded: settled the same way on every rank)
  bool timed_out = false;
  if (ctx->world > 1) {
    // (nothing left to settle: ResolveShardTimeout has, and a time-out every rank saw fails the mailbox)
  } else if (FusedTimedOut(ctx) && ctx->redo_call == ctx->calls - 1) {
    // the factor-and-solve was the last call before this one: redo it level by level instead of reporting a failure
    if (RedoFactorSolveOnLevels(ctx) || SyncMailbox(ctx)) return CXK_FAILURE;
    CXK_TRY(hipStreamSynchronize(ctx->stream));
  } else if (FusedTimedOut(ctx)) {
    // other work went out behind it (a solve-only sweep, the mu selection, a direction, PrepareStep), or the
    // inputs changed: the redo would not rebuild what it computed -- reported as cxk_factor_status does
    if (DisableFusedTree(ctx)) return CXK_FAILURE;
    ctx->timeout_unreported = true;
    timed_out = true;
  }
  if (factor_ok) *factor_ok = ctx->mbv[10] == 0.0 && !timed_out;
  // fold finished timing samples
  for (size_t k = 0; k < ctx->ev_used; k++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev_pool[k].first, ctx->ev_pool[k].second) == hipSuccess) {
      ctx->time_acc_ms[ctx->ev_slot[k]] += ms;
      ctx->time_samples[ctx->ev_slot[k]]++;
    }
  }
  ctx->ev_used = 0;
  return CXK_SUCCESS;
}

int cxk_set_cost(cxk_context* ctx, const double* b) {
  CXK_ENTER(ctx);
  if (DropTriple(ctx)) return CXK_FAILURE;
  const int N = ctx->md.N;
  std::vector<double> bp(N, 0.0);
  for (int i = 0; i < N; i++) {
    const int v = ctx->md.permutation_inverse[i];
    bp[i] = v < ctx->num_vars ? b[v] : 0.0;  // multipliers carry zero cost
  }
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(ctx->b.p, bp.data(), sizeof(double) * N, hipMemcpyHostToDevice));
  return CXK_SUCCESS;
}

// Solve-only sweep of y <- K^-1 rhs with rhs in one of the two forms of RhsIn: formed inside the
// forward kernels when all of them are lean ones, by a launch of its own otherwise.
static int SolveWithRhs(cxk_context* ctx, const RhsIn& form) {
  const int N = ctx->md.N;
  const bool inline_rhs = (ctx->forward_all_lean || ctx->fused_tree) && ctx->world == 1 && ctx->solver_mode != 2 &&
                          ctx->refine_iters <= 0 && !ctx->no_lean;
  if (inline_rhs) {
    ctx->rhs_in = form;
  } else if (form.form == 1) {
    build_rhs<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, form.k, form.bs, form.cs, ctx->b.p, ctx->AQc.p, ctx->AW.p,
                                                        ctx->y.p, nullptr, form.k_from);
  } else {
    build_rhs_comb<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, form.cb, form.cq, form.cw, ctx->b.p, ctx->AQc.p,
                                                             ctx->AW.p, ctx->y.p);
  }
  const int rc = LaunchTree(ctx, 1, true, true);
  ctx->rhs_in = RhsIn{};
  return rc;
}

int cxk_newton_direction(cxk_context* ctx, double k, double bs, double cs) {
  CXK_ENTER(ctx);
  RhsIn f{};
  f.form = 1;
  f.b = ctx->b.p;
  f.AQc = ctx->AQc.p;
  f.AW = ctx->AW.p;
  f.k = k;
  f.bs = bs;
  f.cs = cs;
  return SolveWithRhs(ctx, f);
}

int cxk_solve_rhs(cxk_context* ctx, double cb, double cq, double cw) {
  CXK_ENTER(ctx);
  RhsIn f{};
  f.form = 2;
  f.b = ctx->b.p;
  f.AQc = ctx->AQc.p;
  f.AW = ctx->AW.p;
  f.cb = cb;
  f.cq = cq;
  f.cw = cw;
  return SolveWithRhs(ctx, f);
}

// ComputeMuFromLineSearch cone_program.cc:118-160.  *result = the admissible inv_sqrt_mu, or -1
// when a cone does not support the line search (everything but linear, quadratic-cost and
// equality blocks: constraint.h:24-28) or the interval is empty.  Overwrites y (as the reference
// overwrites its iterate vector).
int cxk_line_search(cxk_context* ctx, double dinf_upper_bound, double b_scaling, double c_scaling,
                    double* result) {
  CXK_ENTER(ctx);
  CXK_DEMAND(result != nullptr, "null output");
  const int N = ctx->md.N, K = (int)ctx->cons.size();
  if (ctx->y2.n != (size_t)N) CXK_TRY(ctx->y2.alloc(N));
  build_rhs_comb<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, 0.0, 0.0, -2.0, ctx->b.p, ctx->AQc.p,
                                                           ctx->AW.p, ctx->y.p);
  if (LaunchTree(ctx, 1, true, true)) return CXK_FAILURE;
  CXK_TRY(hipMemcpyAsync(ctx->y2.p, ctx->y.p, sizeof(double) * N, hipMemcpyDeviceToDevice, ctx->stream));
  build_rhs_comb<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, b_scaling, c_scaling, -2.0, ctx->b.p,
                                                           ctx->AQc.p, ctx->AW.p, ctx->y.p);
  if (LaunchTree(ctx, 1, true, true)) return CXK_FAILURE;
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
    if (cnt == 0 || g.type != CXK_LINEAR) continue;
    linear_line_search<<<cnt, 256, sizeof(double) * 2 * g.m, ctx->stream>>>(MakeVec(g), a);
  }
  CXK_TRY(hipGetLastError());
  std::vector<double> out((size_t)2 * K);
  const double* pairs = ctx->info2.p;
  if (ctx->world > 1) {  // every rank evaluated its own linear constraints: gather the bounds
    if (SettleBeforeUnmarked(ctx)) return CXK_FAILURE;
    CXK_DEMAND((size_t)2 * K <= ctx->shard_tmp.n, "internal error: shard scratch too small");
    masked_copy_pairs<<<GridFor((size_t)2 * K, 256), 256, 0, ctx->stream>>>(K, ctx->d_mask.p, ctx->info2.p, ctx->shard_tmp.p);
    CXK_TRY(hipGetLastError());
    if (ShardAllReduce(ctx, ctx->shard_tmp.p, (size_t)2 * K, kOpSum)) return CXK_FAILURE;
    pairs = ctx->shard_tmp.p;
  }
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(out.data(), pairs, sizeof(double) * 2 * K, hipMemcpyDeviceToHost));
  double lb = -DBL_MAX, ub = DBL_MAX;
  *result = -1;
  for (int i = 0; i < K; i++) {
    const ConstraintRec& c = ctx->cons[i];
    if (c.type == CXK_STATIC) continue;          // quadratic cost / equality: no restriction
    if (c.type != CXK_LINEAR) return CXK_SUCCESS;  // unsupported cone: failure (-1)
    if (out[2 * i] > out[2 * i + 1]) return CXK_SUCCESS;
    lb = std::max(lb, out[2 * i]);
    ub = std::min(ub, out[2 * i + 1]);
  }
  if (lb <= ub) *result = ub;
  return CXK_SUCCESS;
}

int cxk_step_scalars(cxk_context* ctx, double* out6) {
  CXK_ENTER(ctx);  // (a deferred launch has gone out here)
  if (ctx->scal_seq < 0 && LaunchStepScalars(ctx)) return CXK_FAILURE;  // not enqueued yet
  if (ctx->mb_seen < ctx->scal_seq && SyncMailbox(ctx)) return CXK_FAILURE;
  for (int i = 0; i < 6; i++) out6[i] = ctx->mbv[4 + i];
  ctx->scal_seq = -1;  // consumed: the next call computes them afresh
  return CXK_SUCCESS;
}

int cxk_kkt_solve_async(cxk_context* ctx, double k, double bs, double cs) {
  CXK_ENTER(ctx);
  if (DropTriple(ctx)) return CXK_FAILURE;
  if (LaunchSchur(ctx)) return CXK_FAILURE;
  // single GPU, Cholesky, no refinement copies of the assembled system: the assembly rides in
  // the first factor level's launch (BuildPlans decides whether the tree allows it)
  const bool fused = FusedAssembly(ctx);
  if (fused) {
    ctx->asm_pending.on = true;
    ctx->asm_pending.with_rhs = 1;
    ctx->asm_pending.k = k;
    ctx->asm_pending.bs = bs;
    ctx->asm_pending.cs = cs;
  } else if (LaunchGather(ctx, true, k, bs, cs)) {
    return CXK_FAILURE;
  }
  ctx->rhs_c[0] = k * bs;
  ctx->rhs_c[1] = k * cs;
  ctx->rhs_c[2] = -2.0;
  if (LaunchTree(ctx, 0, true, true)) return CXK_FAILURE;  // sharded contexts: local sweep, all-reduce, top, back
  CXK_DEMAND(!ctx->asm_pending.on, "internal error: the folded assembly was not launched");
  ctx->factor_seq = ++ctx->seq;
  ctx->redo_call = ctx->calls;
  return CXK_SUCCESS;
}

int cxk_solve_inplace(cxk_context* ctx, double* yh) {
  if (cxk_set_y(ctx, yh)) return CXK_FAILURE;
  if (LaunchTree(ctx, 1, true, true)) return CXK_FAILURE;
  return cxk_get_y(ctx, yh);
}

int cxk_get_y(cxk_context* ctx, double* yh) {
  CXK_ENTER(ctx);
  const int N = ctx->md.N;
  // a kernel writes y into pinned host memory: the first device-to-host hipMemcpy of a process
  // pays milliseconds of copy-engine set-up, which would dominate a whole C4 solve
  if (!ctx->pin_y) CXK_TRY(hipHostMalloc(reinterpret_cast<void**>(&ctx->pin_y), sizeof(double) * (size_t)N, hipHostMallocDefault));
  const double* ysrc = ctx->y.p;
  // a rank holds y for its own subtrees and the top: assemble the whole vector (callers that run
  // the exchange themselves, without a communicator, get the local vector: cxk_get_valid_variables)
  if (ctx->world > 1 && (ctx->coll_fn || ctx->rccl.comm)) {
    if (SettleBeforeUnmarked(ctx)) return CXK_FAILURE;
    masked_copy<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, ctx->d_count_mask.p, ctx->y.p, ctx->shard_tmp.p);
    CXK_TRY(hipGetLastError());
    if (ShardAllReduce(ctx, ctx->shard_tmp.p, (size_t)N, kOpSum)) return CXK_FAILURE;
    ysrc = ctx->shard_tmp.p;
  }
  copy_doubles<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, ysrc, ctx->pin_y);
  CXK_TRY(hipGetLastError());
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < N; i++) yh[ctx->md.permutation_inverse[i]] = ctx->pin_y[i];
  return CXK_SUCCESS;
}

int cxk_set_y(cxk_context* ctx, const double* yh) {
  CXK_ENTER(ctx);
  const int N = ctx->md.N;
  std::vector<double> yp(N);
  for (int i = 0; i < N; i++) yp[i] = yh[ctx->md.permutation_inverse[i]];
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(ctx->y.p, yp.data(), sizeof(double) * N, hipMemcpyHostToDevice));
  return CXK_SUCCESS;
}

static int PrepareStepImpl(cxk_context* ctx, int affine, double c_weight, double e_weight, double* info, bool take,
                           int* took, const double* cw_from = nullptr, double cw_scale = 1.0);
int cxk_prepare_step(cxk_context* ctx, int affine, double c_weight, double e_weight, double* info) {
  return PrepareStepImpl(ctx, affine, c_weight, e_weight, info, false, nullptr);
}
int cxk_prepare_take_step(cxk_context* ctx, double c_weight, double e_weight, double* info, int* took) {
  if (took) *took = 0;
  return PrepareStepImpl(ctx, 0, c_weight, e_weight, info, true, took);
}
}  // extern "C"
namespace {
// Kernel clocks of the step kernels (CXK_CLOCK_QUERY / _PREPARE / _TAKE): a program whose constraints
// are ONE group on a register kernel carries the event pair on that dispatch; anything else is
// bracketed by event records around its launches.
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
}  // namespace
extern "C" {
static int PrepareStepImpl(cxk_context* ctx, int affine, double c_weight, double e_weight, double* info, bool take,
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
  const int pmode = affine ? 2 : 0;
  bool rows_only = NonEmptyGroups(ctx) == 1;
  for (const Group& g : ctx->groups)
    if (!g.ids.empty())
      rows_only = rows_only && g.type == CXK_LMI && IsPrepareRows(LmiPrepareKernel(ctx, g, pmode));
  const StepClock clk = BeginStepClock(ctx, CXK_CLOCK_PREPARE, rows_only);
  for (Group& g : ctx->groups) {
    const int cnt = (int)g.ids.size();
    if (cnt == 0) continue;
    if (g.type == CXK_LMI) {
      switch (LmiPrepareKernel(ctx, g, pmode)) {
        case kPrepareLarge:
        case kAffineLarge:
          CXK_TRY(LmiLargePrepare(MakeLmi(g), sa, MakeLargeWs(g), 0, ctx->stream));
          break;
        case kPrepareRowsPacked:
        case kPrepareRowsExact:  // (the instance reads g.Apk when there is one)
          CXK_LAUNCH_CLOCKED(clk, (lmi_prepare_rows<0, 20, true>), (cnt + 3) / 4 + (tail.slots ? 1 + tail.ny : 0), 256, MakeLmi(g), sa, tail);
          break;
        case kPrepareRowsOdd:
        case kPrepareRowsEven:  // (an order below 20 on the same instance)
          CXK_LAUNCH_CLOCKED(clk, (lmi_prepare_rows<0, 20, false>), (cnt + 3) / 4 + (tail.slots ? 1 + tail.ny : 0), 256, MakeLmi(g), sa, tail);
          break;
        case kPrepareGeneric20:
        case kAffineGeneric20:
          lmi_prepare_generic<0, 20><<<cnt, 256, LmiPrepareLds(g.n, g.m), ctx->stream>>>(MakeLmi(g), sa);
          break;
        default:  // kPrepareGeneric, kAffineGeneric
          lmi_prepare_generic<0, 0><<<cnt, 256, LmiPrepareLds(g.n, g.m), ctx->stream>>>(MakeLmi(g), sa);
          break;
      }
    }
    else if (g.type == CXK_LINEAR)
      linear_prepare<0><<<cnt, 256, sizeof(double) * g.m, ctx->stream>>>(MakeVec(g), sa);
    else if (g.type == CXK_SOC)
      soc_prepare<0><<<cnt, 64, sizeof(double) * (size_t)(g.m + 3 * (g.n + 1)), ctx->stream>>>(
          MakeVec(g), sa);
    else if (g.type == CXK_QUAD)
      quad_prepare<0><<<cnt, 64, sizeof(double) * (size_t)(g.m + 4 * (g.n + 1)), ctx->stream>>>(MakeQuad(g), sa);
    else if (g.type == CXK_OCT)
      oct_prepare<0><<<cnt, 64, sizeof(double) * (size_t)g.m, ctx->stream>>>(MakeOct(g), sa);
  }
  EndStepClock(ctx, clk);
  CXK_TRY(hipGetLastError());
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

/* per-constraint outputs of the last cxk_prepare_step: {normsqrd, norminfd} for each constraint */
int cxk_get_step_info(cxk_context* ctx, double* out2k) {
  CXK_ENTER(ctx);
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(out2k, ctx->info2.p, sizeof(double) * 2 * ctx->cons.size(), hipMemcpyDeviceToHost));
  return CXK_SUCCESS;
}

int cxk_take_step(cxk_context* ctx, int affine, double e_weight, double step_size) {
  CXK_ENTER(ctx);
  if (affine) return CXK_SUCCESS;  // the affine update is applied inside PrepareStep
  return LaunchTakeStep(ctx, e_weight, step_size, nullptr);
}

static int LaunchTakeStep(cxk_context* ctx, double e_weight, double step_size, const double* step_from,
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
    if (g.type == CXK_LMI) {
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
    }
    else if (g.type == CXK_LINEAR)
      linear_take_step<<<GridFor((size_t)cnt * g.n, 256), 256, 0, ctx->stream>>>(MakeVec(g), sa);
    else if (g.type == CXK_SOC)
      soc_take_step<<<cnt, 64, sizeof(double) * (size_t)(4 * (g.n + 1)), ctx->stream>>>(MakeVec(g), sa);
    else if (g.type == CXK_QUAD)
      quad_take_step<<<cnt, 64, sizeof(double) * (size_t)(3 * (g.n + 1)), ctx->stream>>>(MakeQuad(g), sa);
    else if (g.type == CXK_OCT)
      oct_take_step<<<cnt, 64, 0, ctx->stream>>>(MakeOct(g), sa);
  }
  EndStepClock(ctx, clk);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

static int SlackEigenvaluesImpl(cxk_context* ctx, double c_weight, double* out, const MuRuleArgs* rule);
int cxk_weighted_slack_eigenvalues(cxk_context* ctx, double c_weight, double* out) {
  return SlackEigenvaluesImpl(ctx, c_weight, out, nullptr);
}
// rule != nullptr: the selection of the barrier parameter rides in the launch's tail workgroup and
// nobody waits (cxk_select_mu_async)
static int SlackEigenvaluesImpl(cxk_context* ctx, double c_weight, double* out, const MuRuleArgs* rule) {
  CXK_ENTER(ctx);
  StepArgs sa = MakeStep(ctx, ctx->info4.p, 0, c_weight, 0.0, 1.0);
  const bool with_tail = StepTailOk(ctx, 0);
  StepTail tail;
  tail.slots = nullptr;
  tail.rule.on = 0;
  if (with_tail && MakeStepTail(ctx, 1, &tail)) return CXK_FAILURE;
  if (rule) tail.rule = *rule;
  ctx->lanczos_calls++;
  bool rows_only = NonEmptyGroups(ctx) == 1;
  for (const Group& g : ctx->groups)
    if (!g.ids.empty())
      rows_only = rows_only && g.type == CXK_LMI && IsPrepareRows(LmiPrepareKernel(ctx, g, 1));
  const StepClock clk = BeginStepClock(ctx, CXK_CLOCK_QUERY, rows_only);
  for (Group& g : ctx->groups) {
    const int cnt = (int)g.ids.size();
    if (cnt == 0) continue;
    if (g.type == CXK_LMI) {
      switch (LmiPrepareKernel(ctx, g, 1)) {
        case kQueryLarge:
          CXK_TRY(LmiLargePrepare(MakeLmi(g), sa, MakeLargeWs(g), 1, ctx->stream));
          break;
        case kQueryRowsPacked:
        case kQueryRowsExact:
          CXK_LAUNCH_CLOCKED(clk, (lmi_prepare_rows<1, 20, true>), (cnt + 3) / 4 + (tail.slots ? 1 : 0), 256, MakeLmi(g), sa, tail);
          break;
        case kQueryRowsOdd:
        case kQueryRowsEven:  // (an order below 20 on the same instance)
          CXK_LAUNCH_CLOCKED(clk, (lmi_prepare_rows<1, 20, false>), (cnt + 3) / 4 + (tail.slots ? 1 : 0), 256, MakeLmi(g), sa, tail);
          break;
        case kQueryGeneric20:
          lmi_prepare_generic<1, 20><<<cnt, 256, LmiPrepareLds(g.n, g.m), ctx->stream>>>(MakeLmi(g), sa);
          break;
        default:  // kQueryGeneric
          lmi_prepare_generic<1, 0><<<cnt, 256, LmiPrepareLds(g.n, g.m), ctx->stream>>>(MakeLmi(g), sa);
          break;
      }
    }
    else if (g.type == CXK_LINEAR)
      linear_prepare<1><<<cnt, 256, sizeof(double) * g.m, ctx->stream>>>(MakeVec(g), sa);
    else if (g.type == CXK_SOC)
      soc_prepare<1><<<cnt, 64, sizeof(double) * (size_t)(g.m + 3 * (g.n + 1)), ctx->stream>>>(
          MakeVec(g), sa);
    else if (g.type == CXK_QUAD)
      quad_prepare<1><<<cnt, 64, sizeof(double) * (size_t)(g.m + 4 * (g.n + 1)), ctx->stream>>>(MakeQuad(g), sa);
    else if (g.type == CXK_OCT)
      oct_prepare<1><<<cnt, 64, sizeof(double) * (size_t)g.m, ctx->stream>>>(MakeOct(g), sa);
  }
  EndStepClock(ctx, clk);
  CXK_TRY(hipGetLastError());
  if (ReduceStepInfoAndSync(ctx, 1, ctx->info4.p, nullptr, nullptr, with_tail, false, rule == nullptr, rule))
    return CXK_FAILURE;
  if (out && !rule)
    for (int i = 0; i < 4; i++) out[i] = ctx->mbv[i];
  return CXK_SUCCESS;
}

// ---- the barrier parameter selected on the device: conex::Solve's iteration without the host round
// trip between the eigenvalue query and the Newton direction (cone_program.cc:366-413).
static bool DeviceMuOk(const cxk_context* ctx) {
  // one GPU, Cholesky on the device (the QR mode solves on the host), every TakeStep kernel able to
  // take its step length from the device (TakeStepFromDeviceOk: no equality rows, no LMI beyond LDS)
  return !ctx->no_device_mu && ctx->world <= 1 && ctx->solver_mode != 2 && TakeStepFromDeviceOk(ctx);
}
int cxk_device_mu_supported(cxk_context* ctx) {
  if (!ctx || CheckReady(ctx)) return 0;
  return DeviceMuOk(ctx) ? 1 : 0;
}
int cxk_select_mu_async(cxk_context* ctx, double c_weight, double divergence_upper_bound, int rank, double prev,
                        double lb, double ub) {
  CXK_ENTER_KEEP(ctx);  // (binds the context's device for the allocation below; the query itself enters again)
  CXK_DEMAND(DeviceMuOk(ctx), "cxk_select_mu_async: not supported by this program (cxk_device_mu_supported)");
  if (ctx->mu_dev.n != 1) CXK_TRY(ctx->mu_dev.alloc(1, true));
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
int cxk_newton_direction_device_mu(cxk_context* ctx, double bs, double cs) {
  CXK_ENTER(ctx);
  CXK_DEMAND(DeviceMuOk(ctx) && ctx->mu_dev.n == 1, "cxk_newton_direction_device_mu: no barrier parameter on the device");
  // behind cxk_factor_solve_triple_async the direction is a combination of the three solutions at hand
  // (cone_program.cc:409-411 by linearity): one elementwise launch instead of a sweep over the tree
  if (ctx->y3_valid && bs == ctx->y3_bs && cs == ctx->y3_cs) {  // (other scalings: the sweep below)
    ctx->y3_valid = false;
    ctx->y_deferred = true;  // normally combined inside the PrepareStep launch that follows (PrepareStepImpl)
    if (ctx->no_y_deferral && FlushDirection(ctx)) return CXK_FAILURE;
    return CXK_SUCCESS;
  }
  RhsIn f{};
  f.form = 1;
  f.b = ctx->b.p;
  f.AQc = ctx->AQc.p;
  f.AW = ctx->AW.p;
  f.k = 0.0;
  f.k_from = ctx->mu_dev.p;
  f.bs = bs;
  f.cs = cs;
  return SolveWithRhs(ctx, f);
}
int cxk_prepare_take_step_device_mu(cxk_context* ctx, double c_scaling, double e_weight, double* info, int* took,
                                    double* inv_sqrt_mu) {
  if (took) *took = 0;
  if (!ctx || CheckReady(ctx)) return CXK_FAILURE;
  CXK_DEMAND(DeviceMuOk(ctx) && ctx->mu_dev.n == 1, "cxk_prepare_take_step_device_mu: no barrier parameter on the device");
  if (PrepareStepImpl(ctx, 0, 0.0, e_weight, info, true, took, ctx->mu_dev.p, c_scaling)) return CXK_FAILURE;
  if (inv_sqrt_mu) *inv_sqrt_mu = ctx->mbv[13];
  return CXK_SUCCESS;
}

// ------------------------------------------------------------- inspection
int cxk_get_slab(cxk_context* ctx, double* out) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->segments == 0, "the factor of this chain-shaped program is stored in its segment-parallel order, not in the "
                                 "reference's block layout: set CXK_CHAIN_SEGMENTS=0 (or cxk_set_chain_segments(ctx, 0)) to inspect it");
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(out, ctx->slab.p, sizeof(double) * (size_t)ctx->lay.slab_size,
                    hipMemcpyDeviceToHost));
  return CXK_SUCCESS;
}
int cxk_set_slab(cxk_context* ctx, const double* in) {
  CXK_ENTER(ctx);
  if (DropTriple(ctx)) return CXK_FAILURE;
  CXK_DEMAND(ctx->segments == 0, "cxk_set_slab needs the reference's block layout: CXK_CHAIN_SEGMENTS=0");
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(ctx->slab.p, in, sizeof(double) * (size_t)ctx->lay.slab_size,
                    hipMemcpyHostToDevice));
  return CXK_SUCCESS;
}
int cxk_get_constraint_schur(cxk_context* ctx, int i, double* G, double* AW, double* AQc,
                             double* scalars) {
  CXK_ENTER(ctx);
  CXK_DEMAND(i >= 0 && i < (int)ctx->cons.size(), "invalid constraint");
  const int m = ctx->cons[i].m;
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  if (G)
    CXK_TRY(hipMemcpy(G, ctx->G.p + ctx->g_off[i], sizeof(double) * (size_t)m * m,
                      hipMemcpyDeviceToHost));
  if (AW)
    CXK_TRY(hipMemcpy(AW, ctx->AWc.p + ctx->r_off[i], sizeof(double) * m, hipMemcpyDeviceToHost));
  if (AQc)
    CXK_TRY(hipMemcpy(AQc, ctx->AQcc.p + ctx->r_off[i], sizeof(double) * m, hipMemcpyDeviceToHost));
  if (scalars)
    CXK_TRY(hipMemcpy(scalars, ctx->sc.p + 2 * i, sizeof(double) * 2, hipMemcpyDeviceToHost));
  return CXK_SUCCESS;
}
int cxk_get_residuals(cxk_context* ctx, double* AW, double* AQc, double* scalars) {
  CXK_ENTER(ctx);
  const int N = ctx->md.N;
  std::vector<double> t(N);
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  if (AW) {
    CXK_TRY(hipMemcpy(t.data(), ctx->AW.p, sizeof(double) * N, hipMemcpyDeviceToHost));
    for (int i = 0; i < N; i++) AW[ctx->md.permutation_inverse[i]] = t[i];
  }
  if (AQc) {
    CXK_TRY(hipMemcpy(t.data(), ctx->AQc.p, sizeof(double) * N, hipMemcpyDeviceToHost));
    for (int i = 0; i < N; i++) AQc[ctx->md.permutation_inverse[i]] = t[i];
  }
  if (scalars) CXK_TRY(hipMemcpy(scalars, ctx->sys_sc.p, sizeof(double) * 2, hipMemcpyDeviceToHost));
  return CXK_SUCCESS;
}

int cxk_exchange_buffer(cxk_context* ctx, void** dev_ptr, long* count) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->world > 1, "exchange buffer exists only for sharded contexts");
  *dev_ptr = ctx->xbuf.p;
  *count = (long)(ctx->n_xs + 3 * (int64_t)ctx->n_xv + 4);
  return CXK_SUCCESS;
}

// host copies of the exchange buffer (tests; a real run all-reduces the device buffer in place)
int cxk_exchange_download(cxk_context* ctx, double* out) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->world > 1, "exchange buffer exists only for sharded contexts");
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(out, ctx->xbuf.p, sizeof(double) * (size_t)(ctx->n_xs + 3 * (int64_t)ctx->n_xv + 4),
                    hipMemcpyDeviceToHost));
  return CXK_SUCCESS;
}
int cxk_exchange_upload(cxk_context* ctx, const double* in) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->world > 1, "exchange buffer exists only for sharded contexts");
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(ctx->xbuf.p, in, sizeof(double) * (size_t)(ctx->n_xs + 3 * (int64_t)ctx->n_xv + 4),
                    hipMemcpyHostToDevice));
  return CXK_SUCCESS;
}

// Sharded KKT solve, part 1 (no communication): assemble own constraints, factor + forward own
// subtrees, fold their updates into the partial top blocks and pack the exchange buffer.
int cxk_kkt_local_async(cxk_context* ctx, double k, double bs, double cs) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->world > 1, "cxk_kkt_local_async needs cxk_set_shard(world > 1)");
  if (LaunchSchur(ctx)) return CXK_FAILURE;
  if (LaunchGather(ctx, true, k, bs, cs)) return CXK_FAILURE;
  for (int l = 0; l < ctx->cut_level; l++)
    if (LaunchSweep(ctx, l, l + 1, 0, false, true)) return CXK_FAILURE;
  ExchangeArgs a = MakeExchange(ctx, k, bs, cs);
  const size_t work = (size_t)std::max<int64_t>(ctx->n_xs, ctx->n_xv);
  exchange_pack<<<GridFor(work, 256), 256, 0, ctx->stream>>>(a);
  CXK_TRY(hipGetLastError());
  ctx->factor_seq = ++ctx->seq;
  return CXK_SUCCESS;
}

// Part 2, after the caller has sum-reduced the exchange buffer across ranks: unpack the
// completed top, factor/solve it (replicated), back-substitute the own subtrees.
int cxk_kkt_finish_async(cxk_context* ctx, double k, double bs, double cs) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->world > 1, "cxk_kkt_finish_async needs cxk_set_shard(world > 1)");
  ExchangeArgs a = MakeExchange(ctx, k, bs, cs);
  const size_t work = (size_t)std::max<int64_t>(ctx->n_xs, ctx->n_xv);
  exchange_unpack<<<GridFor(work, 256), 256, 0, ctx->stream>>>(a);
  CXK_TRY(hipGetLastError());
  const int nlev = ctx->nlev, top = ctx->top_level;
  for (int l = ctx->cut_level; l < top; l++)
    if (LaunchSweep(ctx, l, l + 1, 0, false, true)) return CXK_FAILURE;
  if (top < nlev)
    if (LaunchSweep(ctx, top, nlev, 0, true, true)) return CXK_FAILURE;
  for (int l = top - 1; l >= 0; l--)
    if (LaunchSweep(ctx, l, l + 1, 2, false, true)) return CXK_FAILURE;
  ctx->factor_seq = ++ctx->seq;
  return CXK_SUCCESS;
}

int cxk_owns_constraint(const cxk_context* ctx, int i) {
  if (!ctx || !ctx->finalized || i < 0 || i >= (int)ctx->cons.size()) return 0;
  return ctx->owned[i];
}

int cxk_get_valid_variables(const cxk_context* ctx, unsigned char* mask /* N, original order */) {
  if (!ctx || !ctx->finalized) return CXK_FAILURE;
  for (int p = 0; p < ctx->md.N; p++) mask[ctx->md.permutation_inverse[p]] = ctx->var_valid[p];
  return CXK_SUCCESS;
}

int cxk_shard_info(const cxk_context* ctx, int* cut_level, int* num_levels, long* exchange_count) {
  if (!ctx || !ctx->finalized) return CXK_FAILURE;
  if (cut_level) *cut_level = ctx->cut_level;
  if (num_levels) *num_levels = ctx->nlev;
  if (exchange_count) *exchange_count = ctx->world > 1 ? (long)(ctx->n_xs + 3 * (int64_t)ctx->n_xv + 4) : 0;
  return CXK_SUCCESS;
}

int cxk_gemm_f64(int device, int ta, int tb, int M, int N, int K, int batch, const double* A,
                 const double* B, double* C, double alpha, double beta, int lower_only, int splits,
                 int reps, double* avg_ms) {
  if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || !A || !B || !C) return CXK_FAILURE;
  cxk_context scratch_ctx;  // carries the error string for CXK_TRY
  cxk_context* ctx = &scratch_ctx;
  DeviceGuard guard(device);
  const size_t na = (size_t)M * K, nb = (size_t)K * N, nc = (size_t)M * N;
  DevBuf<double> dA, dB, dC, dP;
  CXK_TRY(dA.alloc(na * batch));
  CXK_TRY(dB.alloc(nb * batch));
  CXK_TRY(dC.alloc(nc * batch));
  if (splits > 1) CXK_TRY(dP.alloc(nc * batch * splits));
  CXK_TRY(hipMemcpy(dA.p, A, sizeof(double) * na * batch, hipMemcpyHostToDevice));
  CXK_TRY(hipMemcpy(dB.p, B, sizeof(double) * nb * batch, hipMemcpyHostToDevice));
  GemmArgs g{};
  g.M = M;
  g.N = N;
  g.K = K;
  g.A = dA.p;
  g.lda = ta ? K : M;
  g.sA1 = (int64_t)na;
  g.B = dB.p;
  g.ldb = tb ? N : K;
  g.sB1 = (int64_t)nb;
  g.C = dC.p;
  g.ldc = M;
  g.sC1 = (int64_t)nc * (splits > 1 ? 1 : 1);
  g.inner = 1;
  g.alpha = alpha;
  g.beta = beta;
  g.lower_only = lower_only;
  g.splits = splits > 1 ? splits : 1;
  g.sCs = (int64_t)nc * batch;  // partial s of batch b at part + s*sCs + b*sC1
  hipEvent_t e0, e1;
  CXK_TRY(hipEventCreate(&e0));
  CXK_TRY(hipEventCreate(&e1));
  float total = 0;
  const int n = reps > 0 ? reps : 1;
  for (int r = 0; r < n; r++) {
    // beta != 0 accumulates into C: restore the input every repetition (untimed)
    CXK_TRY(hipMemcpy(dC.p, C, sizeof(double) * nc * batch, hipMemcpyHostToDevice));
    CXK_TRY(hipEventRecord(e0, nullptr));
    CXK_TRY(LaunchGemmSplitK(g, ta != 0, tb != 0, batch, dP.p, nullptr));
    CXK_TRY(hipEventRecord(e1, nullptr));
    CXK_TRY(hipEventSynchronize(e1));
    float ms = 0;
    CXK_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (r > 0 || n == 1) total += ms;
  }
  if (avg_ms) *avg_ms = total / (n > 1 ? n - 1 : 1);
  CXK_TRY(hipMemcpy(C, dC.p, sizeof(double) * nc * batch, hipMemcpyDeviceToHost));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return CXK_SUCCESS;
}

int cxk_dense_top_columns(const cxk_context* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  return ctx->top_dense.on ? ctx->top_dense.args.T : 0;
}

int cxk_count_sparse_lmi(const cxk_context* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  int k = 0;
  for (size_t i = 0; i < ctx->cons.size(); i++) k += ctx->cons[i].type == CXK_LMI && ctx->owned[i] && ctx->cons[i].sparse;
  return k;
}

int cxk_fused_assembly(const cxk_context* ctx) { return ctx && ctx->fused_asm ? 1 : 0; }
/* 1 when assembly, factorization and solve of a KKT solve run as one launch (tree_fused.hip) */
int cxk_fused_tree(const cxk_context* ctx) { return ctx && ctx->fused_tree ? 1 : 0; }

int cxk_fused_tree_timed_out(cxk_context* ctx) {
  if (!ctx || !ctx->timeout_unreported) return 0;
  ctx->timeout_unreported = false;
  return 1;
}

int cxk_debug_force_fused_timeout(cxk_context* ctx) {
  if (!ctx || !ctx->fx_flag || !ctx->fused_tree) return CXK_FAILURE;
  *ctx->fx_flag = 1.0;
  return CXK_SUCCESS;
}

int cxk_debug_fused_timeout_at(cxk_context* ctx, int launch_index, int which) {
  if (!ctx || !ctx->device_ready || !ctx->fx_flag || !ctx->fused_tree) return CXK_FAILURE;
  const bool stream_ordered = (which & CXK_DEBUG_FUSED_STREAM_ORDERED) != 0;
  which &= ~CXK_DEBUG_FUSED_STREAM_ORDERED;
  // (behind the up launch, only a host word raised in time reaches the exchange: stream order is for the top)
  if (stream_ordered && which != CXK_DEBUG_FUSED_SHARD_TOP) return CXK_FAILURE;
  if (which != CXK_DEBUG_FUSED_FACTOR && which != CXK_DEBUG_FUSED_SHARD_UP && which != CXK_DEBUG_FUSED_SHARD_TOP)
    return CXK_FAILURE;
  // (a site this context never launches would never fire: refused, so that a test cannot pass vacuously)
  if ((which == CXK_DEBUG_FUSED_FACTOR) != (ctx->world <= 1) || (ctx->world > 1 && !ctx->fused_shard))
    return CXK_FAILURE;
  ctx->debug_timeout_at = launch_index >= 0 ? ctx->fused_launches + launch_index : -1;
  ctx->debug_timeout_site = which;
  ctx->debug_stream_ordered = stream_ordered;
  return CXK_SUCCESS;
}

int cxk_count_lmi_kernel(const cxk_context* ctx, int which) {
  if (!ctx || !ctx->device_ready) return -1;
  int k = 0;
  for (const Group& g : ctx->groups) {
    if (g.type != CXK_LMI) continue;
    const int kind = g.sparse ? 4 : g.schur_gemm ? 3 : g.mfma ? 2 : 0;
    if (kind == which) k += (int)g.ids.size();
  }
  return k;
}

int cxk_lmi_kernels(const cxk_context* ctx, int constraint, int out[5]) {
  if (!ctx || !ctx->device_ready || !out || constraint < 0 || constraint >= (int)ctx->cons.size()) return CXK_FAILURE;
  const ConstraintRec& c = ctx->cons[constraint];
  if (c.type != CXK_LMI || !ctx->owned[constraint]) return CXK_FAILURE;
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

int cxk_assembly_work(const cxk_context* ctx, double* bytes, double* flops) {
  if (!ctx || !ctx->finalized) return CXK_FAILURE;
  double B = 0, F = 0;
  for (size_t i = 0; i < ctx->cons.size(); i++) {
    const ConstraintRec& c = ctx->cons[i];
    if (c.type != CXK_LMI || !ctx->owned[i]) continue;
    const double n = c.n, m = c.m;
    // FLOPs = 4 n^3 (m+1) + n^2 (m^2 + 3m + 4) + n m ; bytes = 8 [m n^2 + 2 n^2 + m(m+1)/2 + 2m]
    F += 4 * n * n * n * (m + 1) + n * n * (m * m + 3 * m + 4) + n * m;
    B += 8.0 * (m * n * n + 2 * n * n + m * (m + 1) / 2 + 2 * m);
  }
  if (bytes) *bytes = B;
  if (flops) *flops = F;
  return CXK_SUCCESS;
}

#ifdef CXK_CHAIN_STAMPS
int cxk_debug_stamps(long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cxk_stamp), 96 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
int cxk_debug_select(int) { return 0; }
#endif
#ifdef CXK_DEBUG_STAMPS
int cxk_debug_sparse_stamps(long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sparse_stamp), 8 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
int cxk_debug_stamps(long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cxk_stamp), 96 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
int cxk_debug_select(int want) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_cxk_want), &want, sizeof(int)) == hipSuccess ? 0 : 1;
}
#endif

// SupernodalKKTSolver::SetIterativeRefinementIterations (kkt_solver.h:37): every solve after the
// next factorization is followed by `iterations` steps  y <- y + K^-1 (b - K y).
int cxk_set_iterative_refinement(cxk_context* ctx, int iterations) {
  CXK_ENTER(ctx);
  CXK_DEMAND(iterations >= 0, "refinement iterations must be >= 0");
  CXK_DEMAND(ctx->world <= 1 || iterations == 0, "iterative refinement is single-GPU for now");
  if (iterations > 0 && ctx->slab0.n == 0) {
    const size_t N = (size_t)ctx->md.N;
    CXK_TRY(ctx->slab0.alloc(ctx->slab.n));
    CXK_TRY(ctx->rhs0.alloc(N));
    CXK_TRY(ctx->mv_u.alloc(N));
    CXK_TRY(ctx->ysave.alloc(N));
    CXK_TRY(ctx->mvb.alloc(ctx->updb.n, true));
  }
  if (iterations != ctx->refine_iters) ctx->slab0_valid = false;
  ctx->refine_iters = iterations;
  return CXK_SUCCESS;
}

int cxk_set_solver_mode(cxk_context* ctx, int mode) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(mode == 0 || mode == 1 || mode == 2, "solver mode must be 0 (LLT), 1 (LDLT) or 2 (QR)");
  ctx->solver_mode = mode == 2 ? 2 : 0;  // LLT vs LDLT follows the structure (kkt_solver.cc:180-193)
  ctx->qr.valid = false;
  return CXK_SUCCESS;
}

int cxk_phase_timers(cxk_context* ctx, int on) {
  if (!ctx) return CXK_FAILURE;
  ctx->phase_on = on != 0;
  return CXK_SUCCESS;
}

int cxk_phase_mark(cxk_context* ctx, int phase) {
  if (!ctx || !ctx->phase_on) return CXK_SUCCESS;
  CXK_ENTER_KEEP(ctx);  // only records an event: a deferred gather stays deferred (the timed run takes the untimed run's path)
  CXK_DEMAND(phase >= 0 && phase < CXK_PHASE_COUNT, "unknown phase");
  hipEvent_t ev;
  if (!ctx->phase_pool.empty()) {
    ev = ctx->phase_pool.back();
    ctx->phase_pool.pop_back();
  } else {
    CXK_TRY(hipEventCreate(&ev));
  }
  CXK_TRY(hipEventRecord(ev, ctx->stream));
  ctx->phase_marks.emplace_back(ev, phase);
  return CXK_SUCCESS;
}

int cxk_phase_read(cxk_context* ctx, double* us, int reset) {
  if (!ctx || !us) return CXK_FAILURE;
  CXK_ENTER_KEEP(ctx);
  if (!ctx->phase_marks.empty()) {
    CXK_TRY(hipEventSynchronize(ctx->phase_marks.back().first));
    for (size_t k = 0; k + 1 < ctx->phase_marks.size(); k++) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->phase_marks[k].first, ctx->phase_marks[k + 1].first) == hipSuccess)
        ctx->phase_us[ctx->phase_marks[k].second] += 1e3 * ms;
    }
    for (auto& m : ctx->phase_marks) ctx->phase_pool.push_back(m.first);
    ctx->phase_marks.clear();
  }
  for (int k = 0; k < CXK_PHASE_COUNT; k++) us[k] = ctx->phase_us[k];
  if (reset)
    for (int k = 0; k < CXK_PHASE_COUNT; k++) ctx->phase_us[k] = 0;
  return CXK_SUCCESS;
}

int cxk_enable_timing(cxk_context* ctx, int on) {
  if (!ctx) return CXK_FAILURE;
  ctx->timing = on != 0;
  ctx->timing_period = on > 1 ? on : 1;
  for (int k = 0; k < CXK_CLOCK_COUNT; k++) ctx->timing_tick[k] = 0;
  return CXK_SUCCESS;
}

int cxk_kernel_clock(cxk_context* ctx, int which, int reset, double* avg_ms) {
  if (!ctx || which < 0 || which >= CXK_CLOCK_COUNT) return 0;
  const int n = ctx->time_samples[which];
  if (avg_ms) *avg_ms = n ? ctx->time_acc_ms[which] / n : 0.0;
  if (reset) {
    ctx->time_acc_ms[which] = 0;
    ctx->time_samples[which] = 0;
  }
  return n;
}

int cxk_kernel_time(cxk_context* ctx, int reset, double* avg_ms) {
  return cxk_kernel_clock(ctx, CXK_CLOCK_ASSEMBLY, reset, avg_ms);
}

}  // extern "C"
