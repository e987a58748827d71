// The launches of the elimination tree: assembly gather, right-hand sides, level / range / chain / dense-top
// sweeps, the whole-tree launch with its time-out handling, iterative refinement, the step scalars and the
// exchange kernels of sharded contexts.  Owns the plain kernels of kernels_kkt_vec.hip.h and the instances
// of the templates of kernels_tree_level.hip.h, kernels_kkt_big and kernels_kkt_top (and copy_doubles below).
#include "kkt_launch.h"
#include "kernels_gemm.hip.h"
#include "kernels_kkt_big.hip.h"
#include "kernels_kkt_top.hip.h"
#include "kernels_kkt_vec.hip.h"    // its only includer: the plain kernels live in this unit
#include "kernels_tree_level.hip.h"  // its only includer

extern "C" {

__global__ void copy_doubles(int n, const double* __restrict__ src, double* __restrict__ dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

#ifdef CXK_CHAIN_STAMPS
int cxk_debug_stamps(long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cxk_stamp), 96 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
int cxk_debug_select(int) { return 0; }
#endif
#ifdef CXK_DEBUG_STAMPS
int cxk_debug_stamps(long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cxk_stamp), 96 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
int cxk_debug_select(int want) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_cxk_want), &want, sizeof(int)) == hipSuccess ? 0 : 1;
}
#endif

}  // extern "C"

namespace cxk_host {

// The register shapes (NSMAX, SMAX) the level kernels are compiled for, and the pairs of two different ones
// (the smaller first) that share a launch.  Each list is written once; every use expands it.
#define CXK_FOR_EACH_LEVEL_SHAPE(X) X(8, 8) X(16, 8) X(24, 0) X(24, 8) X(32, 16)
#define CXK_FOR_EACH_SHAPE_PAIR(X)                                                \
  X(8, 8, 16, 8) X(8, 8, 24, 0) X(8, 8, 24, 8) X(8, 8, 32, 16) X(16, 8, 24, 0)    \
  X(16, 8, 24, 8) X(16, 8, 32, 16) X(24, 0, 24, 8) X(24, 0, 32, 16) X(24, 8, 32, 16)

// two-shape chains tree_chain_lean is compiled for (LaunchChain): a pair holding <24,0>, or <8,8> with
// <16,8> (second-order cones of dimension 10 with a root of 10 columns: BASELINE config 3)
constexpr bool ChainMixedPair(int sa, int sb) {  // sa < sb
  return sa == (24 << 8) || sb == (24 << 8) || (sa == (8 << 8 | 8) && sb == (16 << 8 | 8));
}
bool ChainPairCompiled(int sa, int sb) {
  if (sb == 0 || sa == sb) return true;
  if (sa > sb) std::swap(sa, sb);
  return ChainMixedPair(sa, sb);
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

// Kernels of this unit that may be launched with more than the default 64 KB of dynamic LDS.
hipError_t RaiseTreeLdsLimits() {
  static PerDeviceOnce once;  // function attributes are per device: every device a context is built on
  return once.run([] {
    return RaiseDynamicLds({
#define CXK_PAIR_K(NA_, SA_, NB_, SB_)                                              \
  reinterpret_cast<const void*>(&tree_factor_level2<NA_, SA_, NB_, SB_, true>),      \
      reinterpret_cast<const void*>(&tree_factor_level2<NA_, SA_, NB_, SB_, false>),
        CXK_FOR_EACH_SHAPE_PAIR(CXK_PAIR_K)
#undef CXK_PAIR_K
        reinterpret_cast<const void*>(&tree_chain_lean<0, 32, 16, 32, 16>),
        reinterpret_cast<const void*>(&tree_chain_lean<0, 24, 0, 32, 16>),
#define CXK_LEVEL_K(NS_, S_)                                           \
  reinterpret_cast<const void*>(&tree_factor_level<NS_, S_, true>),     \
      reinterpret_cast<const void*>(&tree_factor_level<NS_, S_, false>),
        CXK_FOR_EACH_LEVEL_SHAPE(CXK_LEVEL_K)
#undef CXK_LEVEL_K
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
    });
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
            CXK_FOR_EACH_SHAPE_PAIR(CXK_PAIR_ASM)
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
          CXK_FOR_EACH_SHAPE_PAIR(CXK_PAIR)
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
          CXK_FOR_EACH_LEVEL_SHAPE(CXK_LEVEL_ASM)
#undef CXK_LEVEL_ASM
          CXK_DEMAND(done, "internal error: no tree_factor_level_asm instance for the first level's shape");
          continue;
        }
        CXK_FOR_EACH_LEVEL_SHAPE(CXK_LEVEL)
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

namespace {
template <int NP_, int SP_>
bool LaunchBackPairUnder(cxk_context* ctx, const cxk_context::BackPair& bp) {  // parent shape <NP_, SP_>
#define CXK_BACK_PAIR(NC_, SC_)                                                                        \
  if (bp.shape_c == ((NC_) << 8 | (SC_))) {                                                            \
    tree_backward_pair<NP_, SP_, NC_, SC_><<<bp.nwg, 576, 0, ctx->stream>>>(ctx->p_rec.p, bp.tab.p,    \
                                                                            ctx->slab.p, ctx->y.p);    \
    return true;                                                                                       \
  }
  CXK_FOR_EACH_LEVEL_SHAPE(CXK_BACK_PAIR)
#undef CXK_BACK_PAIR
  return false;
}
}  // namespace
int LaunchBackPair(cxk_context* ctx, const cxk_context::BackPair& bp) {
  bool done = false;
#define CXK_BACK_PAIR_ROW(NP_, SP_) \
  if (!done && bp.shape_p == ((NP_) << 8 | (SP_))) done = LaunchBackPairUnder<NP_, SP_>(ctx, bp);
  CXK_FOR_EACH_LEVEL_SHAPE(CXK_BACK_PAIR_ROW)
#undef CXK_BACK_PAIR_ROW
  CXK_DEMAND(done, "internal error: no tree_backward_pair instance for the levels' shapes");
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// The chain at the top of the tree (levels [chain_level, nlev), one supernode each): up and
// straight back down in one launch of one wavefront.  mode 0 factor + forward, mode 1 forward.
// Compiled for one shape, and for the mixed pairs ChainPairCompiled names.
namespace {
template <int NA_, int SA_, int NB_, int SB_>
void LaunchChainAs(cxk_context* ctx, int mode, int pos0, int nchain) {
  const size_t lds = sizeof(double) * 65 * ((NA_) > (NB_) ? (NA_) : (NB_)) + sizeof(SnRec) * (size_t)std::min(nchain, kChainRing);
  if (mode == 0)
    tree_chain_lean<0, NA_, SA_, NB_, SB_><<<1, 64, lds, ctx->stream>>>(
        ctx->plan, ctx->p_rec.p, pos0, nchain, ctx->slab.p, ctx->y.p, ctx->d_fail.p, RhsIn{});
  else
    tree_chain_lean<1, NA_, SA_, NB_, SB_><<<1, 64, lds, ctx->stream>>>(
        ctx->plan, ctx->p_rec.p, pos0, nchain, ctx->slab.p, ctx->y.p, ctx->d_fail.p, ctx->rhs_in);
}
}  // namespace
int LaunchChain(cxk_context* ctx, int mode) {
  const int nlev = (int)ctx->level_ptr.size() - 1;
  // one supernode per chain level: their records are consecutive in level order
  const int pos0 = ctx->level_ptr[ctx->chain_level], nchain = nlev - ctx->chain_level;
  const int sa = ctx->chain_a, sb = ctx->chain_b;
  bool done = false;
#define CXK_CHAIN(NA_, SA_, NB_, SB_)                                        \
  if (!done && sa == ((NA_) << 8 | (SA_)) && sb == ((NB_) << 8 | (SB_))) {   \
    done = true;                                                             \
    LaunchChainAs<NA_, SA_, NB_, SB_>(ctx, mode, pos0, nchain);              \
  }
#define CXK_CHAIN_ONE(NS_, S_) CXK_CHAIN(NS_, S_, NS_, S_)
  // Only the mixed pairs ChainMixedPair names are compiled: for the others the statement is discarded, LaunchChainAs
  // is not instantiated and no tree_chain_lean kernel comes into being (the set of kernels is part of what
  // tools/compare_device_code.py checks; ChainPairCompiled tells kkt_plans.hip which pairs may be planned).
#define CXK_CHAIN_MIXED(NA_, SA_, NB_, SB_) \
  if constexpr (ChainMixedPair((NA_) << 8 | (SA_), (NB_) << 8 | (SB_))) CXK_CHAIN(NA_, SA_, NB_, SB_)
  CXK_FOR_EACH_LEVEL_SHAPE(CXK_CHAIN_ONE)
  CXK_FOR_EACH_SHAPE_PAIR(CXK_CHAIN_MIXED)
#undef CXK_CHAIN_MIXED
#undef CXK_CHAIN_ONE
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
  a.img = ctx->fx_img.p;
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
      if (r.lo == l) return &r;
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

int LaunchBuildRhs(cxk_context* ctx, double k, double bs, double cs, int* fail, const double* k_from) {
  const int N = ctx->md.N;
  build_rhs<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, k, bs, cs, ctx->b.p, ctx->AQc.p, ctx->AW.p, ctx->y.p, fail, k_from);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}
int LaunchBuildRhsComb(cxk_context* ctx, double cb, double cq, double cw, int* fail) {
  const int N = ctx->md.N;
  build_rhs_comb<<<GridFor(N, 256), 256, 0, ctx->stream>>>(N, cb, cq, cw, ctx->b.p, ctx->AQc.p, ctx->AW.p, ctx->y.p, fail);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// ... and the latest factor-and-solve again on the level kernels: the Schur blocks are still in the
// arena, the right-hand side was cb b + cq AQc + cw AW with the coefficients of ctx->rhs_c.
int RedoFactorSolveOnLevels(cxk_context* ctx) {
  if (DisableFusedTree(ctx)) return CXK_FAILURE;
  ctx->asm_pending.on = false;
  ctx->asm_deferred = false;
  if (LaunchGather(ctx, false, 0, 0, 0)) return CXK_FAILURE;
  CXK_TRY(hipMemsetAsync(ctx->d_fail.p, 0, 2 * sizeof(int), ctx->stream));
  if (LaunchBuildRhsComb(ctx, ctx->rhs_c[0], ctx->rhs_c[1], ctx->rhs_c[2], ctx->d_fail.p)) return CXK_FAILURE;
  if (LaunchTree(ctx, 0, true, true)) return CXK_FAILURE;
  ctx->factor_seq = ++ctx->seq;
  return CXK_SUCCESS;
}

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


int LaunchMaskedCopy(cxk_context* ctx, int n, const double* in, double* out) {
  masked_copy<<<GridFor(n, 256), 256, 0, ctx->stream>>>(n, ctx->d_count_mask.p, in, out);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}
int LaunchMaskedCopyPairs(cxk_context* ctx, int K, const double* in, double* out) {
  masked_copy_pairs<<<GridFor((size_t)2 * K, 256), 256, 0, ctx->stream>>>(K, ctx->d_mask.p, in, out);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}
int LaunchCopyDoubles(cxk_context* ctx, int n, const double* src, double* dst) {
  copy_doubles<<<GridFor(n, 256), 256, 0, ctx->stream>>>(n, src, dst);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// One of the exchange kernels of a sharded context, right-hand side cb b + cq AQc + cw AW.
int LaunchExchange(cxk_context* ctx, ExchangeKernel which, double cb, double cq, double cw) {
  ExchangeArgs a = MakeExchange(ctx, 0, 0, 0);
  a.cb = cb;
  a.cq = cq;
  a.cw = cw;
  const int grid = GridFor((size_t)std::max<int64_t>(std::max<int64_t>(ctx->n_xs, ctx->n_xv), 1), 256);
  const int grid_solve = GridFor((size_t)ctx->n_xv, 256);
  if (which == kExchangePackSolve || which == kExchangeUnpackSolve) {
    a.tag = ctx->fx_flag ? ctx->shard_fused_tag : 0;  // (x[n_xv]: the time-out mark, ShardMark)
    a.host_flag = ctx->fx_flag;
  }
  switch (which) {
    case kExchangePack: exchange_pack<<<grid, 256, 0, ctx->stream>>>(a); break;
    case kExchangeUnpack: exchange_unpack<<<grid, 256, 0, ctx->stream>>>(a); break;
    case kExchangeUnpackMatrix: exchange_unpack_matrix<<<grid, 256, 0, ctx->stream>>>(a); break;
    case kExchangePackSolve: exchange_pack_solve<<<grid_solve, 256, 0, ctx->stream>>>(a); break;
    case kExchangeUnpackSolve: exchange_unpack_solve<<<grid_solve, 256, 0, ctx->stream>>>(a); break;
  }
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

}  // namespace cxk_host
