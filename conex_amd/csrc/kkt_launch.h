// What the translation units of the cxk_* path call in one another.  Every kernel is compiled in
// exactly one unit; a unit that needs a kernel it does not own goes through a host function of the owner:
//   kkt_cone_launch.hip  the per-cone stages (Schur, PrepareStep, eigenvalue query, TakeStep), each an exhaustive
//                        switch over Group::route (cone_route.h); route choice and grouping; the mailbox, the step tail
//   cone_linear.hip      the linear blocks' views, finalize stages and launches (what the arms of those switches call:
//   cone_soc.hip         the second-order cones'                                 cone_units.h declares it)
//   cone_quad.hip        the quadratic cones'
//   cone_lmi.hip         the matrix inequalities', and the list of LMI kernel instances with its choosers
//   kkt_tree_launch.hip  assembly gather, right-hand sides, the elimination-tree sweeps, the exchange kernels
//   kkt_shard.hip        sharded sweeps, collectives, communicator and exchange entry points
//   kkt_qr.hip           the host QR mode
//   kkt_solve_block.hip  the block of right-hand sides on the stored factor (cxk_solve_block) and its kernels
//   kkt_context.hip      everything else of the C-ABI (no kernel launch of its own)
#pragma once
#include "kkt_internal.h"

namespace cxk {
struct MuRuleArgs;  // cone_types.h
}

namespace cxk_host {

enum { kOpSum = 0, kOpMax = 1, kOpMin = 2 };  // ShardAllReduce, cxk_allreduce_fn

constexpr int kSparseCParts = 64;  // slices of the <w,c>, <c,Qc> sums of a dense C beyond LDS orders


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

// Raises the dynamic-LDS limit of kernels that may be launched with more than the default 64 KB.
CXK_LOCAL inline hipError_t RaiseDynamicLds(std::initializer_list<const void*> kernels) {
  for (const void* k : kernels) {
    hipFuncAttributes attr;
    hipError_t e = hipFuncGetAttributes(&attr, k);
    if (e != hipSuccess) return e;
    // static + dynamic LDS must stay within the 160 KB of a CU
    const int dyn = std::min((int)kLdsLimit, 160 * 1024 - (int)attr.sharedSizeBytes);
    e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// (The thresholds of the automatic modes -- kLinearLdsMaxVars, kTiledLinearMinWork, kSparseLinear*, kSparseSoc*,
// kQuadStreamMinWork -- and the rules LinearSparsePays / SocSparsePays are cone_route.h's, with the choice they feed.)

// The environment switches of cxk_finalize, read once per call (FinalizeImpl).
struct FinalizeSwitches {
  // the modes of the routes as the environment has them (CXK_SPARSE_LMI, CXK_STREAMED_CONES, CXK_TILED_LINEAR,
  // CXK_STREAMED_QUADRATIC, CXK_SPARSE_LINEAR, CXK_SPARSE_SOC and their _MIN_WORK / _MIN_RATIO: cone_route.h); what the
  // context was told by a cxk_set_* goes in front (GroupConstraints)
  RouteModes modes;
  bool quirks_off = false;      // CXK_REFERENCE_QUIRKS=0: the two corrections instead of the reference as written
  int chain_segments = -1;      // CXK_CHAIN_SEGMENTS: 0 keeps the reference's order, P asks for P segments
  int gemm_min_n = 9;           // CXK_GEMM_MIN_N: smallest LDS-resident order on the batched-GEMM assembly
  bool schur_generic = false;   // CXK_LMI_SCHUR=generic: the LDS-resident literal kernel (comparison runs, tests)
  bool no_herm_fold = false;    // CXK_NO_HERM_FOLD
  bool no_packed_slack = false; // CXK_NO_PACKED_SLACK
  int gram_splits = 0;          // CXK_GRAM_SPLITS: K splits of the GEMM assembly (0: chosen by shape)
  int soc_stream_stages = 0;    // CXK_SOC_STREAM_STAGES=1 / 2: their assembly stops after that stage (timing runs: wrong results)
  int quad_csr_lanes = 0;       // CXK_QUAD_CSR_LANES=1 / 8 / 64: lanes per row of a structured quadratic cone's S (0: QuadCsrLanes)
  int wide_spectrum = -1;     // CXK_WIDE_SPECTRUM: -1 large-order LMI groups beyond the one-workgroup Lanczos run, 0 never, 1 all
  int wide_reduce_min_order = -1;    // CXK_WIDE_REDUCE_MIN_ORDER instead of kWideReduceMinOrder (kernels_lmi_wide.hip.h; tests)
};

// ---- kkt_context.hip
int GridFor(size_t work, int block);
int CheckReady(cxk_context* ctx);
int FlushDeferred(cxk_context* ctx, bool keep_scalars = false, bool keep_y = false);

// ---- kkt_cone_launch.hip (LmiLargeSpectrumMaxOrder: cone_lmi.hip)
CXK_LOCAL hipError_t RaiseConeLdsLimits();
// the largest order whose one-workgroup Lanczos run (lmi_large_spectrum, LmiLargeSpectrumLds) fits kLdsLimit
CXK_LOCAL int LmiLargeSpectrumMaxOrder();
// cxk_set_wide_spectrum's word, else the environment's (kernels_lmi_wide.hip.h: the Lanczos run spread over the chip)
inline int WideSpectrumMode(const cxk_context* ctx, const FinalizeSwitches& sw) {
  return ctx->wide_spectrum != -2 ? ctx->wide_spectrum : sw.wide_spectrum;
}
CXK_LOCAL int GroupConstraints(cxk_context* ctx, const FinalizeSwitches& sw);     // finalize: constraints of one shape form a group
CXK_LOCAL int UploadGroup(cxk_context* ctx, Group& g, const FinalizeSwitches& sw);  // finalize: one group's data and work space
bool ClockSample(cxk_context* ctx, int slot, hipEvent_t* e0, hipEvent_t* e1);
CXK_LOCAL int LaunchSetIdentity(cxk_context* ctx);
int LaunchSchur(cxk_context* ctx);
// the bounds of every linear constraint on the line search's step (y0 = ctx->y2, y1 = ctx->y) into info2
CXK_LOCAL int LaunchLinearLineSearch(cxk_context* ctx, double dinf_upper_bound, double c_scaling);
int FlushDirection(cxk_context* ctx);
CXK_LOCAL bool StepTailOk(const cxk_context* ctx, int affine);
CXK_LOCAL int PrepareStepImpl(cxk_context* ctx, int affine, double c_weight, double e_weight, double* info, bool take, int* took,
                    const double* cw_from = nullptr, double cw_scale = 1.0);
CXK_LOCAL int LaunchTakeStep(cxk_context* ctx, double e_weight, double step_size, const double* step_from, bool skip_on_fail = false);
CXK_LOCAL int SlackEigenvaluesImpl(cxk_context* ctx, double c_weight, double* out, const MuRuleArgs* rule);
// the eigenvalue query with the selection of the barrier parameter (into ctx->mu_dev) in its launch; nobody waits
CXK_LOCAL int SelectMuAsync(cxk_context* ctx, double c_weight, double divergence_upper_bound, int rank, double prev, double lb,
                            double ub);

// ---- kkt_tree_launch.hip
CXK_LOCAL hipError_t RaiseTreeLdsLimits();
int LaunchGather(cxk_context* ctx, bool with_rhs, double k, double bs, double cs);
int LaunchSweep(cxk_context* ctx, int lb, int le, int mode, bool then_backward, bool with_rhs);
int LaunchBackPair(cxk_context* ctx, const cxk_context::BackPair& bp);
int LaunchChain(cxk_context* ctx, int mode);
int LaunchTreeCore(cxk_context* ctx, int mode, bool with_rhs, bool backward);
int LaunchTree(cxk_context* ctx, int mode, bool with_rhs, bool backward);
int MakeFusedTreeArgs(cxk_context* ctx, FusedTreeArgs* out);
int DebugReportTimeout(cxk_context* ctx);
bool FusedTimedOut(const cxk_context* ctx);
int DisableFusedTree(cxk_context* ctx);
int RedoFactorSolveOnLevels(cxk_context* ctx);
int LaunchStepScalars(cxk_context* ctx);
// y <- k (bs b + cs AQc) - 2 AW (k from the device when k_from) / y <- cb b + cq AQc + cw AW; fail: the word to clear
CXK_LOCAL int LaunchBuildRhs(cxk_context* ctx, double k, double bs, double cs, int* fail, const double* k_from = nullptr);
CXK_LOCAL int LaunchBuildRhsComb(cxk_context* ctx, double cb, double cq, double cw, int* fail);
CXK_LOCAL int LaunchMaskedCopy(cxk_context* ctx, int n, const double* in, double* out);       // counted variables, zeros elsewhere
CXK_LOCAL int LaunchMaskedCopyPairs(cxk_context* ctx, int K, const double* in, double* out);  // owned constraints' pairs
CXK_LOCAL int LaunchCopyDoubles(cxk_context* ctx, int n, const double* src, double* dst);
enum ExchangeKernel { kExchangePack, kExchangeUnpack, kExchangeUnpackMatrix, kExchangePackSolve, kExchangeUnpackSolve };
// (right-hand side cb b + cq AQc + cw AW)
CXK_LOCAL int LaunchExchange(cxk_context* ctx, ExchangeKernel which, double cb, double cq, double cw);

// ---- kkt_shard.hip
int ShardAllReduce(cxk_context* ctx, double* buf, size_t count, int op);
long ExchangeCount(const cxk_context* ctx);
int ShardedTree(cxk_context* ctx, int mode, bool with_rhs, bool backward);
int ResolveShardTimeout(cxk_context* ctx);
int SettleBeforeUnmarked(cxk_context* ctx);

// ---- kkt_qr.hip
int QrFactor(cxk_context* ctx);
int QrSolve(cxk_context* ctx);

}  // namespace cxk_host

extern "C" {  // kkt_cone_launch.hip
int SyncMailbox(cxk_context* ctx);  // waits until everything enqueued so far has run and the mailbox carries its results
bool TakeStepFromDeviceOk(const cxk_context* ctx);
}

#define CXK_ENTER_KEEP(ctx)                     \
  if (CheckReady(ctx)) return CXK_FAILURE;      \
  (ctx)->calls++;                               \
  DeviceGuard cxk_device_guard_((ctx)->device); \
  if (ResolveShardTimeout(ctx)) return CXK_FAILURE
#define CXK_ENTER(ctx)   \
  CXK_ENTER_KEEP(ctx);   \
  if (FlushDeferred(ctx)) return CXK_FAILURE
