// What the translation units of the cxk_* path call in one another.  Every kernel is compiled in
// exactly one unit; a unit that needs a kernel it does not own goes through a host function of the owner:
//   kkt_cone_launch.hip  the per-cone stages (Schur, PrepareStep, eigenvalue query, TakeStep), the mailbox
//   kkt_tree_launch.hip  assembly gather, right-hand sides, the elimination-tree sweeps, the exchange kernels
//   kkt_shard.hip        sharded sweeps, collectives, communicator and exchange entry points
//   kkt_qr.hip           the host QR mode
//   kkt_solve_block.hip  the block of right-hand sides on the stored factor (cxk_solve_block) and its kernels
//   kkt_context.hip      everything else of the C-ABI (no kernel launch of its own)
#pragma once
#include "kkt_internal.h"

namespace cxk {
struct MuRuleArgs;  // kernels_cone.hip.h
}

namespace cxk_host {

enum { kOpSum = 0, kOpMax = 1, kOpMin = 2 };  // ShardAllReduce, cxk_allreduce_fn

constexpr int kSparseCParts = 64;  // slices of the <w,c>, <c,Qc> sums of a dense C beyond LDS orders

// A function only the units of the cxk_* path call in one another: not part of the library's dynamic symbols.
#define CXK_LOCAL __attribute__((visibility("hidden")))

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

// The widest linear block the LDS route can run: linear_line_search is launched with 16 m bytes of dynamic LDS
// and has the default limit of 64 KB (linear_prepare's 8 m bytes reach it at 8192).
constexpr int kLinearLdsMaxVars = 4096;
// Automatic mode sends a linear block of rows x m to the tiled route from rows m^2 >= this on.  Measured
// (tools/linear_tiled_speed.py against the build before the tiled route): twice the smallest
// rows m^2 among the measured shapes from which assembly, PrepareStep and the eigenvalue query are each faster on
// the tiled route at that shape and at every larger one, 2000 x 64 (at 256 x 32 the assembly is five times faster
// but the two-launch PrepareStep and query cost 2 us more); twice, because the numbers are one box's on one day.
constexpr long long kTiledLinearMinWork = 2ll * 2000 * 64 * 64;  // 16 384 000

// Automatic mode (cxk_set_sparse_linear(ctx, -1)) sends a linear block to the sparse route when
// R sum_r nnz_r^2 <= rows m^2: the sparse assembly forms about sum_r nnz_r^2 products one fma at a time, the dense
// routes rows m^2 on the matrix pipe.  Measured (tools/linear_sparse_speed.py against the build before the sparse
// route on its own choice): R is twice the smallest rows m^2 / sum_r nnz_r^2 among the measured
// shapes at which assembly, PrepareStep and the eigenvalue query are each faster on the sparse route, 3.9 at the
// half-full 2000 x 64; twice, because the numbers are one box's on one day.  A fully dense block (ratio 1) never moves.
// CXK_SPARSE_LINEAR_MIN_RATIO moves R for comparison runs.  Two more conditions, both from shapes that lost:
//  - a column's rows are one wavefront's dependent chain, 0.33 us per row (100 000 x 50 with one full column: 32.6 ms
//    against 0.38 ms): no column longer than kSparseLinearMaxColumn, twice the longest measured to win (about 1050);
//  - a thousand 20 x 10 blocks with 3 nonzeros per row are 20 % slower at every stage than on the LDS route's one
//    launch per stage: nothing below the rows m^2 of the smallest measured shape that won, 2000 x 64, moves.
constexpr double kSparseLinearMinRatio = 7.8;
constexpr int kSparseLinearMaxColumn = 2048;
constexpr long long kSparseLinearMinWork = 2000ll * 64 * 64;  // 8 192 000
inline bool LinearSparsePays(double rows, double m, double sum_nnz_sq, int longest_column, double ratio) {
  return ratio * sum_nnz_sq <= rows * m * m && rows * m * m >= (double)kSparseLinearMinWork &&
         longest_column <= kSparseLinearMaxColumn;
}

// Automatic mode (cxk_set_sparse_soc(ctx, -1)) sends a second-order cone of dimension len = n + 1 over m variables to
// the sparse route when it can run nowhere else (added by cxk_add_soc_csr, or len m beyond the int range), or when
// R nnz <= len m and len m^2 >= kSparseSocMinWork: the sparse assembly reads the nnz nonzeros and moves the m x m
// square twice, the dense routes stream len m entries (and the streamed one multiplies len m^2).  Measured
// (tools/soc_sparse_speed.py --sweep against the streamed route): each constant is twice the smallest
// value among the swept shapes at which assembly + query + PrepareStep + TakeStep are faster on the sparse route;
// twice, because the numbers are one box's on one day.  The smallest winning len m / nnz is 2.02 (2048 x 64 half full:
// 87.8 us against 129.7 us; the assembly gains 4.3x, the one-thread-per-row slack loses 0.63x); a fully dense 401 x 61
// loses (87.6 us against 82.7 us) and never moves.  The smallest swept shape, 401 x 61 (len m^2 = 1 492 121), wins at
// 3 nonzeros per row (51.4 us against 79.7 us); nothing smaller was measured, so nothing smaller moves.
// CXK_SPARSE_SOC_MIN_RATIO moves R for comparison runs.  No default anywhere asks for this mode.
constexpr double kSparseSocMinRatio = 4.04;
constexpr long long kSparseSocMinWork = 2ll * 401 * 61 * 61;  // 2 984 242
inline bool SocSparsePays(double len, double m, double nnz, double ratio) {
  return ratio * nnz <= len * m && len * m * m >= (double)kSparseSocMinWork;
}

// Automatic mode (cxk_set_streamed_quadratic(ctx, -1)) sends a quadratic cone to the streamed route from this many
// doubles streamed per pass, (Q ? n n : 0) + (n + 1) m, on.  Measured (tools/quad_stream_speed.py):
// the smallest shape of the sweep, n = 32 with Q over m = 8 (32 * 32 + 33 * 8), where assembly + PrepareStep +
// TakeStep already take 48 us on the streamed route against 333 us on the LDS route; every larger swept shape gains
// more.  Nothing smaller was measured, so nothing smaller moves (the cones of a handful of doubles stay where they are).
constexpr long long kQuadStreamMinWork = 32 * 32 + 33 * 8;  // 1288

// The environment switches of cxk_finalize, read once per call (FinalizeImpl).
struct FinalizeSwitches {
  bool quirks_off = false;      // CXK_REFERENCE_QUIRKS=0: the two corrections instead of the reference as written
  int chain_segments = -1;      // CXK_CHAIN_SEGMENTS: 0 keeps the reference's order, P asks for P segments
  int sparse_lmi = -1;          // CXK_SPARSE_LMI=0 / 1 forces sparse evaluation never / always (tests)
  int gemm_min_n = 9;           // CXK_GEMM_MIN_N: smallest LDS-resident order on the batched-GEMM assembly
  bool schur_generic = false;   // CXK_LMI_SCHUR=generic: the LDS-resident literal kernel (comparison runs, tests)
  bool no_herm_fold = false;    // CXK_NO_HERM_FOLD
  bool no_packed_slack = false; // CXK_NO_PACKED_SLACK
  int gram_splits = 0;          // CXK_GRAM_SPLITS: K splits of the GEMM assembly (0: chosen by shape)
  bool streamed_cones = false;  // CXK_STREAMED_CONES=1: second-order cones beyond LDS run from HBM (cxk_set_streamed_cones)
  int soc_stream_stages = 0;    // CXK_SOC_STREAM_STAGES=1 / 2: their assembly stops after that stage (timing runs: wrong results)
  int tiled_linear = -1;        // CXK_TILED_LINEAR=0 / 1: linear blocks never / always on the tiled route (cxk_set_tiled_linear)
  long long tiled_linear_min_work = kTiledLinearMinWork;  // CXK_TILED_LINEAR_MIN_WORK (comparison runs)
  int streamed_quadratic = 0;   // CXK_STREAMED_QUADRATIC=0 / 1: quadratic cones never / always held in HBM (cxk_set_streamed_quadratic)
  long long streamed_quadratic_min_work = kQuadStreamMinWork;  // CXK_STREAMED_QUADRATIC_MIN_WORK (comparison runs)
  int sparse_linear = 0;        // CXK_SPARSE_LINEAR=0 / 1: linear blocks never / always on the sparse route (cxk_set_sparse_linear)
  double sparse_linear_min_ratio = kSparseLinearMinRatio;  // CXK_SPARSE_LINEAR_MIN_RATIO (comparison runs)
  int sparse_soc = 0;           // CXK_SPARSE_SOC=0 / 1: second-order cones never / always on the sparse route (cxk_set_sparse_soc)
  double sparse_soc_min_ratio = kSparseSocMinRatio;  // CXK_SPARSE_SOC_MIN_RATIO (comparison runs)
};

// ---- kkt_context.hip
int GridFor(size_t work, int block);
int CheckReady(cxk_context* ctx);
int FlushDeferred(cxk_context* ctx, bool keep_scalars = false, bool keep_y = false);

// ---- kkt_cone_launch.hip
CXK_LOCAL hipError_t RaiseConeLdsLimits();
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
