// cxk_solve_block / cxk_solve_block_device: Y <- K^-1 Y for a block of right-hand sides with the stored
// factor (kernels_solve_block.hip.h).  One gather launch, one launch per level up, one per level down, one
// scatter launch; the work buffers belong to this feature and grow with the widest block seen.
#include "kkt_launch.h"
#include "kernels_solve_block.hip.h"

namespace cxk_host {
namespace {

// Everything that makes the call impossible, named; a pending assembly / direction has been settled by CXK_ENTER.
int CheckSolveBlock(cxk_context* ctx, const double* Y, int ld, int nrhs) {
  CXK_DEMAND(Y != nullptr, "cxk_solve_block: null pointer for the block of right-hand sides");
  CXK_DEMAND(nrhs >= 1, "cxk_solve_block: nrhs must be at least 1");
  CXK_DEMAND(ld >= ctx->md.N, "cxk_solve_block: leading dimension ld is smaller than the system size N");
  // (rows are addressed by variable: with unused variables the N rows of a column would not hold every index)
  CXK_DEMAND(ctx->md.num_vars <= ctx->md.N,
             "cxk_solve_block: a program that leaves out a variable below the largest one it uses is not supported");
  CXK_DEMAND(ctx->solver_mode != 2, "cxk_solve_block: not available in QR solver mode (the factor lives on the host)");
  CXK_DEMAND(ctx->refine_iters <= 0,
             "cxk_solve_block: iterative refinement is on (cxk_set_iterative_refinement > 0); the block solve is the "
             "plain factor solve and would return unrefined columns");
  CXK_DEMAND(ctx->factor_seq >= 0, "cxk_solve_block: no factorization yet");
  // the outcome of the latest factorization, read once (as cxk_factor_status reads it)
  if (ctx->mb && ctx->mb_seen < ctx->factor_seq && SyncMailbox(ctx)) return CXK_FAILURE;
  CXK_DEMAND((!ctx->mb || ctx->mbv[10] == 0.0) && !FusedTimedOut(ctx),
             "cxk_solve_block: the latest factorization failed: there is no factor to solve with");
  return CXK_SUCCESS;
}

int EnsureBuffers(cxk_context* ctx, int chunks) {
  auto& sb = ctx->solve_block;
  const int N = ctx->md.N;
  if (sb.pinv.n != (size_t)N) {
    std::vector<int> pinv(ctx->md.permutation_inverse.begin(), ctx->md.permutation_inverse.begin() + N);
    CXK_TRY(sb.pinv.upload(pinv));
  }
  if (chunks <= sb.chunks) return CXK_SUCCESS;
  CXK_TRY(hipStreamSynchronize(ctx->stream));  // (an earlier block solve may still be using the smaller buffers)
  sb.chunks = 0;
  CXK_TRY(sb.xp.alloc((size_t)chunks * N * kSbW));
  // slots nobody publishes into are read as 0.0 (as FactorPlan::updb's)
  CXK_TRY(sb.slots.alloc((size_t)chunks * ctx->updb.n * kSbW, true));
  sb.chunks = chunks;
  return CXK_SUCCESS;
}

int SolveBlockOnDevice(cxk_context* ctx, double* Y, long long ld, int nrhs) {
  const int N = ctx->md.N, chunks = (nrhs + kSbW - 1) / kSbW;
  if (EnsureBuffers(ctx, chunks)) return CXK_FAILURE;
  auto& sb = ctx->solve_block;
  SolveBlockArgs a;
  a.P = ctx->plan;
  a.slab = ctx->slab.p;
  a.X = sb.xp.p;
  a.T = sb.slots.p;
  a.tr = ctx->use_ldlt ? ctx->d_tr.p : nullptr;
  a.N = N;
  a.slot_stride = (long long)ctx->updb.n * kSbW;
  const int gg = GridFor((size_t)chunks * N * kSbW, 256);
  solve_block_gather<<<gg, 256, 0, ctx->stream>>>(N, nrhs, chunks, sb.pinv.p, Y, ld, sb.xp.p);
  const int nlev = (int)ctx->level_ptr.size() - 1;
  for (int l = 0; l < nlev; l++) {
    const int cnt = ctx->level_ptr[l + 1] - ctx->level_ptr[l];
    if (cnt <= 0) continue;
    a.base = ctx->level_ptr[l];
    if (ctx->use_ldlt)
      solve_block_forward<true><<<dim3(cnt, chunks), kSbThreads, 0, ctx->stream>>>(a);
    else
      solve_block_forward<false><<<dim3(cnt, chunks), kSbThreads, 0, ctx->stream>>>(a);
  }
  for (int l = nlev - 1; l >= 0; l--) {
    const int cnt = ctx->level_ptr[l + 1] - ctx->level_ptr[l];
    if (cnt <= 0) continue;
    a.base = ctx->level_ptr[l];
    if (ctx->use_ldlt)
      solve_block_backward<true><<<dim3(cnt, chunks), kSbThreads, 0, ctx->stream>>>(a);
    else
      solve_block_backward<false><<<dim3(cnt, chunks), kSbThreads, 0, ctx->stream>>>(a);
  }
  solve_block_scatter<<<gg, 256, 0, ctx->stream>>>(N, nrhs, chunks, sb.pinv.p, sb.xp.p, ld, Y);
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

}  // namespace
}  // namespace cxk_host

static const char kShardedRefusal[] = "cxk_solve_block: sharded contexts (world > 1) are not supported";

int cxk_solve_block_chunk_width(void) { return cxk::kSbW; }

int cxk_solve_block_device(cxk_context* ctx, double* Y_dev, int ld, int nrhs) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(ctx->world <= 1, kShardedRefusal);  // (before anything a sharded context would answer with a collective)
  CXK_ENTER(ctx);
  if (CheckSolveBlock(ctx, Y_dev, ld, nrhs)) return CXK_FAILURE;
  return SolveBlockOnDevice(ctx, Y_dev, ld, nrhs);
}

int cxk_solve_block(cxk_context* ctx, double* Y_host, int ld, int nrhs) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(ctx->world <= 1, kShardedRefusal);  // (before anything a sharded context would answer with a collective)
  CXK_ENTER(ctx);
  if (CheckSolveBlock(ctx, Y_host, ld, nrhs)) return CXK_FAILURE;
  auto& sb = ctx->solve_block;
  const size_t N = (size_t)ctx->md.N;
  if (sb.stage.n < N * (size_t)nrhs) {
    CXK_TRY(hipStreamSynchronize(ctx->stream));
    CXK_TRY(sb.stage.alloc(N * (size_t)nrhs));
  }
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy2D(sb.stage.p, N * sizeof(double), Y_host, (size_t)ld * sizeof(double), N * sizeof(double), (size_t)nrhs,
                      hipMemcpyHostToDevice));
  if (SolveBlockOnDevice(ctx, sb.stage.p, (long long)N, nrhs)) return CXK_FAILURE;
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy2D(Y_host, (size_t)ld * sizeof(double), sb.stage.p, N * sizeof(double), N * sizeof(double), (size_t)nrhs,
                      hipMemcpyDeviceToHost));
  return CXK_SUCCESS;
}
