// Sharded contexts (world > 1): the collectives, the sweeps around the exchange of the replicated top, what a
// time-out of a whole-tree launch means across ranks, the RCCL communicator and the exchange entry points.
// Owns comm_selftest_fill; the exchange kernels are kkt_tree_launch.hip's (LaunchExchange).
#include "kkt_launch.h"

namespace cxk_host {

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

// One sweep of a sharded context.  Bottom-up over this rank's subtrees (mode 0 factor [+ forward
// substitution when with_rhs], mode 1 forward substitution), ONE sum all-reduce of what the
// subtrees contribute to the replicated top of the tree --
//   mode 0: [top slab entries | AW_T | AQc_T | forward values | <w,c> <c,Qc> | failure flag | time-out count]
//           (supernodal_assembler.cc:103-111,162-164 and block_triangular_operations.cc:209-215 are
//            the sums that cross ranks here),
//   mode 1: [forward values | time-out mark]  --
// then the top on every rank (bit-identical: same data, same kernels) and, when `backward`, the
// back-substitution down this rank's subtrees.
int ShardedTree(cxk_context* ctx, int mode, bool with_rhs, bool backward) {
  if (mode == 0 && with_rhs && backward && ctx->fused_tree && ctx->fused_shard && ctx->asm_pending.on &&
      ctx->asm_pending.with_rhs != 0)
    return LaunchFusedShard(ctx);
  if (ctx->use_ldlt && mode == 0) CXK_TRY(hipMemsetAsync(ctx->d_reg.p, 0, sizeof(int), ctx->stream));
  const int cut = ctx->cut_level;
  const bool rhs = with_rhs || mode != 0;
  for (int l = 0; l < cut; l++)
    if (LaunchSweep(ctx, l, l + 1, mode, false, rhs)) return CXK_FAILURE;
  const double* c = ctx->rhs_c;
  if (mode == 0) {
    if (LaunchExchange(ctx, kExchangePack, c[0], c[1], c[2])) return CXK_FAILURE;
    if (ShardAllReduce(ctx, ctx->xbuf.p, (size_t)ExchangeCount(ctx), kOpSum)) return CXK_FAILURE;
    if (LaunchExchange(ctx, with_rhs ? kExchangeUnpack : kExchangeUnpackMatrix, c[0], c[1], c[2])) return CXK_FAILURE;
  } else if (ctx->n_xv > 0) {
    if (LaunchExchange(ctx, kExchangePackSolve, c[0], c[1], c[2])) return CXK_FAILURE;
    if (ShardAllReduce(ctx, ctx->xbuf.p, (size_t)ctx->n_xv + 1, kOpSum)) return CXK_FAILURE;
    if (LaunchExchange(ctx, kExchangeUnpackSolve, c[0], c[1], c[2])) return CXK_FAILURE;
  }
  return ShardedTop(ctx, mode, rhs, backward);
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
  CXK_TRY(hipMemsetAsync(ctx->d_fail.p, 0, 3 * sizeof(int), ctx->stream));  // (the time-out mark with them)
  if (LaunchBuildRhsComb(ctx, ctx->rhs_c[0], ctx->rhs_c[1], ctx->rhs_c[2], nullptr)) return CXK_FAILURE;
  for (int l = 0; l < ctx->cut_level; l++)
    if (LaunchSweep(ctx, l, l + 1, 1, false, true)) return CXK_FAILURE;
  if (LaunchExchange(ctx, kExchangeUnpack, ctx->rhs_c[0], ctx->rhs_c[1], ctx->rhs_c[2])) return CXK_FAILURE;
  return ShardedTop(ctx, 0, true, true);
}

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

}  // namespace cxk_host

extern "C" {

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

int cxk_exchange_buffer(cxk_context* ctx, void** dev_ptr, long* count) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->world > 1, "exchange buffer exists only for sharded contexts");
  *dev_ptr = ctx->xbuf.p;
  *count = ExchangeCount(ctx);
  return CXK_SUCCESS;
}

// host copies of the exchange buffer (tests; a real run all-reduces the device buffer in place)
int cxk_exchange_download(cxk_context* ctx, double* out) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->world > 1, "exchange buffer exists only for sharded contexts");
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(out, ctx->xbuf.p, sizeof(double) * (size_t)ExchangeCount(ctx),
                    hipMemcpyDeviceToHost));
  return CXK_SUCCESS;
}
int cxk_exchange_upload(cxk_context* ctx, const double* in) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->world > 1, "exchange buffer exists only for sharded contexts");
  CXK_TRY(hipStreamSynchronize(ctx->stream));
  CXK_TRY(hipMemcpy(ctx->xbuf.p, in, sizeof(double) * (size_t)ExchangeCount(ctx),
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
  if (LaunchExchange(ctx, kExchangePack, k * bs, k * cs, -2.0)) return CXK_FAILURE;
  ctx->factor_seq = ++ctx->seq;
  return CXK_SUCCESS;
}

// Part 2, after the caller has sum-reduced the exchange buffer across ranks: unpack the
// completed top, factor/solve it (replicated), back-substitute the own subtrees.
int cxk_kkt_finish_async(cxk_context* ctx, double k, double bs, double cs) {
  CXK_ENTER(ctx);
  CXK_DEMAND(ctx->world > 1, "cxk_kkt_finish_async needs cxk_set_shard(world > 1)");
  if (LaunchExchange(ctx, kExchangeUnpack, k * bs, k * cs, -2.0)) return CXK_FAILURE;
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

}  // extern "C"
