// The per-cone stages of the cxk_* path: Schur complement, PrepareStep, eigenvalue query, TakeStep, each an exhaustive
// switch over Group::route whose arms call the unit that owns the route's kernels (cone_units.h); route choice and
// grouping, the shared front of the per-group stage of cxk_finalize, the kernel clocks, the host mailbox and the step
// tail.  Owns the kernels of kernels_stage and kernels_oct (and mailbox_pack, newton_from_three below): the two tiny
// routes kStatic and kOct are launched from here.
#include "cone_units.h"
#include "kernels_oct.hip.h"
#include "kernels_stage.hip.h"

namespace cxk_host {

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
  const size_t a_blk = a_sz + (g.lmi.assembly != LmiAssembly::kGeneric ? c_sz : 0);
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

// Kernels of the cone units that may be launched with more than the default 64 KB of dynamic LDS.
hipError_t RaiseConeLdsLimits() {
  static PerDeviceOnce once;  // function attributes are per device: every device a context is built on
  return once.run([] {
    hipError_t e = RaiseLmiLdsLimits();
    if (e == hipSuccess) e = RaiseSocLdsLimits();
    if (e == hipSuccess) e = RaiseQuadLdsLimits();
    return e;
  });
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

// The kernel clocks (StepClock, AssemblyClock: cone_units.h).
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

// The routes of more than one launch, and both quadratic ones (tools/quad_stream_speed.py compares them), carry the
// assembly clock when timing is on; a dense LMI group takes its own (lmi_schur_mfma carries the pair on its dispatch).
int LaunchSchur(cxk_context* ctx) {
  Arena ar = MakeArena(ctx);
  hipStream_t st = ctx->stream;
  for (Group& g : ctx->groups) {
    const int count = (int)g.ids.size();
    if (count == 0) continue;
    switch (g.route) {
      case ConeRoute::kLmiDense: if (LaunchLmiDenseSchur(ctx, g, ar)) return CXK_FAILURE; break;
      case ConeRoute::kLmiSparse: { const AssemblyClock clock(ctx); if (LaunchLmiSparseSchur(ctx, g, ar)) return CXK_FAILURE; break; }
      case ConeRoute::kLmiFactored: { const AssemblyClock clock(ctx); if (LaunchLmiFactoredSchur(ctx, g, ar)) return CXK_FAILURE; break; }
      case ConeRoute::kLinearLds: LaunchLinearLdsSchur(g, ar, st); break;
      case ConeRoute::kLinearTiled: { const AssemblyClock clock(ctx); CXK_TRY(LaunchLinearTiledSchur(g, ar, st)); break; }
      case ConeRoute::kLinearSparse: { const AssemblyClock clock(ctx); CXK_TRY(LaunchLinearSparseSchur(g, ar, st)); break; }
      case ConeRoute::kSocLds: LaunchSocLdsSchur(ctx, g, ar); break;
      case ConeRoute::kSocStreamed: { const AssemblyClock clock(ctx); CXK_TRY(LaunchSocStreamSchur(g, ar, st)); break; }
      case ConeRoute::kSocSparse: { const AssemblyClock clock(ctx); CXK_TRY(LaunchSocSparseSchur(g, ar, st)); break; }
      case ConeRoute::kQuadLds: { const AssemblyClock clock(ctx); LaunchQuadLdsSchur(g, ar, st); break; }
      case ConeRoute::kQuadStreamed: { const AssemblyClock clock(ctx); CXK_TRY(LaunchQuadStreamSchur(g, ar, st)); break; }
      case ConeRoute::kStatic: static_schur<<<count, 64, 0, st>>>(MakeStatic(g), ar); break;
      case ConeRoute::kOct: oct_schur<<<count, 64, 0, st>>>(MakeOct(g), ar); break;
    }
  }
  CXK_TRY(hipGetLastError());
  return CXK_SUCCESS;
}

// The nonzero statistics Choose asks for, of a dense-added linear block (rows = n) or second-order cone (rows = n + 1)
// whose sparse mode is not 0; and the nonzeros themselves (LinearNonzeros) when ints can point at them.
static void MeasureNonzeros(ConstraintRec* c, ConeShape* s) {
  if (c->rows.ptr.empty()) {
    size_t nnz = 0;
    for (double v : c->A) nnz += v != 0.0;
    s->nnz = (double)nnz;
    s->nnz_fits_int = nnz <= (size_t)INT_MAX;
    if (!s->nnz_fits_int) return;
    LinearNonzeros(c);
  }
  s->nnz = (double)c->rows.col.size();
  for (size_t r = 0; r + 1 < c->rows.ptr.size(); r++) {
    const double nz = c->rows.ptr[r + 1] - c->rows.ptr[r];
    s->sum_nnz_sq += nz * nz;
  }
  std::vector<int> per_col((size_t)c->m, 0);
  for (int v : c->rows.col) per_col[(size_t)v]++;
  s->longest_column = c->m ? *std::max_element(per_col.begin(), per_col.end()) : 0;
}

// cxk_finalize, per-group stages.  Every owned constraint gets its route (cone_route.h: Choose, or the refusal
// cxk_finalize fails with); constraints of one shape on one route form a group, numbered by first appearance.
int GroupConstraints(cxk_context* ctx, const FinalizeSwitches& sw) {
  const int K = (int)ctx->cons.size();
  std::map<std::tuple<int, int, int, int, ConeRoute, bool, bool, int, bool, bool, int, int, bool>, int> gmap;
  ctx->groups.clear();
  ctx->sparse_soc_setup_ms = 0;
  // what the context was told (-1 / -2: nothing) goes in front of the environment's word
  RouteModes modes = sw.modes;
  if (ctx->streamed_cones >= 0) modes.streamed_cones = ctx->streamed_cones != 0;
  if (ctx->tiled_linear >= 0) modes.tiled_linear = ctx->tiled_linear;
  if (ctx->streamed_quadratic != -2) modes.streamed_quadratic = ctx->streamed_quadratic;
  if (ctx->sparse_linear != -2) modes.sparse_linear = ctx->sparse_linear;
  if (ctx->sparse_soc != -2) modes.sparse_soc = ctx->sparse_soc;
  if (ctx->sparse_affine != -2) modes.sparse_affine = ctx->sparse_affine;
  if (ctx->sparse_fold != -2) modes.sparse_fold = ctx->sparse_fold;
  for (int i = 0; i < K; i++) {
    ConstraintRec& c = ctx->cons[i];
    c.route = ConeRoute::kStatic;
    c.entries.sparse_affine = false;
    c.entries.fold = false;
    if (!ctx->owned[i]) continue;
    ConeShape s{c.type, c.n, c.m, c.herm_d, c.symmetric, c.csr_only, c.factors.given,
                c.type == CXK_QUAD && (!c.Q.empty() || c.sq.given)};
    s.q_structured = c.sq.given;
    s.q_nnz = (double)c.sq.col.size();
    s.q_rank = c.sq.rank;
    if (c.type == CXK_QUAD && c.csr_only) s.nnz = (double)c.rows.col.size();
    const int sparse_mode = c.type == CXK_LINEAR ? modes.sparse_linear : c.type == CXK_SOC ? modes.sparse_soc : 0;
    if (sparse_mode != 0 && !c.csr_only) MeasureNonzeros(&c, &s);
    if (c.type == CXK_LMI && !c.factors.given) MeasureLmi(c, &s);
    const RouteChoice choice = Choose(s, modes);
    CXK_DEMAND(!choice.refusal, choice.refusal);
    c.route = choice.route;
    const bool literal = c.type == CXK_LMI && !c.symmetric;
    const int f_R = c.factors.given ? c.factors.R : 0;
    // (nobody said: the default of the entry point the constraint came through; a group mixes no modes)
    if (c.route == ConeRoute::kLmiSparse)
      c.entries.sparse_affine = LmiTakesSparseAffine(c, modes.sparse_affine != -2 ? modes.sparse_affine : c.entries.affine_default,
                                             modes.sparse_affine_min_ratio);
    // (likewise the folded sums of a Hermitian constraint over C or H: the real one, d = 1, has nothing to fold)
    if (c.route == ConeRoute::kLmiSparse && c.herm_d > 1)
      c.entries.fold = (modes.sparse_fold != -2 ? modes.sparse_fold : c.entries.fold_default) != 0;
    // the form of a quadratic cone's Q: 0 dense or none (has_q), else structured with (2) or without (1) a sparse part,
    // and the rank; the nonzero counts of the members may differ
    const int q_form = c.sq.given ? (c.sq.ptr.empty() ? 1 : 2) : 0;
    // the form of a quadratic cone's A: dense, or its nonzeros (cxk_add_quadratic_csr); the patterns of the members may differ
    const bool a_csr = c.type == CXK_QUAD && c.csr_only;
    const auto key = std::make_tuple(c.type, c.n, c.m, c.herm_d, c.route, literal, s.has_q, f_R, c.entries.sparse_affine, c.entries.fold,
                                     q_form, c.sq.rank, a_csr);
    auto it = gmap.find(key);
    if (it == gmap.end()) {
      it = gmap.emplace(key, (int)ctx->groups.size()).first;
      Group& g = ctx->groups.emplace_back();
      g.type = c.type;
      g.n = c.n;
      g.m = c.m;
      g.herm_d = c.herm_d;
      g.route = c.route;
      // the rest of the key: the one place outside a family's unit that writes its state (cone_state.h)
      g.lmi.literal = literal;
      g.quad.has_q = s.has_q;
      g.quad.sq.on = c.sq.given;
      g.quad.sq.has_s = q_form == 2;
      g.quad.sq.rank = c.sq.rank;
      g.quad.sa.on = a_csr;
      g.lmi.f.R = f_R;
      g.lmi.sa.on = c.entries.sparse_affine;
      g.lmi.sp.fold = c.entries.fold;
    }
    c.group = it->second;
    c.member = (int)ctx->groups[it->second].ids.size();
    ctx->groups[it->second].ids.push_back(i);
  }
  return CXK_SUCCESS;
}

// The device copy of one group's data in the layout its kernels read, and its work space: what every route shares,
// then the route's own stage (in its family's unit, each beside the view of what it allocates).
int UploadGroup(cxk_context* ctx, Group& g, const FinalizeSwitches& sw) {
  const size_t cnt = g.ids.size();
  const GroupSizes sz = SizesOf(g);
  if (g.type == CXK_LMI && PlanLmiGroup(ctx, g, sw)) return CXK_FAILURE;
  // the routes that hold their data as nonzeros or factors keep no dense copy of A on the device
  const bool dense_a = g.route != ConeRoute::kLmiSparse && g.route != ConeRoute::kLmiFactored &&
                       g.route != ConeRoute::kLinearSparse && g.route != ConeRoute::kSocSparse && !g.quad.sa.on;
  if (UploadDenseData(ctx, g, dense_a ? sz.a : 0, sz.c)) return CXK_FAILURE;
  CXK_TRY(g.W.alloc(sz.w * cnt));
  CXK_TRY(g.T1.alloc(sz.w * cnt));
  if (AllocLinearT2(ctx, g)) return CXK_FAILURE;
  CXK_TRY(g.dids.upload(g.ids));
  switch (g.route) {
    case ConeRoute::kLinearLds: case ConeRoute::kSocLds: case ConeRoute::kStatic: case ConeRoute::kOct:
      return CXK_SUCCESS;  // (the dense copy is all their kernels read)
    case ConeRoute::kLinearTiled: return UploadLinearTiled(ctx, g, sw);
    case ConeRoute::kLinearSparse: return UploadLinearSparse(ctx, g);
    case ConeRoute::kSocStreamed: return UploadSocStream(ctx, g, sw);
    case ConeRoute::kSocSparse: return UploadSocSparse(ctx, g);
    case ConeRoute::kQuadLds: return UploadQuadGram(ctx, g);
    case ConeRoute::kQuadStreamed:
      if (g.quad.sa.on && UploadQuadSparseA(ctx, g)) return CXK_FAILURE;  // (the nonzeros of A first: the constants read them)
      return g.quad.sq.on ? UploadQuadStructured(ctx, g, sw) : UploadQuadStream(ctx, g, sw);
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
        LaunchLmiSetIdentity(g, ctx->stream);
        break;
      case ConeRoute::kLinearLds: case ConeRoute::kLinearTiled: case ConeRoute::kLinearSparse:
        LaunchVecSetIdentity(g, false, ctx->stream);
        break;
      case ConeRoute::kSocLds: case ConeRoute::kSocStreamed: case ConeRoute::kSocSparse:
      case ConeRoute::kQuadLds: case ConeRoute::kQuadStreamed:
        LaunchVecSetIdentity(g, true, ctx->stream);
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
    if (g.ids.empty()) continue;
    switch (g.route) {
      case ConeRoute::kLinearLds: case ConeRoute::kLinearTiled: case ConeRoute::kLinearSparse:
        if (LaunchLinearGroupLineSearch(ctx, g, a)) return CXK_FAILURE;
        break;
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
    if (g.type == CXK_LMI && g.lmi.large && !g.ids.empty()) return false;  // its step argument kernel takes the value
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
  // brings all partial results to every rank, which combines them in rank order (kernels_stage.hip.h:
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
  return only && only->type == CXK_LMI && !only->lmi.large && !only->lmi.literal && only->ids.size() == ctx->cons.size() &&
         LmiRowsServePrepare(*only);
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

// PrepareStep (mode 0; pmode 0, or 2 for the affine update) or the eigenvalue query (mode 1; pmode 1) of every
// group.  tail_blocks: what the tail workgroup adds to the grid of lmi_prepare_rows.
int LaunchPrepareGroups(cxk_context* ctx, int mode, int pmode, const StepArgs& sa, const StepTail& tail, int tail_blocks, int clock_slot) {
  bool rows_only = NonEmptyGroups(ctx) == 1;
  for (const Group& g : ctx->groups)
    if (!g.ids.empty())
      rows_only = rows_only && g.type == CXK_LMI && LmiPrepareOnRows(ctx, g, pmode);
  const StepClock clk = BeginStepClock(ctx, clock_slot, rows_only);
  for (Group& g : ctx->groups) {
    const int cnt = (int)g.ids.size();
    if (cnt == 0) continue;
    switch (g.route) {
      case ConeRoute::kLmiDense: case ConeRoute::kLmiSparse: case ConeRoute::kLmiFactored:
        if (LaunchLmiPrepare(ctx, g, mode, pmode, sa, tail, tail_blocks, clk)) return CXK_FAILURE;
        break;
      case ConeRoute::kLinearLds: case ConeRoute::kLinearTiled: case ConeRoute::kLinearSparse:
        if (LaunchLinearPrepare(ctx, g, mode, sa)) return CXK_FAILURE;
        break;
      case ConeRoute::kSocLds: case ConeRoute::kSocStreamed: case ConeRoute::kSocSparse:
        if (LaunchSocPrepare(ctx, g, mode, sa)) return CXK_FAILURE;
        break;
      case ConeRoute::kQuadLds: case ConeRoute::kQuadStreamed:
        if (LaunchQuadPrepare(ctx, g, mode, sa)) return CXK_FAILURE;
        break;
      case ConeRoute::kStatic: break;  // (no cone: nothing to prepare)
      case ConeRoute::kOct:
        if (mode == 0)
          oct_prepare<0><<<cnt, 64, sizeof(double) * (size_t)g.m, ctx->stream>>>(MakeOct(g), sa);
        else
          oct_prepare<1><<<cnt, 64, sizeof(double) * (size_t)g.m, ctx->stream>>>(MakeOct(g), sa);
        break;
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
  if (LaunchPrepareGroups(ctx, 0, affine ? 2 : 0, sa, tail, tail.slots ? 1 + tail.ny : 0, CXK_CLOCK_PREPARE)) return CXK_FAILURE;
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
    if (!g.ids.empty()) rows_only = rows_only && g.type == CXK_LMI && LmiTakeOnRows(g);
  const StepClock clk = BeginStepClock(ctx, CXK_CLOCK_TAKE, rows_only);
  for (Group& g : ctx->groups) {
    const int cnt = (int)g.ids.size();
    if (cnt == 0) continue;
    switch (g.route) {
      case ConeRoute::kLmiDense: case ConeRoute::kLmiSparse: case ConeRoute::kLmiFactored:
        if (LaunchLmiTakeStep(ctx, g, sa, clk)) return CXK_FAILURE;
        break;
      case ConeRoute::kLinearLds: case ConeRoute::kLinearTiled: case ConeRoute::kLinearSparse:
        LaunchLinearTakeStep(g, sa, ctx->stream);
        break;
      case ConeRoute::kSocLds: case ConeRoute::kSocStreamed: case ConeRoute::kSocSparse:
        if (LaunchSocTakeStep(ctx, g, sa)) return CXK_FAILURE;
        break;
      case ConeRoute::kQuadLds: case ConeRoute::kQuadStreamed:
        if (LaunchQuadTakeStep(ctx, g, sa)) return CXK_FAILURE;
        break;
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
  if (LaunchPrepareGroups(ctx, 1, 1, sa, tail, tail.slots ? 1 : 0, CXK_CLOCK_QUERY)) return CXK_FAILURE;
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
