// cxk_* C-ABI: device-resident Newton-step KKT path (see include/conex_kkt_hip.h).
//
// Host side = structure + launches only.  All fp64 state (A_i, C, W, Schur blocks, the
// supernodal slab, right-hand sides) lives in HBM for the lifetime of the context; per
// Newton step only scalars cross PCIe.
#include "cone_units.h"  // what the counters ask the LMI unit (LmiAssemblyOf, LmiOnWideSpectrum)
#include "kernels_gemm.hip.h"  // GemmArgs, LaunchGemmSplitK (cxk_gemm_f64)

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

hipError_t RaiseLdsLimits() {
  const hipError_t e = RaiseConeLdsLimits();
  return e != hipSuccess ? e : RaiseTreeLdsLimits();
}

int CheckReady(cxk_context* ctx) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(ctx->finalized, "context not finalized");
  CXK_DEMAND(ctx->device >= 0,
             "no HIP device bound to this context: the KKT path has no CPU fallback");
  CXK_DEMAND(ctx->device_ready, "device state of this context was not built (cxk_finalize failed)");
  return CXK_SUCCESS;
}

// cxk_kkt_solve_async and the factor-and-solve entry points fold the assembly into the first
// factor level when the tree allows it (BuildPlans) and nothing needs the assembled system as
// such: Cholesky sweeps, no refinement copy (sharded contexts: when the first level lies below the cut).
bool FusedAssembly(const cxk_context* ctx) {
  return (ctx->fused_asm || ctx->fused_tree) && ctx->solver_mode != 2 && ctx->refine_iters <= 0 && !ctx->no_lean;
}
// cxk_assemble leaves the gather to the factorization that normally follows; any other entry point
// that runs first gets the assembled system by the separate launch.
int FlushDeferred(cxk_context* ctx, bool keep_scalars, bool keep_y) {
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
// ---- cxk_finalize as a sequence of stages
static FinalizeSwitches ReadFinalizeSwitches() {
  FinalizeSwitches sw;
  const char* v = getenv("CXK_REFERENCE_QUIRKS");
  sw.quirks_off = v && atoi(v) == 0 && v[0] != '\0';
  if ((v = getenv("CXK_CHAIN_SEGMENTS"))) sw.chain_segments = atoi(v);
  if ((v = getenv("CXK_SPARSE_LMI"))) sw.modes.sparse_lmi = atoi(v) != 0;
  if ((v = getenv("CXK_GEMM_MIN_N"))) sw.gemm_min_n = atoi(v);
  v = getenv("CXK_LMI_SCHUR");
  sw.schur_generic = v && !strcmp(v, "generic");
  sw.no_herm_fold = getenv("CXK_NO_HERM_FOLD") != nullptr;
  sw.no_packed_slack = getenv("CXK_NO_PACKED_SLACK") != nullptr;
  if ((v = getenv("CXK_GRAM_SPLITS"))) sw.gram_splits = std::max(1, atoi(v));
  if ((v = getenv("CXK_STREAMED_CONES"))) sw.modes.streamed_cones = atoi(v) != 0;
  if ((v = getenv("CXK_SOC_STREAM_STAGES"))) sw.soc_stream_stages = atoi(v);
  if ((v = getenv("CXK_TILED_LINEAR")) && v[0] != '\0') sw.modes.tiled_linear = atoi(v) != 0;
  if ((v = getenv("CXK_STREAMED_QUADRATIC")) && v[0] != '\0') sw.modes.streamed_quadratic = atoi(v) != 0;
  if ((v = getenv("CXK_STREAMED_QUADRATIC_MIN_WORK")) && v[0] != '\0') sw.modes.streamed_quadratic_min_work = std::max(0ll, atoll(v));
  if ((v = getenv("CXK_QUAD_CSR_LANES")) && (atoi(v) == 1 || atoi(v) == 8 || atoi(v) == 64)) sw.quad_csr_lanes = atoi(v);
  if ((v = getenv("CXK_SPARSE_LINEAR")) && v[0] != '\0') sw.modes.sparse_linear = atoi(v) != 0;
  if ((v = getenv("CXK_SPARSE_LINEAR_MIN_RATIO")) && v[0] != '\0') sw.modes.sparse_linear_min_ratio = std::max(0.0, atof(v));
  if ((v = getenv("CXK_TILED_LINEAR_MIN_WORK")) && v[0] != '\0') sw.modes.tiled_linear_min_work = std::max(0ll, atoll(v));
  if ((v = getenv("CXK_SPARSE_SOC")) && v[0] != '\0') sw.modes.sparse_soc = atoi(v) != 0;
  if ((v = getenv("CXK_SPARSE_SOC_MIN_RATIO")) && v[0] != '\0') sw.modes.sparse_soc_min_ratio = std::max(0.0, atof(v));
  if ((v = getenv("CXK_SPARSE_AFFINE")) && v[0] != '\0') sw.modes.sparse_affine = std::max(-1, std::min(1, atoi(v)));
  if ((v = getenv("CXK_SPARSE_AFFINE_MIN_RATIO")) && v[0] != '\0') sw.modes.sparse_affine_min_ratio = std::max(0.0, atof(v));
  if ((v = getenv("CXK_SPARSE_FOLD")) && v[0] != '\0') sw.modes.sparse_fold = atoi(v) != 0;
  if ((v = getenv("CXK_WIDE_SPECTRUM")) && v[0] != '\0') sw.wide_spectrum = std::max(-1, std::min(1, atoi(v)));
  if ((v = getenv("CXK_WIDE_REDUCE_MIN_ORDER")) && v[0] != '\0') sw.wide_reduce_min_order = std::max(0, atoi(v));
  return sw;
}

// The elimination structure: the reference's analysis, a segment-parallel order for long chain-shaped trees,
// the tree's levels and partition, the constraints' offsets in the Schur arena.
static int ChooseEliminationStructure(cxk_context* ctx, const FinalizeSwitches& sw) {
  // default: the reference as written; CXK_REFERENCE_QUIRKS=0 opts into the two corrections
  if (ctx->reference_identity < 0) ctx->reference_identity = !sw.quirks_off;
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
    if (want < 0) want = sw.chain_segments;
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
  return CXK_SUCCESS;
}

// The system's device buffers: Schur arena, slab, vectors, failure words, per-constraint step outputs.
static int AllocateSystemBuffers(cxk_context* ctx) {
  const int K = (int)ctx->cons.size();
  const int64_t go = ctx->g_off.empty() ? 0 : ctx->g_off[K - 1] + (int64_t)ctx->cons[K - 1].m * ctx->cons[K - 1].m;
  const int64_t ro = ctx->r_off.empty() ? 0 : ctx->r_off[K - 1] + ctx->cons[K - 1].m;
  // (two more words behind the last block: the +0.0 and the 1.0 the whole-tree launch's load images point entries
  // at that do not exist, PlanFusedTree)
  CXK_TRY(ctx->G.alloc((size_t)go + 2));
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
  return CXK_SUCCESS;
}

static int FinalizeImpl(cxk_context* ctx) {
  const FinalizeSwitches sw = ReadFinalizeSwitches();
  for (const ConstraintRec& c : ctx->cons)
    if (c.factors.given && c.herm_d) {
      // Hermitian factors (order c.n = d x the hyper-complex order, factors.F = L(F) of d R columns): the Taylor TakeStep
      // has no LU; what bounds the order is the one-workgroup Lanczos of lmi_large_spectrum, then the int indexing
      const int64_t N = c.n, R = c.factors.R, d = c.herm_d;
      if (c.n > LmiLargeSpectrumMaxOrder()) {
        ctx->err = "a factored Hermitian constraint whose real representation has an order above " +
                   std::to_string(LmiLargeSpectrumMaxOrder()) + " is not supported (the vectors of its Lanczos run exceed the " +
                   std::to_string(kLdsLimit) + " B of LDS)";
        fprintf(stderr, "%s line %d: %s\n", __FILE__, __LINE__, ctx->err.c_str());
        return CXK_FAILURE;
      }
      CXK_DEMAND(N * R <= INT_MAX, "a factored Hermitian constraint whose N x R entries (N = d n) exceed the int range is not supported");
      CXK_DEMAND(d * R * R <= INT_MAX, "a factored Hermitian constraint whose d x R x R entries exceed the int range is not supported");
      CXK_DEMAND(N * d * R <= INT_MAX, "a factored Hermitian constraint whose N x dR entries (N = d n) exceed the int range is not supported");
      CXK_DEMAND((int64_t)c.m * c.m <= INT_MAX, "a factored Hermitian constraint whose m x m entries exceed the int range is not supported");
    } else if (c.factors.given) {  // the limit of LmiLargeLuSolve, and the int indexing of kernels_lmi_factored.hip.h
      CXK_DEMAND(c.n <= 1024, "a factored LMI of order above 1024 is not supported (one panel row per thread in the Pade LU)");
      CXK_DEMAND((int64_t)c.n * c.factors.R <= INT_MAX && (int64_t)c.factors.R * c.factors.R <= INT_MAX && (int64_t)c.m * c.m <= INT_MAX,
                 "a factored LMI whose n x R, R x R or m x m entries exceed the int range is not supported");
    }
  // matrix inequalities given by their matrices: any order whose n x n entries the kernels can index; beyond the
  // one-workgroup Lanczos run (lmi_large_spectrum) only with the chip-wide one (cxk_set_wide_spectrum)
  for (const ConstraintRec& c : ctx->cons)
    if (c.type == CXK_LMI && !c.factors.given) {
      CXK_DEMAND((int64_t)c.n * c.n <= INT_MAX,
                 "a matrix inequality of order above 46340 is not supported (the kernels index its n x n entries with ints)");
      if (c.n > LmiLargeSpectrumMaxOrder() && WideSpectrumMode(ctx, sw) == 0) {
        ctx->err = "a matrix inequality whose (real representation's) order is above " + std::to_string(LmiLargeSpectrumMaxOrder()) +
                   " needs the chip-wide Lanczos run (cxk_set_wide_spectrum / CXK_WIDE_SPECTRUM, which is 0)";
        fprintf(stderr, "%s line %d: %s\n", __FILE__, __LINE__, ctx->err.c_str());
        return CXK_FAILURE;
      }
    }
  // a matrix inequality held by its nonzeros has one route (a host-only context says so too: cone_route.h has the words)
  for (const ConstraintRec& c : ctx->cons)
    if (c.type == CXK_LMI && c.csr_only) {
      ConeShape s;
      s.type = c.type, s.n = c.n, s.m = c.m, s.herm_d = c.herm_d, s.csr_only = true;
      const RouteChoice choice = Choose(s, sw.modes);
      CXK_DEMAND(!choice.refusal, choice.refusal);
    }
  if (ChooseEliminationStructure(ctx, sw)) return CXK_FAILURE;
  ctx->finalized = true;
  if (ctx->device < 0) return CXK_SUCCESS;  // symbolic-only context

  CXK_TRY(RaiseLdsLimits());
  CXK_TRY(hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  if (GroupConstraints(ctx, sw)) return CXK_FAILURE;
  for (Group& g : ctx->groups)
    if (UploadGroup(ctx, g, sw)) return CXK_FAILURE;
  if (AllocateSystemBuffers(ctx)) return CXK_FAILURE;
  if (BuildPlans(ctx) != CXK_SUCCESS) return CXK_FAILURE;
  ctx->device_ready = true;
  return cxk_set_identity(ctx);
}

static bool DeviceMuOk(const cxk_context* ctx) {
  // one GPU, Cholesky on the device (the QR mode solves on the host), every TakeStep kernel able to
  // take its step length from the device (TakeStepFromDeviceOk: no equality rows, no LMI beyond LDS)
  return !ctx->no_device_mu && ctx->world <= 1 && ctx->solver_mode != 2 && TakeStepFromDeviceOk(ctx);
}

}  // namespace cxk_host

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
  if (const char* v = getenv("CXK_LMI_ORDER")) ctx->lmi_order_forward = !strcmp(v, "forward");
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
  // (an order whose n x n entries no int indexes is refused by cxk_finalize, by name: its 17 GB and more are not copied)
  if ((int64_t)n * n > INT_MAX) return AddConstraint(ctx, std::move(r), vars);
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

int cxk_add_lmi_factored(cxk_context* ctx, int n, int m, const int* rank_ptr, const double* F, const double* sigma,
                         const double* C, const int* vars) {
  if (!ctx) return -1;
  auto refuse = [ctx](const char* msg) {
    ctx->err = std::string("cxk_add_lmi_factored: ") + msg;
    return -1;
  };
  if (n < 1 || m < 0) return refuse("n is at least 1 and m at least 0");
  if (!rank_ptr || !C) return refuse("rank_ptr or C is null");
  if (rank_ptr[0] != 0) return refuse("rank_ptr[0] is not 0");
  for (int i = 0; i < m; i++)
    if (rank_ptr[i + 1] < rank_ptr[i]) return refuse("rank_ptr decreases");
  const int R = rank_ptr[m];
  if (R > 0 && !F) return refuse("F is null");
  const size_t nr = (size_t)n * R, nn = (size_t)n * n;
  for (size_t q = 0; q < nr; q++)
    if (!std::isfinite(F[q])) return refuse("F holds a value that is not finite");
  for (int k = 0; sigma && k < R; k++)
    if (!std::isfinite(sigma[k])) return refuse("sigma holds a value that is not finite");
  for (size_t q = 0; q < nn; q++)
    if (!std::isfinite(C[q])) return refuse("C holds a value that is not finite");
  for (int c = 0; c < n; c++)
    for (int q = c + 1; q < n; q++)
      if (C[q + (size_t)c * n] != C[c + (size_t)q * n]) return refuse("C is not symmetric");
  ConstraintRec r;
  r.type = CXK_LMI;
  r.n = n;
  r.m = m;
  r.factors.given = true;
  r.factors.R = R;
  r.factors.ptr.assign(rank_ptr, rank_ptr + m + 1);
  r.factors.F.assign(F, F + nr);
  if (sigma)
    r.factors.sigma.assign(sigma, sigma + R);
  else
    r.factors.sigma.assign((size_t)R, 1.0);
  r.C.assign(C, C + nn);
  return AddConstraint(ctx, std::move(r), vars);
}

int cxk_add_lmi_coo(cxk_context* ctx, int n, int m, const int* ptr, const int* row, const int* col, const double* val,
                    const int* vars) {
  if (!ctx) return -1;
  auto refuse = [ctx](const std::string& msg) {
    ctx->err = "cxk_add_lmi_coo: " + msg;
    return -1;
  };
  if (n < 1 || m < 0) return refuse("n is at least 1 and m at least 0");
  if (!ptr) return refuse("ptr is null");
  // (before anything of size n x n is touched)
  if (n > kSparseLmiMaxIndex || m > kSparseLmiMaxIndex)
    return refuse("n or m is above " + std::to_string(kSparseLmiMaxIndex) +
                  " (the entry table packs row | col << 16 and the pair table i | j << 16 into ints that the kernels "
                  "unpack with signed shifts)");
  if (ptr[0] != 0) return refuse("ptr[0] is not 0");
  for (int i = 0; i <= m; i++)
    if (ptr[i + 1] < ptr[i]) return refuse("ptr decreases");
  if (ptr[m + 1] > 0 && (!row || !col || !val)) return refuse("row, col or val is null");
  ConstraintRec r;
  r.type = CXK_LMI;
  r.n = n;
  r.m = m;
  r.csr_only = true;
  r.entries.affine_default = -1;
  r.entries.ptr.assign((size_t)m + 2, 0);
  std::vector<std::pair<int, double>> list;  // (row | col << 16, value): both triangles of one matrix
  for (int i = 0; i <= m; i++) {
    list.clear();
    for (int s = ptr[i]; s < ptr[i + 1]; s++) {
      if (row[s] < 0 || row[s] >= n || col[s] < 0 || col[s] >= n) return refuse("an index is outside [0, n)");
      if (row[s] < col[s]) return refuse("an entry lies above the diagonal (row < col): the lower triangle is given");
      if (!std::isfinite(val[s])) return refuse("a value is not finite");
      list.emplace_back(row[s] | (col[s] << 16), val[s]);
      if (row[s] != col[s]) list.emplace_back(col[s] | (row[s] << 16), val[s]);
    }
    // by column, then row: the packed word orders exactly so
    std::sort(list.begin(), list.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
    for (size_t s = 1; s < list.size(); s++)
      if (list[s].first == list[s - 1].first) return refuse("a list names a position twice");
    for (const auto& e : list)
      if (e.second != 0.0) {  // explicit zeros are dropped
        r.entries.rc.push_back(e.first);
        r.entries.val.push_back(e.second);
      }
    if (r.entries.rc.size() > (size_t)INT_MAX) return refuse("more than 2^31 nonzeros");
    r.entries.ptr[(size_t)i + 1] = (int)r.entries.rc.size();
  }
  r.C.assign((size_t)n * n, 0.0);
  for (int e = r.entries.ptr[m]; e < r.entries.ptr[m + 1]; e++)
    r.C[(size_t)(r.entries.rc[e] & 0xffff) + (size_t)(r.entries.rc[e] >> 16) * n] = r.entries.val[e];
  return AddConstraint(ctx, std::move(r), vars);
}

// jordan_matrix_algebra.cc:103-124 (4 x 4 corner): plane i ^ j of X Y receives sign[i][j] X_i Y_j.
// Real representation L(X): block (k, j) = sign[k ^ j][j] X_{k ^ j}; L(XY) = L(X) L(Y),
// L(X^*) = L(X)^T, tr L(X) = d Re tr X.
const int kHcSign[4][4] = {{1, 1, 1, 1}, {1, -1, -1, 1}, {1, 1, -1, -1}, {1, -1, 1, -1}};
// (also for rectangular arguments, planes of n x cols: L(X) is (d n) x (d cols), and stays multiplicative)
void EmbedPlanesRect(int d, int n, int cols, const double* planes, double* out /* (d n) x (d cols) col-major */) {
  const size_t nc = (size_t)n * cols, N = (size_t)d * n;
  for (int k = 0; k < d; k++)
    for (int j = 0; j < d; j++) {
      const double* X = planes + (size_t)(k ^ j) * nc;
      const double sg = kHcSign[k ^ j][j];
      for (int c = 0; c < cols; c++)
        for (int r = 0; r < n; r++) out[((size_t)j * cols + c) * N + (size_t)k * n + r] = sg * X[(size_t)c * n + r];
    }
}
void EmbedPlanes(int d, int n, const double* planes, double* out /* (d n)^2 col-major */) { EmbedPlanesRect(d, n, n, planes, out); }
void ExtractPlanes(int d, int n, const double* emb, double* planes) {
  const size_t nn = (size_t)n * n, N = (size_t)d * n;
  for (int k = 0; k < d; k++)  // block (k, 0) = sign[k][0] X_k = X_k
    for (int c = 0; c < n; c++)
      for (int r = 0; r < n; r++) planes[(size_t)k * nn + (size_t)c * n + r] = emb[(size_t)c * N + (size_t)k * n + r];
}

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

int cxk_add_hermitian_coo(cxk_context* ctx, int n, int d, int m, const int* ptr, const int* row, const int* col,
                          const double* val, const int* vars) {
  if (!ctx) return -1;
  auto refuse = [ctx](const std::string& msg) {
    ctx->err = "cxk_add_hermitian_coo: " + msg;
    return -1;
  };
  if (n < 1 || m < 0) return refuse("n is at least 1 and m at least 0");
  if (d == 8) return refuse("hyper-complex dimension 8: the octonions have no real representation, entries are for d = 1, 2, 4");
  if (d != 1 && d != 2 && d != 4) return refuse("the hyper-complex dimension is 1, 2 or 4");
  if (!ptr) return refuse("ptr is null");
  // (before anything of size d n x d n is touched)
  if ((int64_t)d * n > kSparseLmiMaxIndex || m > kSparseLmiMaxIndex)
    return refuse("d n or m is above " + std::to_string(kSparseLmiMaxIndex) +
                  " (the entry table packs row | col << 16 and the pair table i | j << 16 into ints that the kernels "
                  "unpack with signed shifts)");
  if (ptr[0] != 0) return refuse("ptr[0] is not 0");
  for (int i = 0; i <= m; i++)
    if (ptr[i + 1] < ptr[i]) return refuse("ptr decreases");
  if (ptr[m + 1] > 0 && (!row || !col || !val)) return refuse("row, col or val is null");
  ConstraintRec r;
  r.type = CXK_LMI;
  r.herm_d = d;
  r.n = d * n;
  r.m = m;
  r.csr_only = true;
  r.entries.fold_default = 1;
  r.entries.ptr.assign((size_t)m + 2, 0);
  std::vector<int> seen;                     // the positions of one list, both triangles
  std::vector<std::pair<int, double>> list;  // (row | col << 16, value) of one real representation
  for (int i = 0; i <= m; i++) {
    seen.clear();
    list.clear();
    for (int s = ptr[i]; s < ptr[i + 1]; s++) {
      const int rs = row[s], cs = col[s];
      const double* v = val + (size_t)d * s;
      if (rs < 0 || rs >= n || cs < 0 || cs >= n) return refuse("an index is outside [0, n)");
      if (rs < cs) return refuse("an entry lies above the diagonal (row < col): the lower triangle is given");
      for (int p = 0; p < d; p++)
        if (!std::isfinite(v[p])) return refuse("a value is not finite");
      for (int p = 1; p < d; p++)
        if (rs == cs && v[p] != 0.0)
          return refuse("a diagonal entry has a nonzero plane beyond the first (the diagonal of a Hermitian matrix is real)");
      seen.push_back(rs | (cs << 16));
      // block (k, j) of L(X) is kHcSign[k ^ j][j] X_{k ^ j}; the mirrored entry is the conjugate: X_p[c,r] = -X_p[r,c], p >= 1
      for (int p = 0; p < d; p++) {
        if (v[p] == 0.0) continue;  // (a zero plane makes no real entry; an entry of zero planes is dropped)
        for (int j = 0; j < d; j++) {
          const int k = p ^ j;
          const double a = kHcSign[p][j] * v[p];
          list.emplace_back((k * n + rs) | ((j * n + cs) << 16), a);
          if (rs != cs) list.emplace_back((k * n + cs) | ((j * n + rs) << 16), p ? -a : a);
        }
      }
    }
    std::sort(seen.begin(), seen.end());
    for (size_t s = 1; s < seen.size(); s++)
      if (seen[s] == seen[s - 1]) return refuse("a list names a position twice");
    // by column, then row: the packed word orders exactly so (distinct positions give distinct real entries)
    std::sort(list.begin(), list.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
    if (r.entries.rc.size() + list.size() > (size_t)INT_MAX) return refuse("more than 2^31 nonzeros");
    for (const auto& e : list) {
      r.entries.rc.push_back(e.first);
      r.entries.val.push_back(e.second);
    }
    r.entries.ptr[(size_t)i + 1] = (int)r.entries.rc.size();
  }
  r.C.assign((size_t)r.n * r.n, 0.0);
  for (int e = r.entries.ptr[m]; e < r.entries.ptr[m + 1]; e++)
    r.C[(size_t)(r.entries.rc[e] & 0xffff) + (size_t)(r.entries.rc[e] >> 16) * r.n] = r.entries.val[e];
  return AddConstraint(ctx, std::move(r), vars);
}

int cxk_add_hermitian_factored(cxk_context* ctx, int n, int d, int m, const int* rank_ptr, const double* F, const double* sigma,
                               const double* C, const int* vars) {
  if (!ctx) return -1;
  auto refuse = [ctx](const char* msg) {
    ctx->err = std::string("cxk_add_hermitian_factored: ") + msg;
    return -1;
  };
  if (n < 1 || m < 0) return refuse("n is at least 1 and m at least 0");
  if (d == 8) return refuse("hyper-complex dimension 8: the octonions have no real representation, factors are for d = 1, 2, 4");
  if (d != 1 && d != 2 && d != 4) return refuse("the hyper-complex dimension is 1, 2 or 4");
  if (!rank_ptr || !C) return refuse("rank_ptr or C is null");
  if (rank_ptr[0] != 0) return refuse("rank_ptr[0] is not 0");
  for (int i = 0; i < m; i++)
    if (rank_ptr[i + 1] < rank_ptr[i]) return refuse("rank_ptr decreases");
  const int R = rank_ptr[m];
  if (R > 0 && !F) return refuse("F is null");
  const size_t nr = (size_t)n * R, nn = (size_t)n * n;
  for (size_t q = 0; q < d * nr; q++)
    if (!std::isfinite(F[q])) return refuse("F holds a value that is not finite");
  for (int k = 0; sigma && k < R; k++)
    if (!std::isfinite(sigma[k])) return refuse("sigma holds a value that is not finite");
  for (size_t q = 0; q < d * nn; q++)
    if (!std::isfinite(C[q])) return refuse("C holds a value that is not finite");
  for (int p = 0; p < d; p++)
    for (int c = 0; c < n; c++)
      for (int q = c; q < n; q++) {
        const double lo = C[p * nn + q + (size_t)c * n], up = C[p * nn + c + (size_t)q * n];
        if (p == 0 ? lo != up : lo != -up) return refuse("C is not Hermitian (plane 0 symmetric, the others skew)");
      }
  ConstraintRec r;
  r.type = CXK_LMI;
  r.herm_d = d;
  r.n = d * n;
  r.m = m;
  r.factors.given = true;
  r.factors.R = R;
  r.factors.ptr.assign(rank_ptr, rank_ptr + m + 1);
  r.factors.F.resize((size_t)d * d * nr);  // L(F): (d n) x (d R); its first R columns are the stacked planes
  if (R > 0) EmbedPlanesRect(d, n, R, F, r.factors.F.data());
  if (sigma)
    r.factors.sigma.assign(sigma, sigma + R);
  else
    r.factors.sigma.assign((size_t)R, 1.0);
  r.C.resize((size_t)r.n * r.n);
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

// cxk_add_linear_csr / cxk_add_soc_csr: a constraint of `type` whose matrix of `rows` rows is given by its nonzeros;
// `fn` names the caller in the refusals, `size` its size argument.
static int AddCsrConstraint(cxk_context* ctx, const char* fn, const char* size, int type, int n, int rows, int m,
                            const int* rowptr, const int* col, const double* val, const double* c, const int* vars) {
  if (!ctx) return -1;
  auto refuse = [ctx, fn](const std::string& msg) {
    ctx->err = std::string(fn) + ": " + msg;
    return -1;
  };
  if (n < 1 || rows < 1 || m < 0) return refuse(std::string(size) + " is at least 1 and m at least 0");
  if (!rowptr || !c) return refuse("rowptr or c is null");
  if (rowptr[0] != 0) return refuse("rowptr[0] is not 0");
  for (int r = 0; r < rows; r++)
    if (rowptr[r + 1] < rowptr[r]) return refuse("rowptr decreases");
  if (rowptr[rows] > 0 && (!col || !val)) return refuse("col or val is null");
  ConstraintRec rec;
  rec.type = type;
  rec.n = n;
  rec.m = m;
  rec.csr_only = true;
  rec.C.assign(c, c + rows);
  rec.rows.ptr.assign((size_t)rows + 1, 0);
  std::vector<std::pair<int, double>> row;
  for (int r = 0; r < rows; r++) {
    row.clear();
    for (int s = rowptr[r]; s < rowptr[r + 1]; s++) {
      if (col[s] < 0 || col[s] >= m) return refuse("a column is outside [0, m)");
      row.emplace_back(col[s], val[s]);
    }
    std::sort(row.begin(), row.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
    for (size_t s = 1; s < row.size(); s++)
      if (row[s].first == row[s - 1].first) return refuse("a row names a column twice");
    for (const auto& e : row)
      if (e.second != 0.0) {  // explicit zeros are dropped
        rec.rows.col.push_back(e.first);
        rec.rows.val.push_back(e.second);
      }
    rec.rows.ptr[(size_t)r + 1] = (int)rec.rows.col.size();
  }
  return AddConstraint(ctx, std::move(rec), vars);
}

int cxk_add_linear_csr(cxk_context* ctx, int rows, int m, const int* rowptr, const int* col, const double* val,
                       const double* c, const int* vars) {
  return AddCsrConstraint(ctx, "cxk_add_linear_csr", "rows", CXK_LINEAR, rows, rows, m, rowptr, col, val, c, vars);
}

int cxk_add_soc_csr(cxk_context* ctx, int n, int m, const int* rowptr, const int* col, const double* val, const double* c,
                    const int* vars) {
  return AddCsrConstraint(ctx, "cxk_add_soc_csr", "n", CXK_SOC, n, n < INT_MAX ? n + 1 : 0, m, rowptr, col, val, c, vars);
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

// The parts of Q = S + F diag(sigma) F' as cxk_add_quadratic_structured and cxk_add_quadratic_csr take them (n >= 1):
// why they are refused, or null.
static const char* StructuredQRefusal(int n, const int* q_rowptr, const int* q_col, const double* q_val, int rank, const double* F,
                                      const double* sigma) {
  if (rank < 0) return "rank is negative";
  if (!q_rowptr && rank == 0) return "neither a sparse part nor factors: for the identity pass Q = NULL to cxk_add_quadratic";
  if (rank > 0 && !F) return "F is null";
  if (q_rowptr) {
    if (q_rowptr[0] != 0) return "q_rowptr[0] is not 0";
    for (int r = 0; r < n; r++)
      if (q_rowptr[r + 1] < q_rowptr[r]) return "q_rowptr decreases";
    if (q_rowptr[n] > 0 && (!q_col || !q_val)) return "q_col or q_val is null";
    for (int e = 0; e < q_rowptr[n]; e++) {
      if (q_col[e] < 0 || q_col[e] >= n) return "a column of the sparse part is outside [0, n)";
      if (!std::isfinite(q_val[e])) return "q_val holds a value that is not finite";
    }
  }
  const size_t nr = (size_t)n * rank;
  for (size_t q = 0; q < nr; q++)
    if (!std::isfinite(F[q])) return "F holds a value that is not finite";
  for (int k = 0; sigma && k < rank; k++)
    if (!std::isfinite(sigma[k])) return "sigma holds a value that is not finite";
  return nullptr;
}
// ... and the record's copy of them, once they have passed.
static void KeepStructuredQ(ConstraintRec* r, int n, const int* q_rowptr, const int* q_col, const double* q_val, int rank,
                            const double* F, const double* sigma) {
  r->sq.given = true;
  r->sq.rank = rank;
  if (q_rowptr) {  // as given: duplicates stay, the kernels sum them
    r->sq.ptr.assign(q_rowptr, q_rowptr + n + 1);
    r->sq.col.assign(q_col, q_col + q_rowptr[n]);
    r->sq.val.assign(q_val, q_val + q_rowptr[n]);
  }
  if (rank > 0) r->sq.F.assign(F, F + (size_t)n * rank);
  if (sigma)
    r->sq.sigma.assign(sigma, sigma + rank);
  else
    r->sq.sigma.assign((size_t)rank, 1.0);
}

int cxk_add_quadratic_structured(cxk_context* ctx, int n, int m, const int* q_rowptr, const int* q_col, const double* q_val,
                                 int rank, const double* F, const double* sigma, const double* A, const double* c,
                                 const int* vars) {
  if (!ctx) return -1;
  auto refuse = [ctx](const char* msg) {
    ctx->err = std::string("cxk_add_quadratic_structured: ") + msg;
    return -1;
  };
  if (n < 1 || m < 0) return refuse("n is at least 1 and m at least 0");
  if (!A || !c) return refuse("A or c is null");
  if (const char* why = StructuredQRefusal(n, q_rowptr, q_col, q_val, rank, F, sigma)) return refuse(why);
  ConstraintRec r;
  r.type = CXK_QUAD;
  r.n = n;
  r.m = m;
  r.A.assign(A, A + (size_t)(n + 1) * m);
  r.C.assign(c, c + n + 1);
  KeepStructuredQ(&r, n, q_rowptr, q_col, q_val, rank, F, sigma);
  return AddConstraint(ctx, std::move(r), vars);
}

int cxk_add_quadratic_csr(cxk_context* ctx, int n, int m, const double* Q, const int* q_rowptr, const int* q_col, const double* q_val,
                          int rank, const double* F, const double* sigma, const int* a_rowptr, const int* a_col, const double* a_val,
                          const double* c, const int* vars) {
  if (!ctx) return -1;
  auto refuse = [ctx](const char* msg) {
    ctx->err = std::string("cxk_add_quadratic_csr: ") + msg;
    return -1;
  };
  if (n < 1 || n == INT_MAX || m < 0) return refuse("n is at least 1 and m at least 0");
  if (!a_rowptr || !c) return refuse("a_rowptr or c is null");
  const bool parts = q_rowptr || rank != 0 || F || sigma;
  if (Q && parts) return refuse("Q is given dense and by its parts: one form, or none for the identity");
  if (parts)
    if (const char* why = StructuredQRefusal(n, q_rowptr, q_col, q_val, rank, F, sigma)) return refuse(why);
  if (Q && (int64_t)n * n > INT_MAX) return refuse("a dense Q of more than 2^31 entries: give it by its parts");
  for (size_t q = 0; Q && q < (size_t)n * n; q++)
    if (!std::isfinite(Q[q])) return refuse("Q holds a value that is not finite");
  const int rows = n + 1;
  if (a_rowptr[0] != 0) return refuse("a_rowptr[0] is not 0");
  for (int r = 0; r < rows; r++)
    if (a_rowptr[r + 1] < a_rowptr[r]) return refuse("a_rowptr decreases");
  if (a_rowptr[rows] > 0 && (!a_col || !a_val)) return refuse("a_col or a_val is null");
  for (int r = 0; r < rows; r++)
    if (!std::isfinite(c[r])) return refuse("c holds a value that is not finite");
  ConstraintRec rec;
  rec.type = CXK_QUAD;
  rec.n = n;
  rec.m = m;
  rec.csr_only = true;
  rec.C.assign(c, c + rows);
  rec.rows.ptr.assign((size_t)rows + 1, 0);
  std::vector<std::pair<int, double>> row;
  for (int r = 0; r < rows; r++) {
    row.clear();
    for (int s = a_rowptr[r]; s < a_rowptr[r + 1]; s++) {
      if (a_col[s] < 0 || a_col[s] >= m) return refuse("a column is outside [0, m)");
      if (!std::isfinite(a_val[s])) return refuse("a_val holds a value that is not finite");
      row.emplace_back(a_col[s], a_val[s]);
    }
    std::sort(row.begin(), row.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
    for (size_t s = 1; s < row.size(); s++)
      if (row[s].first == row[s - 1].first) return refuse("a row names a column twice");
    for (const auto& e : row)
      if (e.second != 0.0) {  // explicit zeros are dropped
        rec.rows.col.push_back(e.first);
        rec.rows.val.push_back(e.second);
      }
    rec.rows.ptr[(size_t)r + 1] = (int)rec.rows.col.size();
  }
  if (Q) rec.Q.assign(Q, Q + (size_t)n * n);
  if (parts) KeepStructuredQ(&rec, n, q_rowptr, q_col, q_val, rank, F, sigma);
  return AddConstraint(ctx, std::move(rec), vars);
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

// The owned constraints cxk_finalize put on `route` (what the cxk_count_* of the routes report); -1 before it.
static int CountOnRoute(const cxk_context* ctx, ConeRoute route) {
  if (!ctx || !ctx->finalized) return -1;
  int k = 0;
  for (size_t i = 0; i < ctx->cons.size(); i++) k += ctx->owned[i] && ctx->cons[i].route == route;
  return k;
}

int cxk_set_streamed_cones(cxk_context* ctx, int on) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(!ctx->finalized, "cxk_set_streamed_cones: the context is finalized (the choice is made by cxk_finalize)");
  ctx->streamed_cones = on != 0;
  return CXK_SUCCESS;
}
int cxk_count_streamed_cones(const cxk_context* ctx) { return CountOnRoute(ctx, ConeRoute::kSocStreamed); }

int cxk_set_tiled_linear(cxk_context* ctx, int mode) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(!ctx->finalized, "cxk_set_tiled_linear: the context is finalized (the choice is made by cxk_finalize)");
  CXK_DEMAND(mode >= -1 && mode <= 1, "cxk_set_tiled_linear: the mode is -1 (automatic), 0 (never) or 1 (every linear block)");
  ctx->tiled_linear = mode;
  return CXK_SUCCESS;
}
int cxk_count_tiled_linear(const cxk_context* ctx) { return CountOnRoute(ctx, ConeRoute::kLinearTiled); }

int cxk_set_sparse_linear(cxk_context* ctx, int mode) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(!ctx->finalized, "cxk_set_sparse_linear: the context is finalized (the choice is made by cxk_finalize)");
  CXK_DEMAND(mode >= -1 && mode <= 1, "cxk_set_sparse_linear: the mode is -1 (automatic), 0 (never) or 1 (every linear block)");
  ctx->sparse_linear = mode;
  return CXK_SUCCESS;
}
int cxk_count_sparse_linear(const cxk_context* ctx) { return CountOnRoute(ctx, ConeRoute::kLinearSparse); }

int cxk_set_sparse_soc(cxk_context* ctx, int mode) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(!ctx->finalized, "cxk_set_sparse_soc: the context is finalized (the choice is made by cxk_finalize)");
  CXK_DEMAND(mode >= -1 && mode <= 1, "cxk_set_sparse_soc: the mode is -1 (automatic), 0 (never) or 1 (every second-order cone)");
  ctx->sparse_soc = mode;
  return CXK_SUCCESS;
}
int cxk_count_sparse_soc(const cxk_context* ctx) { return CountOnRoute(ctx, ConeRoute::kSocSparse); }

double cxk_sparse_soc_setup_ms(const cxk_context* ctx) { return ctx && ctx->finalized ? ctx->sparse_soc_setup_ms : 0.0; }

int cxk_set_sparse_affine(cxk_context* ctx, int mode) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(!ctx->finalized, "cxk_set_sparse_affine: the context is finalized (the choice is made by cxk_finalize)");
  CXK_DEMAND(mode >= -1 && mode <= 1, "cxk_set_sparse_affine: the mode is -1 (automatic), 0 (never) or 1 (every eligible sparse matrix inequality)");
  ctx->sparse_affine = mode;
  return CXK_SUCCESS;
}
int cxk_count_sparse_affine(const cxk_context* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  int k = 0;
  for (size_t i = 0; i < ctx->cons.size(); i++) k += ctx->owned[i] && ctx->cons[i].route == ConeRoute::kLmiSparse && ctx->cons[i].entries.sparse_affine;
  return k;
}

int cxk_set_sparse_fold(cxk_context* ctx, int mode) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(!ctx->finalized, "cxk_set_sparse_fold: the context is finalized (the choice is made by cxk_finalize)");
  CXK_DEMAND(mode == 0 || mode == 1, "cxk_set_sparse_fold: the mode is 0 (never) or 1 (every sparse Hermitian matrix inequality over C or H)");
  ctx->sparse_fold = mode;
  return CXK_SUCCESS;
}
int cxk_count_sparse_fold(const cxk_context* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  int k = 0;
  for (size_t i = 0; i < ctx->cons.size(); i++) k += ctx->owned[i] && ctx->cons[i].route == ConeRoute::kLmiSparse && ctx->cons[i].entries.fold;
  return k;
}

int cxk_set_wide_spectrum(cxk_context* ctx, int mode) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(!ctx->finalized, "cxk_set_wide_spectrum: the context is finalized (the choice is made by cxk_finalize)");
  CXK_DEMAND(mode >= -1 && mode <= 1, "cxk_set_wide_spectrum: the mode is -1 (automatic), 0 (never) or 1 (every large-order matrix inequality)");
  ctx->wide_spectrum = mode;
  return CXK_SUCCESS;
}
int cxk_count_wide_spectrum(const cxk_context* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  int k = 0;
  for (const Group& g : ctx->groups)
    if (LmiOnWideSpectrum(g)) k += (int)g.ids.size();
  return k;
}

int cxk_set_streamed_quadratic(cxk_context* ctx, int mode) {
  if (!ctx) return CXK_FAILURE;
  CXK_DEMAND(!ctx->finalized, "cxk_set_streamed_quadratic: the context is finalized (the choice is made by cxk_finalize)");
  CXK_DEMAND(mode >= -1 && mode <= 1, "cxk_set_streamed_quadratic: the mode is -1 (automatic), 0 (never) or 1 (every quadratic cone)");
  ctx->streamed_quadratic = mode;
  return CXK_SUCCESS;
}
int cxk_count_streamed_quadratic(const cxk_context* ctx) { return CountOnRoute(ctx, ConeRoute::kQuadStreamed); }
int cxk_count_structured_quadratic(const cxk_context* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  int k = 0;
  for (size_t i = 0; i < ctx->cons.size(); i++) k += ctx->owned[i] && ctx->cons[i].route == ConeRoute::kQuadStreamed && ctx->cons[i].sq.given;
  return k;
}

int cxk_count_sparse_quadratic(const cxk_context* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  int k = 0;
  for (size_t i = 0; i < ctx->cons.size(); i++)
    k += ctx->owned[i] && ctx->cons[i].route == ConeRoute::kQuadStreamed && ctx->cons[i].type == CXK_QUAD && ctx->cons[i].csr_only;
  return k;
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
  return LaunchSetIdentity(ctx);
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
  if (ctx->asm_deferred && FusedAssembly(ctx)) {  // gather and right-hand side ride in the first factor level
    ctx->asm_deferred = false;
    ctx->asm_pending.on = true;
    ctx->asm_pending.with_rhs = 2;
    ctx->asm_pending.cb = cb;
    ctx->asm_pending.cq = cq;
    ctx->asm_pending.cw = cw;
  } else {
    if (FlushDeferred(ctx)) return CXK_FAILURE;
    if (LaunchBuildRhsComb(ctx, cb, cq, cw, ctx->d_fail.p)) return CXK_FAILURE;
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
  if (ctx->asm_deferred && FusedAssembly(ctx)) {
    ctx->asm_deferred = false;
    ctx->asm_pending.on = true;
    ctx->asm_pending.with_rhs = 1;
    ctx->asm_pending.k = k;
    ctx->asm_pending.bs = bs;
    ctx->asm_pending.cs = cs;
  } else {
    if (FlushDeferred(ctx)) return CXK_FAILURE;
    if (LaunchBuildRhs(ctx, k, bs, cs, ctx->d_fail.p)) return CXK_FAILURE;
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
  const bool inline_rhs = (ctx->forward_all_lean || ctx->fused_tree) && ctx->world == 1 && ctx->solver_mode != 2 &&
                          ctx->refine_iters <= 0 && !ctx->no_lean;
  if (inline_rhs) {
    ctx->rhs_in = form;
  } else if (form.form == 1) {
    if (LaunchBuildRhs(ctx, form.k, form.bs, form.cs, nullptr, form.k_from)) return CXK_FAILURE;
  } else {
    if (LaunchBuildRhsComb(ctx, form.cb, form.cq, form.cw, nullptr)) return CXK_FAILURE;
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
  if (LaunchBuildRhsComb(ctx, 0.0, 0.0, -2.0, nullptr)) return CXK_FAILURE;
  if (LaunchTree(ctx, 1, true, true)) return CXK_FAILURE;
  CXK_TRY(hipMemcpyAsync(ctx->y2.p, ctx->y.p, sizeof(double) * N, hipMemcpyDeviceToDevice, ctx->stream));
  if (LaunchBuildRhsComb(ctx, b_scaling, c_scaling, -2.0, nullptr)) return CXK_FAILURE;
  if (LaunchTree(ctx, 1, true, true)) return CXK_FAILURE;
  if (LaunchLinearLineSearch(ctx, dinf_upper_bound, c_scaling)) return CXK_FAILURE;
  std::vector<double> out((size_t)2 * K);
  const double* pairs = ctx->info2.p;
  if (ctx->world > 1) {  // every rank evaluated its own linear constraints: gather the bounds
    if (SettleBeforeUnmarked(ctx)) return CXK_FAILURE;
    CXK_DEMAND((size_t)2 * K <= ctx->shard_tmp.n, "internal error: shard scratch too small");
    if (LaunchMaskedCopyPairs(ctx, K, ctx->info2.p, ctx->shard_tmp.p)) return CXK_FAILURE;
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
    if (LaunchMaskedCopy(ctx, N, ctx->y.p, ctx->shard_tmp.p)) return CXK_FAILURE;
    if (ShardAllReduce(ctx, ctx->shard_tmp.p, (size_t)N, kOpSum)) return CXK_FAILURE;
    ysrc = ctx->shard_tmp.p;
  }
  if (LaunchCopyDoubles(ctx, N, ysrc, ctx->pin_y)) return CXK_FAILURE;
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

int cxk_prepare_step(cxk_context* ctx, int affine, double c_weight, double e_weight, double* info) {
  return PrepareStepImpl(ctx, affine, c_weight, e_weight, info, false, nullptr);
}
int cxk_prepare_take_step(cxk_context* ctx, double c_weight, double e_weight, double* info, int* took) {
  if (took) *took = 0;
  return PrepareStepImpl(ctx, 0, c_weight, e_weight, info, true, took);
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

int cxk_weighted_slack_eigenvalues(cxk_context* ctx, double c_weight, double* out) {
  return SlackEigenvaluesImpl(ctx, c_weight, out, nullptr);
}

// ---- the barrier parameter selected on the device: conex::Solve's iteration without the host round
// trip between the eigenvalue query and the Newton direction (cone_program.cc:366-413).
int cxk_device_mu_supported(cxk_context* ctx) {
  if (!ctx || CheckReady(ctx)) return 0;
  return DeviceMuOk(ctx) ? 1 : 0;
}
int cxk_select_mu_async(cxk_context* ctx, double c_weight, double divergence_upper_bound, int rank, double prev,
                        double lb, double ub) {
  CXK_ENTER_KEEP(ctx);  // (binds the context's device for the allocation below; the query itself enters again)
  CXK_DEMAND(DeviceMuOk(ctx), "cxk_select_mu_async: not supported by this program (cxk_device_mu_supported)");
  if (ctx->mu_dev.n != 1) CXK_TRY(ctx->mu_dev.alloc(1, true));
  return SelectMuAsync(ctx, c_weight, divergence_upper_bound, rank, prev, lb, ub);
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
  if (G) {
    // Entry (r, c) of the block sits at c * m + r, and the contract is r >= c (Arena::G, lmi_types.h): above the
    // diagonal lies whatever the route left there, on the matrix-inequality routes memory nobody wrote.  The caller
    // gets what the consumers read, mirrored into the full symmetric square.
    CXK_TRY(hipMemcpy(G, ctx->G.p + ctx->g_off[i], sizeof(double) * (size_t)m * m,
                      hipMemcpyDeviceToHost));
    for (int c = 1; c < m; c++)
      for (int r = 0; r < c; r++) G[(size_t)c * m + r] = G[(size_t)r * m + c];
  }
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

int cxk_owns_constraint(const cxk_context* ctx, int i) {
  if (!ctx || !ctx->finalized || i < 0 || i >= (int)ctx->cons.size()) return 0;
  return ctx->owned[i];
}

int cxk_get_valid_variables(const cxk_context* ctx, unsigned char* mask /* one per variable and multiplier, original order */) {
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

int cxk_gemm_f64_layout(int device, double* arena, long long arena_len, const long long* f, double alpha, double beta,
                        int* route) {
  if (!arena || !f || arena_len <= 0) return CXK_FAILURE;
  enum { kM, kN, kK, kTa, kTb, kBatch, kInner, kLower, kSplits, kOrdered, kTile, kGeneral, kOffA, kLda, kSA1, kSA2, kOffB, kLdb,
         kSB1, kSB2, kOffC, kLdc, kSC1, kSC2, kOffCt, kLdct, kST1, kST2, kCtb, kSTb, kOffPart, kSCs };
  const long long M = f[kM], N = f[kN], K = f[kK], batch = f[kBatch], inner = f[kInner], splits = f[kSplits];
  const bool ta = f[kTa] != 0, tb = f[kTb] != 0, ordered = f[kOrdered] != 0;
  const long long kMaxDim = 1ll << 24;  // (keeps every product below in 64 bits)
  if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || inner <= 0 || splits <= 0) return CXK_FAILURE;
  if (M > kMaxDim || N > kMaxDim || K > kMaxDim || batch > kMaxDim || splits > kMaxDim || inner > kMaxDim) return CXK_FAILURE;
  if (f[kTile] != 0 && f[kTile] != 64 && f[kTile] != 128 && f[kTile] != 12864) return CXK_FAILURE;
  for (int i = kOffA; i <= kSCs; i++) {
    const bool optional = i == kOffCt || i == kOffPart;
    if (f[i] > arena_len || f[i] < (optional ? -1 : 0)) return CXK_FAILURE;
  }
  const bool has_ct = f[kOffCt] >= 0, split = splits > 1;
  if (split && f[kOffPart] < 0) return CXK_FAILURE;
  if (f[kCtb] < 0 || (has_ct && f[kLdct] < 1)) return CXK_FAILURE;
  // Footprints, in 64-bit host arithmetic: of every operand and of C for every batch member (a matrix of `rows` rows
  // in columns `ld` apart ends (columns - 1) ld + rows behind its first element, so that a block of a larger matrix
  // may end where that matrix ends; an operand's rows count up to the next even number, the 16-byte chunks of the
  // LDS-DMA kernels), the partials of every split, and the image of C in Ct.  Every offset, stride and leading
  // dimension is in [0, arena_len] and every count at most 2^24, so no term below leaves 64 bits.
  auto extent = [](long long rows, long long ld, long long cols) { return (cols - 1) * ld + std::min(ld, rows); };
  auto inside = [&](long long lo, long long len) { return lo >= 0 && len >= 0 && lo <= arena_len && len <= arena_len - lo; };
  const long long rows_a = ta ? K : M, cols_a = ta ? M : K, rows_b = tb ? N : K, cols_b = tb ? K : N;
  if (f[kLda] < rows_a || f[kLdb] < rows_b || f[kLdc] < M) return CXK_FAILURE;
  if (f[kLda] > arena_len / cols_a || f[kLdb] > arena_len / cols_b || f[kLdc] > arena_len / N) return CXK_FAILURE;
  // Strides are not negative, so the footprints reach furthest at the first member, at the last one, and (inner > 1)
  // at the last member of the last full group of `inner`; the last split reaches furthest among the splits.
  const long long last = batch - 1, ends[3] = {0, last, (last / inner) * inner - 1};
  for (int e = 0; e < 3; e++) {
    const long long z = ends[e];
    if (z < 0) continue;
    const long long b1 = z / inner, b2 = z % inner;
    if (b1 > 0 && (f[kSA1] > arena_len / b1 || f[kSB1] > arena_len / b1 || f[kSC1] > arena_len / b1 || f[kST1] > arena_len / b1))
      return CXK_FAILURE;
    if (b2 > 0 && (f[kSA2] > arena_len / b2 || f[kSB2] > arena_len / b2 || f[kSC2] > arena_len / b2 || f[kST2] > arena_len / b2))
      return CXK_FAILURE;
    if (!inside(f[kOffA] + b1 * f[kSA1] + b2 * f[kSA2], extent(rows_a + (rows_a & 1), f[kLda], cols_a))) return CXK_FAILURE;
    if (!inside(f[kOffB] + b1 * f[kSB1] + b2 * f[kSB2], extent(rows_b + (rows_b & 1), f[kLdb], cols_b))) return CXK_FAILURE;
    const long long c_rel = b1 * f[kSC1] + b2 * f[kSC2];
    if (!split || ordered) {
      if (!inside(f[kOffC] + c_rel, extent(M, f[kLdc], N))) return CXK_FAILURE;
    }
    if (split) {
      if (f[kSCs] > arena_len / splits) return CXK_FAILURE;
      for (long long sp = 0; sp < splits; sp += std::max(1ll, splits - 1))
        if (!inside(f[kOffPart] + c_rel + sp * f[kSCs], extent(M, f[kLdc], N))) return CXK_FAILURE;
    }
    if (has_ct) {
      // Ct[n + m ldct + (n / ctb) sTb]: largest at n = N - 1, m = M - 1 (strides are not negative)
      const long long blocks = f[kCtb] > 0 ? (N - 1) / f[kCtb] : 0;
      if (f[kLdct] > arena_len / M || (blocks > 0 && f[kSTb] > arena_len / blocks)) return CXK_FAILURE;
      if (!inside(f[kOffCt] + b1 * f[kST1] + b2 * f[kST2], (N - 1) + (M - 1) * f[kLdct] + blocks * f[kSTb] + 1))
        return CXK_FAILURE;
    }
  }
  cxk_context scratch_ctx;  // carries the error string for CXK_TRY
  cxk_context* ctx = &scratch_ctx;
  DeviceGuard guard(device);
  DevBuf<double> dev;
  CXK_TRY(dev.alloc((size_t)arena_len));
  CXK_TRY(hipMemcpy(dev.p, arena, sizeof(double) * (size_t)arena_len, hipMemcpyHostToDevice));
  GemmArgs g{};
  g.M = (int)M;
  g.N = (int)N;
  g.K = (int)K;
  g.A = dev.p + f[kOffA];
  g.lda = f[kLda];
  g.sA1 = f[kSA1];
  g.sA2 = f[kSA2];
  g.B = dev.p + f[kOffB];
  g.ldb = f[kLdb];
  g.sB1 = f[kSB1];
  g.sB2 = f[kSB2];
  g.C = dev.p + ((split && !ordered) ? f[kOffPart] : f[kOffC]);  // raw partials: C = part, as LmiLargeSchur calls it
  g.ldc = f[kLdc];
  g.sC1 = f[kSC1];
  g.sC2 = f[kSC2];
  g.Ct = has_ct ? dev.p + f[kOffCt] : nullptr;
  g.ldct = f[kLdct];
  g.sT1 = f[kST1];
  g.sT2 = f[kST2];
  g.ctb = (int)f[kCtb];
  g.sTb = f[kSTb];
  g.inner = (int)inner;
  g.alpha = alpha;
  g.beta = beta;
  g.lower_only = f[kLower] != 0;
  g.splits = (int)splits;
  g.sCs = f[kSCs];
  cxk_host::GemmModes modes = GemmProcessModes();
  if (f[kTile]) modes.forced_tile = (int)f[kTile];
  if (f[kGeneral]) modes.force_general = true;
  cxk_host::GemmRoute r = cxk_host::GemmRoute::kGeneral;
  if (split && ordered)
    CXK_TRY(LaunchGemmSplitKWith(g, ta, tb, (int)batch, dev.p + f[kOffPart], nullptr, modes, &r));
  else
    CXK_TRY(LaunchGemmWith(g, ta, tb, (int)batch, nullptr, modes, &r));
  CXK_TRY(hipDeviceSynchronize());
  CXK_TRY(hipMemcpy(arena, dev.p, sizeof(double) * (size_t)arena_len, hipMemcpyDeviceToHost));
  if (route) {
    switch (r) {
      case cxk_host::GemmRoute::kGeneral: *route = CXK_GEMM_ROUTE_GENERAL; break;
      case cxk_host::GemmRoute::kDma16: *route = CXK_GEMM_ROUTE_DMA16; break;
      case cxk_host::GemmRoute::kDma32: *route = CXK_GEMM_ROUTE_DMA32; break;
      case cxk_host::GemmRoute::kDma128x128: *route = CXK_GEMM_ROUTE_DMA128X128; break;
      case cxk_host::GemmRoute::kDma128x64: *route = CXK_GEMM_ROUTE_DMA128X64; break;
    }
  }
  return CXK_SUCCESS;
}

int cxk_dense_top_columns(const cxk_context* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  return ctx->top_dense.on ? ctx->top_dense.args.T : 0;
}

int cxk_count_sparse_lmi(const cxk_context* ctx) { return CountOnRoute(ctx, ConeRoute::kLmiSparse); }

int cxk_count_factored_lmi(const cxk_context* ctx) {
  if (!ctx || !ctx->finalized) return -1;
  int k = 0;  // (how a constraint was added, not a choice of cxk_finalize: a host-only context counts them too)
  for (size_t i = 0; i < ctx->cons.size(); i++) k += ctx->cons[i].type == CXK_LMI && ctx->owned[i] && ctx->cons[i].factors.given;
  return k;
}

int cxk_fused_assembly(const cxk_context* ctx) { return ctx && ctx->fused_asm ? 1 : 0; }
/* 1 when assembly, factorization and solve of a KKT solve run as one launch (tree_fused.hip) */
int cxk_fused_tree(const cxk_context* ctx) { return ctx && ctx->fused_tree ? 1 : 0; }

int cxk_fused_tree_frames(const cxk_context* ctx, int* frame_a, int* frame_b) {
  if (!ctx || !frame_a || !frame_b) return CXK_FAILURE;
  *frame_a = ctx->fused_tree ? ctx->fused_sa : 0;
  *frame_b = ctx->fused_tree ? ctx->fused_sb : 0;
  return CXK_SUCCESS;
}

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
    if (g.type != CXK_LMI || g.route == ConeRoute::kLmiFactored) continue;
    const LmiAssembly how = LmiAssemblyOf(g);
    const int kind = g.route == ConeRoute::kLmiSparse ? 4 : how == LmiAssembly::kGemm ? 3 : how == LmiAssembly::kMfma ? 2 : 0;
    if (kind == which) k += (int)g.ids.size();
  }
  return k;
}

int cxk_assembly_work(const cxk_context* ctx, double* bytes, double* flops) {
  if (!ctx || !ctx->finalized) return CXK_FAILURE;
  double B = 0, F = 0;
  for (size_t i = 0; i < ctx->cons.size(); i++) {
    const ConstraintRec& c = ctx->cons[i];
    if (c.type != CXK_LMI || !ctx->owned[i]) continue;
    const double n = c.n, m = c.m;
    if (c.factors.given) {
      // Z = W F, Y = C Z, P = F' Z (lower), C W and W (C W), then the sums of the finalize kernel; bytes: F, W, C,
      // Z (written, read twice), Y, P, the two squares of the scalars, G's triangle and the three vectors
      const double R = c.factors.R;
      double terms = 0;  // sum over i >= j of r_i r_j
      for (int i = 0, below = 0; i < c.m; i++) {
        const double ri = c.factors.ptr[i + 1] - c.factors.ptr[i];
        below += (int)ri;
        terms += ri * below;
      }
      if (c.herm_d > 1) {
        // the folded Hermitian form (n = d x order): Z and Y from F0 alone, P = L(F)' Z (d planes of R x R, full),
        // 2 d + 1 flops per term of G; bytes: F0 and L(F) read once each, P's d planes
        const double d = c.herm_d;
        F += 4 * n * n * R + 2 * n * d * R * R + 4 * n * n * n + 4 * n * n + (2 * d + 1) * terms + 2 * n * R + 2 * R;
        B += 8.0 * (n * R + n * d * R + 2 * n * n + 4 * n * R + n * R + d * R * R + 4 * n * n + m * (m + 1) / 2 + 2 * m + R + m);
        continue;
      }
      F += 4 * n * n * R + n * R * (R + 1) + 4 * n * n * n + 4 * n * n + 3 * terms + 2 * n * R + 2 * R;
      B += 8.0 * (n * R + 2 * n * n + 4 * n * R + n * R + R * (R + 1) / 2 + 4 * n * n + m * (m + 1) / 2 + 2 * m + R + m);
      continue;
    }
    if (c.csr_only && c.herm_d > 0) {
      // a Hermitian constraint held by its nonzeros (cxk_add_hermitian_coo): the sums over the entry lists, a pair
      // (i, j) as first(longer) x full(shorter) -- `first` the top block row of a folded group, else the whole list --
      // at three flops a term; a C of more than 64 nonzeros leaves the pair sums for W C W (4 n^3) and sums over n^2.
      // Bytes: the entries (12 B each), W, G's triangle and the three vectors
      const bool fold = c.entries.fold;
      const int lists = c.entries.ptr[c.m + 1] - c.entries.ptr[c.m] > 64 ? c.m : c.m + 1;
      double terms = 0, firsts = 0;
      for (int a = 0; a < lists; a++) {
        const double na = c.entries.ptr[a + 1] - c.entries.ptr[a];
        firsts += fold ? na / c.herm_d : na;
        for (int b = 0; b <= a; b++) {
          const double nb = c.entries.ptr[b + 1] - c.entries.ptr[b];
          terms += (fold ? std::max(na, nb) / c.herm_d : std::max(na, nb)) * std::min(na, nb);
        }
      }
      F += 3 * terms + 4 * firsts + (lists == c.m ? 4 * n * n * n + 4 * n * n : 0);
      B += 12.0 * c.entries.ptr[lists] + 8.0 * ((lists == c.m ? 4 : 1) * n * n + m * (m + 1) / 2 + 2 * m);
      continue;
    }
    // FLOPs = 4 n^3 (m+1) + n^2 (m^2 + 3m + 4) + n m ; bytes = 8 [m n^2 + 2 n^2 + m(m+1)/2 + 2m]
    F += 4 * n * n * n * (m + 1) + n * n * (m * m + 3 * m + 4) + n * m;
    B += 8.0 * (m * n * n + 2 * n * n + m * (m + 1) / 2 + 2 * m);
  }
  if (bytes) *bytes = B;
  if (flops) *flops = F;
  return CXK_SUCCESS;
}

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
