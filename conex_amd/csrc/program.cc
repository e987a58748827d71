// CONEX_* outer C-ABI (include/conex.h) and the IPM driver on top of the device-resident
// Newton-step path (cxk_*, include/conex_kkt_hip.h).
//
// Host side only: constraint builders, argument checks, the interior-point control loop and the
// scalar mu rules.  Restates
//   interfaces/conex.cc:20-407        argument checks, copies, status codes
//   conex/cone_program.cc:78-112      Initialize
//   conex/cone_program.cc:166-224     MinimizeNormInf, ComputeMuFromDivergence, ApplyLimits
//   conex/cone_program.cc:235-552     Solve
//   conex/divergence.cc:17-110        DivergenceUpperBoundInverse and helpers
//   conex/linear_constraint.cc:14-46  PreprocessLinearInequality
//   conex/hermitian_psd.cc:249-313, linear_constraint.cc:207-228, soc_constraint.cc:305-335
//                                     UpdateLinearOperator / UpdateAffineTerm checks
// Every fp64 vector/matrix operation of the loop is a cxk_* call; per iteration only the
// scalars of cxk_step_scalars / cxk_prepare_step / cxk_weighted_slack_eigenvalues cross PCIe.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../include/conex.h"
#include "../../include/conex_kkt_hip.h"
#include "mu_rule.h"
#include "solve_route.h"

namespace {

#define CONEX_DEMAND(x, msg)                                         \
  if (!(x)) {                                                        \
    fprintf(stderr, "%s line %d: %s\n", __FILE__, __LINE__, msg);    \
    return 1;                                                        \
  }

int g_verbose = -1;
bool Verbose() {
  if (g_verbose < 0) {
    const char* e = getenv("CONEX_VERBOSE");
    g_verbose = (e && *e && *e != '0') ? 1 : 0;
  }
  return g_verbose == 1;
}

enum ConeKind { kLmi, kLinear, kSoc, kQuadCost, kEquality, kQuadCone };

struct Cone {
  ConeKind kind = kLmi;
  int order = 0;        // LMI n ; linear rows ; SOC n (vectors in R^{n+1})
  int hyper = 1;        // LMI only: 1, 2, 4, 8
  // true: HermitianPsdConstraint<T> (CONEX_NewLinearMatrixInequality, conex.cc:286-318);
  // false: DenseLMIConstraint (CONEX_Add{Dense,Sparse}LMIConstraint, conex.cc:137-188)
  bool hermitian = false;
  std::vector<int> vars;                   // clique (variable ids) fixed at creation time
  // LMI: mats[v] = hyper planes of n*n (col-major); affine likewise. Linear/SOC: dense A (rows x cols)
  std::vector<std::vector<double>> mats;
  std::vector<double> affine;
  int cols = 0;         // linear / SOC: number of columns currently allocated in `A`
  std::vector<double> A;
  std::vector<double> c;
  std::vector<double> Q;  // kQuadCone: inner-product matrix (order x order), empty = identity
  // kQuadCone added by CONEX_HIP_AddStructuredQuadraticConstraint: Q = S + F diag(sigma) F' by its parts (S in CSR as
  // q_ptr / q_col / q_val, q_ptr empty: no sparse part; F order x q_rank in `F`, `sigma`); Q stays empty and is never formed
  bool structured_q = false;
  int q_rank = 0;
  std::vector<int> q_ptr, q_col;
  std::vector<double> q_val;
  // kQuadCone added by CONEX_HIP_AddSparseQuadraticConstraint: the (order + 1) x cols matrix by its nonzeros in CSR
  // (row 0 is A0), columns ascending within a row, no explicit zeros; `A` stays empty and is never formed
  bool sparse_a = false;
  std::vector<int> a_ptr, a_col;
  std::vector<double> a_val;
  // kLmi added by CONEX_HIP_AddFactoredLMIConstraint: A_v = sum_k sigma[k] f_k f_k', k in rank_ptr[v] .. rank_ptr[v + 1] - 1,
  // f_k the columns of F (order x rank_ptr.back()); `mats` stays empty, `affine` holds C.  Added by
  // CONEX_HIP_AddFactoredHermitianConstraint (`hermitian` set): F and `affine` hold `hyper` planes
  bool factored = false;
  std::vector<double> F, sigma;
  std::vector<int> rank_ptr;
  // kLmi added by CONEX_HIP_AddLMIConstraintFromEntries: the lower triangles of A_v (list v) and of the affine term
  // (list vars.size()) as e_ptr / e_row / e_col / e_val; `mats` and `affine` stay empty: the matrices are never formed.
  // Added by CONEX_HIP_AddHermitianConstraintFromEntries (`hermitian` set): e_val holds `hyper` planes per entry
  bool from_entries = false;
  std::vector<int> e_ptr, e_row, e_col;
  std::vector<double> e_val;
};

struct Program {
  unsigned magic = 0xC0DEC0DEu;
  int num_vars = 0;
  std::vector<Cone> cones;
  bool contains_quadratic_costs = false;
  std::vector<double> linear_cost;
  // solver state
  cxk_context* ctx = nullptr;
  bool initialized = false;
  bool dirty = true;
  int device = 0;
  int reference_identity = -1;  // -1: environment (CXK_REFERENCE_QUIRKS); see CONEX_HIP_SetReferenceIdentity
  int streamed_cones = 1;       // second-order cones beyond LDS run from HBM; see CONEX_HIP_SetStreamedCones
  int tiled_linear = -1;        // linear blocks on the tiled kernels: -1 by size; see CONEX_HIP_SetTiledLinear
  int sparse_linear = -1;       // linear blocks from their nonzeros: -1 by pattern; see CONEX_HIP_SetSparseLinear
  int sparse_soc = 0;           // second-order cones from their nonzeros: 0 none; see CONEX_HIP_SetSparseSoc
  int sparse_affine = -2;       // affine terms of sparse LMIs from their nonzeros: -2 nothing said; see CONEX_HIP_SetSparseAffine
  int sparse_fold = -2;         // folded sums of sparse Hermitian LMIs: -2 nothing said; see CONEX_HIP_SetSparseFold
  int streamed_quadratic = -1;  // quadratic cones held in HBM: -1 beyond LDS or by size; see CONEX_HIP_SetStreamedQuadratic
  // multi-GPU (one process per GPU, every rank builds the same program): see CONEX_HIP_SetCommunicator
  int shard_rank = 0, shard_world = 1;
  int debug_timeout_at = -1, debug_timeout_site = 0;  // CONEX_HIP_DebugFusedTimeoutAt (test hook)
  bool have_unique_id = false;
  unsigned char unique_id[128] = {0};
  cxk_allreduce_fn allreduce_fn = nullptr;
  void* allreduce_user = nullptr;
  double b_scaling = 1, c_scaling = 1;
  std::vector<double> sqrt_inv_mu;
  int num_iter = 0;
  bool stats_ready = false;
  int solved = 0, primal_infeasible = 0, dual_infeasible = 0;
  std::string why;
  ~Program() {
    if (ctx) cxk_destroy(ctx);
  }
};

// SAFER_CAST_TO_Program interfaces/conex.cc:20-33
#define CAST_PROGRAM(x, prog)                                       \
  CONEX_DEMAND(x, "Program pointer is null.");                      \
  Program* prog = static_cast<Program*>(x);                         \
  CONEX_DEMAND(prog->magic == 0xC0DEC0DEu, "Program corrupted or invalid pointer.");

std::vector<int> AllVars(const Program& p) {
  std::vector<int> v(p.num_vars);
  for (int i = 0; i < p.num_vars; i++) v[i] = i;
  return v;
}

int AddCone(Program* p, Cone&& c) {
  p->cones.push_back(std::move(c));
  p->dirty = true;
  return static_cast<int>(p->cones.size()) - 1;
}

// ---------------------------------------------------------------- divergence.cc: mu_rule.h
using cxk_mu::Wse;

int RankOf(const Cone& c) {
  switch (c.kind) {
    case kLmi: return c.order;
    case kLinear: return c.order;
    case kSoc: return 2;
    case kQuadCone: return 2;  // quadratic_cone_constraint.h:38
    default: return 0;
  }
}

// The first min(cols, m) columns of a column-major rows x cols matrix in a zero-padded rows x m one.
std::vector<double> PaddedColumns(const std::vector<double>& A, int rows, int cols, int m) {
  std::vector<double> out((size_t)rows * m, 0.0);
  std::copy(A.begin(), A.begin() + (size_t)rows * std::max(0, std::min(cols, m)), out.begin());
  return out;
}

// Upload the builder state into a fresh device context (Initialize, cone_program.cc:78-112).
int BuildContext(Program* p) {
  if (p->ctx) {
    cxk_destroy(p->ctx);
    p->ctx = nullptr;
  }
  if (cxk_create(p->num_vars, p->device, nullptr, &p->ctx) != CXK_SUCCESS) {
    fprintf(stderr, "conex: no HIP device available; this library has no CPU fallback.\n");
    return 1;
  }
  if (p->reference_identity >= 0) cxk_set_reference_identity(p->ctx, p->reference_identity);
  // the reference takes a second-order cone of any size (CONEX_NewLorentzConeConstraint makes every cone as wide
  // as the program): none is refused for its size here either
  cxk_set_streamed_cones(p->ctx, p->streamed_cones);
  if (p->tiled_linear >= 0) cxk_set_tiled_linear(p->ctx, p->tiled_linear);
  // (automatic, where the cxk_* interface defaults to never: bounds and polytopic rows are almost empty)
  cxk_set_sparse_linear(p->ctx, p->sparse_linear);
  // (never, as the cxk_* interface defaults: every program keeps its route and its bits unless asked)
  cxk_set_sparse_soc(p->ctx, p->sparse_soc);
  // (nothing said: every constraint keeps the default of the entry point it comes through)
  if (p->sparse_affine != -2) cxk_set_sparse_affine(p->ctx, p->sparse_affine);
  if (p->sparse_fold != -2) cxk_set_sparse_fold(p->ctx, p->sparse_fold);
  // (likewise no quadratic cone is refused for its size: automatic, where the cxk_* interface defaults to never)
  cxk_set_streamed_quadratic(p->ctx, p->streamed_quadratic);
  if (p->shard_world > 1) {
    if (cxk_set_shard(p->ctx, p->shard_rank, p->shard_world)) return 1;
    if (p->allreduce_fn) {
      if (cxk_comm_set_allreduce(p->ctx, p->allreduce_fn, p->allreduce_user)) return 1;
    } else if (p->have_unique_id) {
      if (cxk_comm_init_rccl(p->ctx, p->unique_id, p->shard_rank, p->shard_world)) return 1;
    } else {
      fprintf(stderr, "conex: a sharded program needs CONEX_HIP_SetCommunicator or CONEX_HIP_SetAllReduce\n");
      return 1;
    }
  }
  for (const Cone& c : p->cones) {
    int id = -1;
    const int m = static_cast<int>(c.vars.size());
    switch (c.kind) {
      case kLmi: {  // (hyper is 1 for a DenseLMIConstraint)
        if (c.factored) {  // the factors go to the device as they are: the matrices are never formed
          id = c.hermitian ? cxk_add_hermitian_factored(p->ctx, c.order, c.hyper, m, c.rank_ptr.data(), c.F.data(),
                                                        c.sigma.data(), c.affine.data(), c.vars.data())
                           : cxk_add_lmi_factored(p->ctx, c.order, m, c.rank_ptr.data(), c.F.data(), c.sigma.data(),
                                                  c.affine.data(), c.vars.data());
          break;
        }
        if (c.from_entries) {  // the lists go to the device as they are: nothing of size m n^2 is formed
          id = c.hermitian ? cxk_add_hermitian_coo(p->ctx, c.order, c.hyper, m, c.e_ptr.data(), c.e_row.data(), c.e_col.data(),
                                                   c.e_val.data(), c.vars.data())
                           : cxk_add_lmi_coo(p->ctx, c.order, m, c.e_ptr.data(), c.e_row.data(), c.e_col.data(), c.e_val.data(), c.vars.data());
          CONEX_DEMAND(id >= 0, cxk_last_error(p->ctx));
          break;
        }
        const size_t sz = (size_t)c.order * c.order * c.hyper;
        std::vector<double> A((size_t)m * sz, 0.0), C(sz, 0.0);
        for (int v = 0; v < m && v < (int)c.mats.size(); v++)
          if (!c.mats[v].empty()) std::copy(c.mats[v].begin(), c.mats[v].begin() + sz, A.begin() + v * sz);
        if (!c.affine.empty()) std::copy(c.affine.begin(), c.affine.begin() + sz, C.begin());
        id = c.hermitian ? cxk_add_hermitian(p->ctx, c.order, c.hyper, m, A.data(), C.data(), c.vars.data())
                         : cxk_add_lmi(p->ctx, c.order, m, A.data(), C.data(), c.vars.data());
        break;
      }
      case kLinear:
        id = cxk_add_linear(p->ctx, c.order, m, PaddedColumns(c.A, c.order, c.cols, m).data(), c.c.data(),
                            c.vars.data());
        break;
      case kSoc: {
        std::vector<double> cc(c.order + 1, 0.0);
        std::copy(c.c.begin(), c.c.end(), cc.begin());
        id = cxk_add_soc(p->ctx, c.order, m, PaddedColumns(c.A, c.order + 1, c.cols, m).data(), cc.data(),
                         c.vars.data());
        break;
      }
      case kQuadCost:
        id = cxk_add_static(p->ctx, m, c.A.data(), c.vars.data());
        break;
      case kQuadCone:
        if (c.sparse_a) {  // the nonzeros go to the device as they are, with whatever form Q has
          id = cxk_add_quadratic_csr(p->ctx, c.order, m, c.Q.empty() ? nullptr : c.Q.data(),
                                     c.structured_q && !c.q_ptr.empty() ? c.q_ptr.data() : nullptr, c.q_col.data(), c.q_val.data(),
                                     c.q_rank, c.q_rank > 0 ? c.F.data() : nullptr, c.q_rank > 0 ? c.sigma.data() : nullptr,
                                     c.a_ptr.data(), c.a_col.data(), c.a_val.data(), c.c.data(), c.vars.data());
          CONEX_DEMAND(id >= 0, cxk_last_error(p->ctx));
          break;
        }
        if (c.structured_q) {  // the parts go to the device as they are
          id = cxk_add_quadratic_structured(p->ctx, c.order, m, c.q_ptr.empty() ? nullptr : c.q_ptr.data(), c.q_col.data(),
                                            c.q_val.data(), c.q_rank, c.q_rank > 0 ? c.F.data() : nullptr,
                                            c.q_rank > 0 ? c.sigma.data() : nullptr, c.A.data(), c.c.data(), c.vars.data());
          CONEX_DEMAND(id >= 0, cxk_last_error(p->ctx));
          break;
        }
        id = cxk_add_quadratic(p->ctx, c.order, m, c.Q.empty() ? nullptr : c.Q.data(), c.A.data(), c.c.data(),
                               c.vars.data());
        break;
      case kEquality:
        id = cxk_add_equality(p->ctx, c.order, m, PaddedColumns(c.A, c.order, c.cols, m).data(), c.c.data(),
                              c.vars.data());
        break;
    }
    CONEX_DEMAND(id >= 0, "constraint rejected while building the device program");
  }
  CONEX_DEMAND(cxk_finalize(p->ctx) == CXK_SUCCESS, cxk_last_error(p->ctx));
  if (p->debug_timeout_at >= 0)
    CONEX_DEMAND(cxk_debug_fused_timeout_at(p->ctx, p->debug_timeout_at, p->debug_timeout_site) == CXK_SUCCESS,
                 "CONEX_HIP_DebugFusedTimeoutAt: the context makes no such whole-tree launch");
  p->dirty = false;
  return 0;
}

using cxk_mu::ApplyLimits;

#define REPORT(name, val) \
  if (Verbose()) printf(#name ": %.2e, ", (double)(val));
#define PRINTSTATUS(x) \
  if (Verbose()) printf("Status: %s\n\n", x);

struct Config {  // conex::SolverConfiguration
  int prepare_dual_variables, initialization_mode;
  double inv_sqrt_mu_max, minimum_mu, maximum_mu, divergence_upper_bound;
  int enable_line_search;
  double dinf_upper_bound;
  int final_centering_steps;
  double final_centering_tolerance;
  int initial_centering_steps_warmstart, initial_centering_steps_coldstart;
  double warmstart_abort_threshold;
  int max_iterations;
  double infeasibility_threshold, kkt_error_tolerance;
  int kkt_solver, enable_rescaling, iterative_refinement_iterations;
};

Config FromApi(const CONEX_SolverConfiguration* c) {  // interfaces/conex.cc:65-90
  Config o;
  o.prepare_dual_variables = c->prepare_dual_variables;
  o.initialization_mode = c->initialization_mode;
  o.inv_sqrt_mu_max = c->inv_sqrt_mu_max;
  o.minimum_mu = c->minimum_mu;
  o.maximum_mu = c->maximum_mu;
  o.divergence_upper_bound = c->divergence_upper_bound;
  o.enable_line_search = c->enable_line_search;
  o.dinf_upper_bound = c->dinf_upper_bound;
  o.final_centering_steps = c->final_centering_steps;
  o.final_centering_tolerance = c->final_centering_tolerance;
  o.initial_centering_steps_warmstart = c->initial_centering_steps_warmstart;
  o.initial_centering_steps_coldstart = c->initial_centering_steps_coldstart;
  o.warmstart_abort_threshold = c->warmstart_abort_threshold;
  o.max_iterations = c->max_iterations;
  o.iterative_refinement_iterations = c->iterative_refinement_iterations;
  o.infeasibility_threshold = c->infeasibility_threshold;
  o.kkt_error_tolerance = c->kkt_error_tolerance;
  o.enable_rescaling = c->enable_rescaling;
  o.kkt_solver = c->kkt_solver;
  return o;
}

// ---------------------------------------------------------------- conex::Solve cone_program.cc:235-533
// SolveProgram at the end of this section reads as the list of its stages.  Which device calls an
// iteration makes is decided once per iteration by cxk_route::Choose (solve_route.h).

using Clock = std::chrono::steady_clock;
double MsSince(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// How a stage, and with it an iteration, ends.
enum class Outcome {
  kNext,           // go on: the next stage, the next iteration
  kRedo,           // the same iteration again, from the state it started with
  kRetryCold,      // the warm start was aborted: counts as an iteration, the next one starts from identity
  kCenteringDone,  // stop: the final centering budget is exhausted
  kConverged,      // stop
  kFailed,         // CONEX_Maximize returns 0
  kFatal           // CONEX_Maximize returns 1, as the reference's CONEX_DEMAND does
};

// What a solve fixes before its first iteration, and its instruments.
struct Solve {
  Program* p;
  const Config& cfg;
  bool timers;   // CONEX_ENABLE_TIMER=1 (the reference's compile-time macro of debug_macros.h:18-52 as an
                 // environment switch): device time of the four phases the reference brackets, per iteration
  bool profile;  // CONEX_PROFILE=1: wall time of set-up, of the iteration loop and of the host side of each
                 // device call on stderr
  cxk_context* ctx = nullptr;
  int N = 0, rankK = 0, initial_centering_steps = 0;
  double phase_prev[CXK_PHASE_COUNT] = {0, 0, 0, 0, 0};
  double prof_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  Clock::time_point t_loop;
};
enum ProfSlot { kProfAssemble, kProfFactorAsync, kProfMu, kProfFactorStatus, kProfDirection, kProfPrepare,
                kProfScalars, kProfTakeStep };
const char* const kProfName[8] = {"assemble", "factor_async", "mu selection", "factor_status",
                                  "newton_direction", "prepare_step", "step_scalars", "take_step"};

// call(), its host wall time added to the slot under CONEX_PROFILE
template <class F>
inline auto Timed(Solve& sv, ProfSlot slot, F&& call) -> decltype(call()) {
  if (!sv.profile) return call();
  const auto t0 = Clock::now();
  const auto r = call();
  sv.prof_ms[slot] += MsSince(t0);
  return r;
}

// Everything the loop carries from one iteration to the next.  An iteration starts from a copy;
// redoing it is assigning the copy back.
struct Iterate {
  double inv_sqrt_mu = 0, inv_sqrt_mu_max = 0;
  double b_scaling = 1, c_scaling = 1;  // Program's, written back where SolveProgram leaves the loop
  int centering_steps = 0;
  bool warmstart_aborted = false;
  double cx = 1, by = -1, kkt_error = 0;
};

// What one iteration's stages hand each other.
struct Pass {
  int i = 0;
  bool warm_first = false;  // first iteration of a warm start: it may yet be aborted
  bool initial_centering = false, final_centering = false, update_mu = false;
  cxk_route::Route route{};
  double selected = -1;  // host mu selection: the new inv_sqrt_mu, or not positive
  double info[2] = {0, 0};
  int took_step = 0;
};

bool EnvSwitchOn(const char* name) {
  const char* e = getenv(name);
  return e != nullptr && atoi(e) != 0;
}

// Initialize :78-112, then context, solver mode, refinement, timers, cost and the first iterate
Outcome SetUp(Solve& sv, Iterate* st) {
  Program* p = sv.p;
  const Config& cfg = sv.cfg;
  const auto t_start = Clock::now();
  if (!p->initialized || p->dirty || cfg.initialization_mode == 0) {
    if (p->dirty || !p->ctx) {
      // "Sparsity Analysis(us)" of cone_program.cc:95-109: symbolic analysis + upload, host wall time
      const auto t_sp = Clock::now();
      if (BuildContext(p)) return Outcome::kFailed;
      if (sv.timers)
        printf("Sparsity Analysis(us): %.0f, \n",
               std::chrono::duration<double, std::micro>(Clock::now() - t_sp).count());
    }
    if (cfg.initialization_mode == 0) {
      p->b_scaling = 1;
      p->c_scaling = 1;
      if (cxk_set_identity(p->ctx)) return Outcome::kFailed;
    }
    p->initialized = true;
  }
  cxk_context* ctx = sv.ctx = p->ctx;
  cxk_phase_timers(ctx, sv.timers ? 1 : 0);
  if (cxk_set_solver_mode(ctx, cfg.kkt_solver)) return Outcome::kFailed;  // solver->SetSolverMode(config.kkt_solver) :305
  if (sv.timers) cxk_phase_read(ctx, sv.phase_prev, 1);  // start this solve's phase totals from zero
  for (int k = 0; k < CXK_PHASE_COUNT; k++) sv.phase_prev[k] = 0;
  // solver.SetIterativeRefinementIterations(config.iterative_refinement_iterations)
  if (cxk_set_iterative_refinement(ctx, cfg.iterative_refinement_iterations > 0 ? cfg.iterative_refinement_iterations : 0))
    return Outcome::kFailed;
  if (sv.profile) fprintf(stderr, "conex profile: set-up (symbolic analysis, plans, upload) %.2f ms\n", MsSince(t_start));
  sv.t_loop = Clock::now();
  p->sqrt_inv_mu.assign(std::max(cfg.max_iterations, 1), 0.0);
  p->num_iter = 0;
  p->stats_ready = true;
  if (Verbose()) printf("\n");

  sv.N = cxk_system_size(ctx);
  std::vector<double> bin(p->num_vars);
  for (int i = 0; i < p->num_vars; i++) bin[i] = -p->linear_cost[i];
  if (cxk_set_cost(ctx, bin.data())) return Outcome::kFailed;

  for (const Cone& c : p->cones) sv.rankK += RankOf(c);
  sv.initial_centering_steps = cfg.initial_centering_steps_coldstart;
  if (cfg.initialization_mode) {
    PRINTSTATUS("Warmstarting...");
    sv.initial_centering_steps = cfg.initial_centering_steps_warmstart;
  }
  st->inv_sqrt_mu_max = cfg.inv_sqrt_mu_max;
  st->b_scaling = p->b_scaling;
  st->c_scaling = p->c_scaling;
  return Outcome::kNext;
}

// Whether this iteration centers, whether it selects a new mu, and whether the centering budget ends the loop
Outcome DecideCentering(const Solve& sv, Pass* it, Iterate* st) {
  const Config& cfg = sv.cfg;
  it->initial_centering = it->i < sv.initial_centering_steps;
  it->final_centering = (st->inv_sqrt_mu >= st->inv_sqrt_mu_max) || (st->kkt_error > cfg.kkt_error_tolerance) ||
                        it->i >= (cfg.max_iterations - cfg.final_centering_steps);
  it->update_mu = (it->i == 0) || !(it->initial_centering || it->final_centering) || st->warmstart_aborted;
  st->warmstart_aborted = false;
  if (it->final_centering && st->centering_steps >= cfg.final_centering_steps) return Outcome::kCenteringDone;
  return Outcome::kNext;
}

// solver->Assemble() :338-341, and the first iteration's rescaling of b and c
Outcome AssembleAndRescale(Solve& sv, const Pass& it, Iterate* st) {
  const Config& cfg = sv.cfg;
  cxk_context* ctx = sv.ctx;
  cxk_phase_mark(ctx, CXK_PHASE_ASSEMBLE);
  if (Timed(sv, kProfAssemble, [&] { return cxk_assemble(ctx); })) return Outcome::kFailed;
  if (it.i < 1 && cfg.enable_rescaling) {
    if (cfg.initialization_mode == 0) {
      double sc[6];
      if (cxk_step_scalars(ctx, sc)) return Outcome::kFailed;
      st->b_scaling = 1.0 / (1 + std::sqrt(sc[2]));
      st->c_scaling = 1.0 / (1 + std::sqrt(sc[3]));
    }
    double mu_target = 1.0 / (st->inv_sqrt_mu_max * st->inv_sqrt_mu_max);
    mu_target *= (st->b_scaling * st->c_scaling);
    st->inv_sqrt_mu_max = 1.0 / std::sqrt(mu_target);
  }
  return Outcome::kNext;
}

// The route of this iteration.  Both capabilities are asked behind this iteration's assembly and never
// kept: a timed-out whole-tree launch switches the context to its level kernels, and the triple
// right-hand side wants the assembly still waiting to ride in the factorization.
cxk_route::Route ChooseRoute(const Solve& sv, const Pass& it) {
  cxk_route::Inputs in{};
  in.update_mu = it.update_mu;
  in.line_search = sv.cfg.enable_line_search != 0;
  in.quadratic_costs = sv.p->contains_quadratic_costs;
  in.timers = sv.timers;
  in.warm_first = it.warm_first;
  in.device_mu_supported = cxk_device_mu_supported(sv.ctx) == 1;
  in.triple_supported = cxk_triple_supported(sv.ctx) == 1;
  return cxk_route::Choose(in);
}

// solver->Factor() :360.  The LLT flag travels back with the first host round trip of this
// iteration (mu selection or PrepareStep); everything enqueued in between only overwrites
// scratch state (y, the step temporaries) -- the PrepareStep kernels of the cones that keep
// w^{1/2} in W (second-order, quadratic) and every TakeStep kernel read the flag on the device
// and leave W alone when it is set -- so acting on the flag there is equivalent.
// One upward pass serves the factorization and the first solve of the iteration: the
// right-hand side of the mu selection (ComputeMuFromDivergence) when mu is updated without a
// line search -- all three right-hand sides the Newton direction for ANY mu is a combination of
// when the device selects it --, the Newton direction itself when mu stays (its value is final
// before Factor()).
Outcome EnqueueFactorization(Solve& sv, const Pass& it, Iterate* st) {
  using cxk_route::Factor;
  cxk_context* ctx = sv.ctx;
  cxk_phase_mark(ctx, CXK_PHASE_FACTOR);  // (a fused first solve of the iteration rides in the factor sweep)
  if (it.route.factor == Factor::kDirection) {
    if (!it.initial_centering) st->centering_steps++;
    ApplyLimits(&st->inv_sqrt_mu, std::sqrt(1.0 / (1e-15 + sv.cfg.maximum_mu)), st->inv_sqrt_mu_max);
  }
  const double bs = st->b_scaling, cs = st->c_scaling, mu = st->inv_sqrt_mu;
  const int failed = Timed(sv, kProfFactorAsync, [&] {
    switch (it.route.factor) {
      case Factor::kTriple: return cxk_factor_solve_triple_async(ctx, bs, cs);
      case Factor::kSolve: return cxk_factor_solve_async(ctx, -bs, cs, 0.0);
      case Factor::kDirection: return cxk_factor_direction_async(ctx, mu, bs, cs);
      default: return cxk_factor_async(ctx);
    }
  });
  return failed ? Outcome::kFailed : Outcome::kNext;
}

// ComputeMuFromDivergence cone_program.cc:173-214
int MuFromDivergence(const Solve& sv, const Iterate& st, bool solved_already, double* out) {
  cxk_context* ctx = sv.ctx;
  // y = AQc*cs - b*bs ; SolveInPlace (already done when the factorization carried this right-hand side)
  if (!solved_already && cxk_solve_rhs(ctx, -st.b_scaling, st.c_scaling, 0.0)) return 1;
  double e4[4];
  if (cxk_weighted_slack_eigenvalues(ctx, st.c_scaling, e4)) return 1;
  Wse mp;
  mp.lmin = e4[0];
  mp.lmax = e4[1];
  mp.frob = e4[2];
  mp.trace = e4[3];
  *out = cxk_mu::SelectFromDivergence(sv.cfg.divergence_upper_bound, sv.rankK, mp);
  return 0;
}

double MuLowerBound(const Config& cfg) { return std::sqrt(1.0 / (1e-15 + cfg.maximum_mu)); }

// The selection of mu.  On the device (cxk_select_mu_async): the eigenvalue query's launch evaluates
// the rule itself, the Newton direction and PrepareStep read inv_sqrt_mu from device memory, and the
// host learns it, with everything else, from the one mailbox at the end of the iteration.  On the
// host: it->selected, which AdoptMu takes once the factorization is known to have succeeded.
Outcome SelectMu(Solve& sv, Pass* it, const Iterate& st) {
  using cxk_route::Mu;
  const Config& cfg = sv.cfg;
  cxk_context* ctx = sv.ctx;
  if (it->route.mu == Mu::kKept) return Outcome::kNext;
  cxk_phase_mark(ctx, CXK_PHASE_OTHER);  // mu selection: untimed in the reference
  if (it->route.mu == Mu::kDevice) {
    const int failed = Timed(sv, kProfMu, [&] {
      return cxk_select_mu_async(ctx, st.c_scaling, cfg.divergence_upper_bound, sv.rankK, st.inv_sqrt_mu,
                                 MuLowerBound(cfg), st.inv_sqrt_mu_max);
    });
    return failed ? Outcome::kFailed : Outcome::kNext;
  }
  double temp = -1;
  if (cfg.enable_line_search) {  // cone_program.cc:376-384
    if (cxk_line_search(ctx, cfg.dinf_upper_bound, st.b_scaling, st.c_scaling, &temp)) return Outcome::kFailed;
    if (temp < 0) temp = st.inv_sqrt_mu;
  }
  if (temp < 0) {
    if (sv.p->contains_quadratic_costs) {
      fprintf(stderr, "%s line %d: Solver terminating with error: line-search failed.\n", __FILE__, __LINE__);
      return Outcome::kFatal;
    }
    if (Timed(sv, kProfMu, [&] { return MuFromDivergence(sv, st, it->route.mu_solve_done, &temp); }))
      return Outcome::kFailed;
  }
  it->selected = temp;
  return Outcome::kNext;
}

// :386-392 the host's selection, or half the current value; the limits (on the device: part of the rule)
void AdoptMu(const Solve& sv, const Pass& it, Iterate* st) {
  using cxk_route::Mu;
  if (it.route.mu == Mu::kHost) {
    if (it.selected > 0)
      st->inv_sqrt_mu = it.selected;
    else
      st->inv_sqrt_mu *= .5;
  }
  if (it.route.mu != Mu::kDevice) ApplyLimits(&st->inv_sqrt_mu, MuLowerBound(sv.cfg), st->inv_sqrt_mu_max);
}

// What became of this iteration's factorization.  Called once per iteration, behind the host round
// trip the route names (free there: the stream has been waited for).
Outcome ReadFactorOutcome(Solve& sv, const Pass& it, Iterate* st) {
  cxk_context* ctx = sv.ctx;
  int ok = 0;
  if (Timed(sv, kProfFactorStatus, [&] { return cxk_factor_status(ctx, &ok); })) return Outcome::kFailed;
  if (ok) return Outcome::kNext;
  // a wait inside the whole-tree launch ran out (shared device): nothing wrong with the matrix,
  // the context has switched to its level kernels -- the same iteration again (W is untouched:
  // every kernel that would have changed it looked at the failure flag first)
  if (cxk_fused_tree_timed_out(ctx) == 1) return Outcome::kRedo;
  if (it.warm_first) {
    PRINTSTATUS("Aborting warmstart...");
    cxk_set_identity(ctx);
    st->warmstart_aborted = true;
    return Outcome::kRetryCold;
  }
  sv.p->solved = 0;
  PRINTSTATUS("Factorization failed.");
  return Outcome::kFailed;
}

// The Newton direction :409-413 where the factorization did not carry it, and the step scalars
Outcome NewtonDirection(Solve& sv, const Pass& it, const Iterate& st) {
  using cxk_route::Direction;
  cxk_context* ctx = sv.ctx;
  cxk_phase_mark(ctx, CXK_PHASE_SOLVE);
  if (it.route.direction == Direction::kDeviceMu) {
    if (Timed(sv, kProfDirection, [&] { return cxk_newton_direction_device_mu(ctx, st.b_scaling, st.c_scaling); }))
      return Outcome::kFailed;
  } else if (it.route.direction == Direction::kHost) {
    if (Timed(sv, kProfDirection,
              [&] { return cxk_newton_direction(ctx, st.inv_sqrt_mu, st.b_scaling, st.c_scaling); }))
      return Outcome::kFailed;
  }
  // by / cx of :439-446 need y only: same round trip
  if (Timed(sv, kProfScalars, [&] { return cxk_step_scalars_async(ctx); })) return Outcome::kFailed;
  return Outcome::kNext;
}

// PrepareStep :417.  Where the route allows, TakeStep is enqueued behind it with the step rule of
// :417-418 evaluated on the device: the host round trip no longer separates them.
Outcome PrepareStep(Solve& sv, Pass* it, Iterate* st) {
  using Call = cxk_route::Step;
  cxk_context* ctx = sv.ctx;
  const double e_weight = 1, c_weight = st->inv_sqrt_mu * st->c_scaling;
  cxk_phase_mark(ctx, CXK_PHASE_UPDATE);
  const int failed = Timed(sv, kProfPrepare, [&] {
    switch (it->route.step) {
      case Call::kPrepareTakeDeviceMu:  // (the host learns the device's inv_sqrt_mu here)
        return cxk_prepare_take_step_device_mu(ctx, st->c_scaling, e_weight, it->info, &it->took_step,
                                               &st->inv_sqrt_mu);
      case Call::kPrepareTake: return cxk_prepare_take_step(ctx, c_weight, e_weight, it->info, &it->took_step);
      default: return cxk_prepare_step(ctx, 0, c_weight, e_weight, it->info);
    }
  });
  return failed ? Outcome::kFailed : Outcome::kNext;
}

// The step scalars, then TakeStep :418-436 where PrepareStep's launch has not taken it -- or, on the first
// iteration of a warm start that is too far from the central path, a cold start instead of the step
Outcome TakeStep(Solve& sv, const Pass& it, Iterate* st, double sc[6]) {
  cxk_context* ctx = sv.ctx;
  double step_size = 2.0 / (it.info[1] * it.info[1]);
  if (step_size > 1) step_size = 1;
  if (Timed(sv, kProfScalars, [&] { return cxk_step_scalars(ctx, sc); })) return Outcome::kFailed;
  if (it.warm_first && it.info[1] >= sv.cfg.warmstart_abort_threshold) {
    PRINTSTATUS("Aborting warmstart...");
    cxk_set_identity(ctx);
    st->warmstart_aborted = true;
  } else if (!it.took_step) {
    if (Timed(sv, kProfTakeStep, [&] { return cxk_take_step(ctx, 0, 1.0, step_size); })) return Outcome::kFailed;
  }
  return Outcome::kNext;
}

// The iteration's line of the log, its statistics, and whether the loop has converged :439-470
Outcome Report(Solve& sv, const Pass& it, const double sc[6], Iterate* st) {
  Program* p = sv.p;
  cxk_phase_mark(sv.ctx, CXK_PHASE_OTHER);
  if (sv.timers) {  // "Assemble(us): 12, Factor(us): 40, ..." as the reference's END_TIMER prints them
    double us[CXK_PHASE_COUNT];
    if (cxk_phase_read(sv.ctx, us, 0) == CXK_SUCCESS) {
      static const char* const names[4] = {"Assemble", "Factor", "Solve", "Update"};
      for (int k = 0; k < 4; k++) printf("%s(us): %.0f, ", names[k], us[k] - sv.phase_prev[k]);
      for (int k = 0; k < CXK_PHASE_COUNT; k++) sv.phase_prev[k] = us[k];
    }
  }
  const double inv_sqrt_mu = st->inv_sqrt_mu, b_scaling = st->b_scaling, c_scaling = st->c_scaling;
  const double d_2 = std::sqrt(std::fabs(it.info[0]));
  const double d_inf = std::fabs(it.info[1]);
  st->by = sc[0] * 1.0 / (inv_sqrt_mu * c_scaling);
  st->cx = 2 * sc[4] + sc[1] - inv_sqrt_mu * sc[5] * c_scaling;
  st->cx /= (inv_sqrt_mu * b_scaling);
  double mu = 1.0 / inv_sqrt_mu;
  mu *= mu;
  const double s_dot_x = mu * (sv.rankK - d_2 * d_2) / (b_scaling * c_scaling);
  mu = mu / (c_scaling * b_scaling);
  REPORT(mu, mu);
  REPORT(d_2, d_2);
  REPORT(d_inf, d_inf);
  if (!p->contains_quadratic_costs) {
    REPORT(by, st->by);
    REPORT(cx, st->cx);
    st->kkt_error = std::fabs(st->cx - st->by - s_dot_x) / s_dot_x;
    REPORT(kkt_error, st->kkt_error);
  }
  p->num_iter = it.i + 1;
  p->sqrt_inv_mu[it.i] = inv_sqrt_mu;
  if (Verbose()) printf("\n");
  if ((it.final_centering || inv_sqrt_mu >= st->inv_sqrt_mu_max) && d_inf <= sv.cfg.final_centering_tolerance)
    return Outcome::kConverged;
  return Outcome::kNext;
}

// One iteration of :330-470 on the route chosen behind its assembly
Outcome Iteration(Solve& sv, int i, Iterate* st) {
  using cxk_route::OutcomeRead;
  Pass it;
  it.i = i;
  it.warm_first = i == 0 && sv.cfg.initialization_mode == 1;
  if (Verbose()) printf(i < 10 ? "i:  %d, " : "i: %d, ", i);
  Outcome o;
  if ((o = DecideCentering(sv, &it, st)) != Outcome::kNext) return o;
  if ((o = AssembleAndRescale(sv, it, st)) != Outcome::kNext) return o;
  it.route = ChooseRoute(sv, it);
  if ((o = EnqueueFactorization(sv, it, st)) != Outcome::kNext) return o;
  if ((o = SelectMu(sv, &it, *st)) != Outcome::kNext) return o;
  if (it.route.outcome_read == OutcomeRead::kAfterMuSelection &&
      (o = ReadFactorOutcome(sv, it, st)) != Outcome::kNext)
    return o;
  AdoptMu(sv, it, st);
  if ((o = NewtonDirection(sv, it, *st)) != Outcome::kNext) return o;
  if ((o = PrepareStep(sv, &it, st)) != Outcome::kNext) return o;
  if (it.route.outcome_read == OutcomeRead::kAfterPrepare &&
      (o = ReadFactorOutcome(sv, it, st)) != Outcome::kNext)
    return o;
  double sc[6];
  if ((o = TakeStep(sv, it, st, sc)) != Outcome::kNext) return o;
  return Report(sv, it, sc, st);
}

// Behind the loop :472-533: y, the infeasibility flags, the dual variables, the status line
Outcome WrapUp(Solve& sv, const Iterate& st, bool max_iters_reached, double* yout) {
  Program* p = sv.p;
  const Config& cfg = sv.cfg;
  cxk_context* ctx = sv.ctx;
  const int m = p->num_vars;
  if (sv.profile) fprintf(stderr, "conex profile: loop left after %.2f ms\n", MsSince(sv.t_loop));
  std::vector<double> y(sv.N, 0.0);
  if (cxk_get_y(ctx, y.data())) return Outcome::kFailed;
  for (int i = 0; i < m; i++) yout[i] = y[i];
  if (sv.profile) {
    fprintf(stderr, "conex profile: %d iterations in %.2f ms (%.3f ms each)\n", p->num_iter, MsSince(sv.t_loop),
            MsSince(sv.t_loop) / std::max(p->num_iter, 1));
    for (int k = 0; k < 8; k++)
      fprintf(stderr, "conex profile:   host time in %-18s %.3f ms per iteration\n", kProfName[k],
              sv.prof_ms[k] / std::max(p->num_iter, 1));
  }
  double mu = 1.0 / st.inv_sqrt_mu;
  mu *= mu;
  if (mu > cfg.infeasibility_threshold) {
    PRINTSTATUS("Infeasible Or Unbounded!!.");
    p->solved = 0;
    p->primal_infeasible = st.cx * st.inv_sqrt_mu <= -.5;
    p->dual_infeasible = st.by * st.inv_sqrt_mu >= .5;
  } else {
    p->solved = 1;
  }
  if (cfg.prepare_dual_variables) {  // :500-516
    int ok = 0;
    if (cxk_assemble(ctx) || cxk_factor(ctx, &ok)) return Outcome::kFailed;
    if (cxk_solve_rhs(ctx, st.inv_sqrt_mu * st.b_scaling, 0.0, -1.0)) return Outcome::kFailed;
    double info[2];
    if (cxk_prepare_step(ctx, 1, 0.0, 0.0, info)) return Outcome::kFailed;
  }
  if (p->solved) {
    for (int i = 0; i < m; i++) yout[i] /= st.inv_sqrt_mu;
    for (int i = 0; i < m; i++) yout[i] /= st.c_scaling;
    if (max_iters_reached) {
      p->solved = 0;
      PRINTSTATUS("Terminating at maximum iteration limit.");
    } else {
      PRINTSTATUS("Solved.");
    }
  }
  return Outcome::kNext;
}

// conex::Solve cone_program.cc:235-533. Returns the solved flag (1 = solved).
int SolveProgram(Program* p, const Config& cfg, double* yout) {
  if (p->contains_quadratic_costs && !(cfg.enable_line_search && !cfg.enable_rescaling)) {
    fprintf(stderr, "%s line %d: %s\n", __FILE__, __LINE__,
            "Must enable line search and disable rescaling for problems with quadratic costs.");
    return 1;  // the reference's CONEX_DEMAND returns 1 here too
  }
  p->solved = 0;
  p->primal_infeasible = 0;
  p->dual_infeasible = 0;
  if (p->cones.empty()) {  // empty program :265-270
    for (int i = 0; i < p->num_vars; i++) yout[i] = -p->linear_cost[i] * std::numeric_limits<double>::infinity();
    return 0;
  }
  Solve sv{p, cfg, EnvSwitchOn("CONEX_ENABLE_TIMER"), getenv("CONEX_PROFILE") != nullptr};
  Iterate st;
  if (SetUp(sv, &st) != Outcome::kNext) return 0;

  int i = 0;
  Outcome o = Outcome::kNext;  // (still kNext behind the loop: it ran out of iterations)
  while (o == Outcome::kNext && i < cfg.max_iterations) {
    const Iterate start = st;
    o = Iteration(sv, i, &st);
    if (o == Outcome::kRedo) {
      st = start;
      o = Outcome::kNext;
    } else if (o == Outcome::kRetryCold) {
      i++;
      o = Outcome::kNext;
    } else if (o == Outcome::kNext) {
      i++;
    }
  }
  p->b_scaling = st.b_scaling;
  p->c_scaling = st.c_scaling;
  if (o == Outcome::kFatal) return 1;
  if (o == Outcome::kFailed) return 0;
  const bool max_iters_reached =
      o == Outcome::kNext || (o == Outcome::kCenteringDone && i >= cfg.max_iterations - 1);
  if (WrapUp(sv, st, max_iters_reached, yout) != Outcome::kNext) return 0;
  return p->solved;
}

}  // namespace

// =========================================================================== C-ABI
extern "C" {

void* CONEX_CreateConeProgram() { return new Program(); }

void CONEX_DeleteConeProgram(void* prog) { delete static_cast<Program*>(prog); }

CONEX_STATUS CONEX_SetNumberOfVariables(void* x, int number_of_variables) {
  CONEX_DEMAND(number_of_variables >= 1, "Number of variables must be > 0.");
  CAST_PROGRAM(x, p);
  CONEX_DEMAND(p->num_vars == 0, "Number of variables already set.");
  p->num_vars = number_of_variables;
  p->linear_cost.assign(number_of_variables, 0.0);
  p->dirty = true;
  return CONEX_SUCCESS;
}

int CONEX_AddDenseLMIConstraint(void* x, const double* A, int Ar, int Ac, int m, const double* c,
                                int cr, int cc) {
  Program* p = static_cast<Program*>(x);
  if (!p || Ar != Ac || Ar != cr || cc != cr || !A || !c) return -1;
  if (p->num_vars == 0) {  // Program(0) + dense constraint: the reference sizes by the clique
    p->num_vars = m;
    p->linear_cost.assign(m, 0.0);
  }
  Cone k;
  k.kind = kLmi;
  k.order = cc;
  k.hyper = 1;
  k.vars = AllVars(*p);
  const size_t nn = (size_t)Ar * Ac;
  for (int i = 0; i < m; i++) k.mats.emplace_back(A + i * nn, A + (i + 1) * nn);
  k.affine.assign(c, c + nn);
  return AddCone(p, std::move(k));
}

int CONEX_AddSparseLMIConstraint(void* x, const double* A, int Ar, int Ac, int num_vars,
                                 const double* c, int cr, int cc, const long* vars, int vars_rows) {
  Program* p = static_cast<Program*>(x);
  if (!p || Ar != Ac || Ar != cr || cc != cr || vars_rows != num_vars || !A || !c || !vars) return -1;
  Cone k;
  k.kind = kLmi;
  k.order = cc;
  k.hyper = 1;
  std::vector<char> seen(std::max(p->num_vars, 1), 0);
  for (int i = 0; i < num_vars; i++) {  // IsUnique constraint_manager.h:11-24
    const long v = vars[i];
    if (v < 0 || v >= p->num_vars || seen[v]++) return -1;
    k.vars.push_back(static_cast<int>(v));
  }
  const size_t nn = (size_t)Ar * Ac;
  for (int i = 0; i < num_vars; i++) k.mats.emplace_back(A + i * nn, A + (i + 1) * nn);
  k.affine.assign(c, c + nn);
  return AddCone(p, std::move(k));
}

int CONEX_AddDenseLinearConstraint(void* x, const double* A, int Ar, int Ac, const double* c,
                                   int cr) {
  Program* p = static_cast<Program*>(x);
  if (!p || Ar != cr || !A || !c) return -1;
  if (p->num_vars == 0) {
    p->num_vars = Ac;
    p->linear_cost.assign(Ac, 0.0);
  }
  Cone k;
  k.kind = kLinear;
  k.order = Ar;
  k.cols = Ac;
  k.vars = AllVars(*p);
  k.A.assign(A, A + (size_t)Ar * Ac);
  k.c.assign(c, c + Ar);
  return AddCone(p, std::move(k));
}

int CONEX_AddLinearInequalities(void* x, const double* A, int Ar, int Ac, const double* lb,
                                int num_lb, const double* ub, int num_ub) {
  Program* p = static_cast<Program*>(x);
  if (!p || Ar != num_lb || Ar != num_ub) return -1;
  // PreprocessLinearInequality linear_constraint.cc:14-46
  std::vector<std::vector<double>> rows, eq_rows;
  std::vector<double> rhs, eq_rhs;
  for (int i = 0; i < Ar; i++) {
    double n2 = 0;
    for (int j = 0; j < Ac; j++) n2 += A[i + (size_t)j * Ar] * A[i + (size_t)j * Ar];
    if (lb[i] == ub[i]) {  // equality row: scaled like the others, goes to EqualityConstraints
      const double scale = 1.0 / std::sqrt(n2 + ub[i] * ub[i]);
      std::vector<double> r(Ac);
      for (int j = 0; j < Ac; j++) r[j] = scale * A[i + (size_t)j * Ar];
      eq_rows.push_back(r);
      eq_rhs.push_back(scale * ub[i]);
      continue;
    }
    if (ub[i] < 1e8) {
      const double scale = 1.0 / std::sqrt(n2 + ub[i] * ub[i]);
      std::vector<double> r(Ac);
      for (int j = 0; j < Ac; j++) r[j] = scale * A[i + (size_t)j * Ar];
      rows.push_back(r);
      rhs.push_back(scale * ub[i]);
    }
    if (lb[i] > -1e8) {
      const double scale = 1.0 / std::sqrt(n2 + lb[i] * lb[i]);
      std::vector<double> r(Ac);
      for (int j = 0; j < Ac; j++) r[j] = -scale * A[i + (size_t)j * Ar];
      rows.push_back(r);
      rhs.push_back(-scale * lb[i]);
    }
  }
  if (!rows.empty()) {
    if (p->num_vars == 0) {
      p->num_vars = Ac;
      p->linear_cost.assign(Ac, 0.0);
    }
    Cone k;
    k.kind = kLinear;
    k.order = static_cast<int>(rows.size());
    k.cols = Ac;
    k.vars = AllVars(*p);
    k.A.assign((size_t)k.order * Ac, 0.0);
    for (int i = 0; i < k.order; i++)
      for (int j = 0; j < Ac; j++) k.A[i + (size_t)j * k.order] = rows[i][j];
    k.c = rhs;
    AddCone(p, std::move(k));
  }
  if (!eq_rows.empty()) {  // program.AddConstraint(EqualityConstraints(Aeq, beq)) conex.cc:209-211
    if (p->num_vars == 0) {
      p->num_vars = Ac;
      p->linear_cost.assign(Ac, 0.0);
    }
    Cone k;
    k.kind = kEquality;
    k.order = static_cast<int>(eq_rows.size());
    k.cols = Ac;
    k.vars = AllVars(*p);
    k.A.assign((size_t)k.order * Ac, 0.0);
    for (int i = 0; i < k.order; i++)
      for (int j = 0; j < Ac; j++) k.A[i + (size_t)j * k.order] = eq_rows[i][j];
    k.c = eq_rhs;
    AddCone(p, std::move(k));
  }
  return -1;  // interfaces/conex.cc:213-214
}

CONEX_STATUS CONEX_AddQuadraticCost(void* x, const double* A, int Ar, int Ac) {
  CAST_PROGRAM(x, p);
  CONEX_DEMAND(A && Ar == Ac, "Quadratic cost matrix must be square.");
  // NonZeroSubMat interfaces/conex.cc:44-64
  std::vector<int> vars;
  for (int i = 0; i < Ar; i++)
    if (A[i + (size_t)i * Ar] > 0) vars.push_back(i);
  const int m = static_cast<int>(vars.size());
  Cone k;
  k.kind = kQuadCost;
  k.vars = vars;
  k.A.assign((size_t)m * m, 0.0);
  for (int r = 0; r < m; r++)
    for (int c = 0; c < m; c++) {
      const double v = (A[vars[r] + (size_t)vars[c] * Ar] + A[vars[c] + (size_t)vars[r] * Ar]) / 2.0;
      k.A[r + (size_t)c * m] = v;
      k.A[c + (size_t)r * m] = v;
    }
  p->contains_quadratic_costs = true;
  AddCone(p, std::move(k));
  return CONEX_SUCCESS;  // AddQuadraticCost returns "failure = false"
}

CONEX_STATUS CONEX_NewQuadraticCost(void* x, int* constraint_id) {
  CONEX_DEMAND(constraint_id, "Received output null pointer.");
  CAST_PROGRAM(x, p);
  Cone k;
  k.kind = kQuadCost;
  k.vars = AllVars(*p);
  k.A.assign((size_t)p->num_vars * p->num_vars, 0.0);
  p->contains_quadratic_costs = true;
  *constraint_id = AddCone(p, std::move(k));
  return CONEX_SUCCESS;
}

CONEX_STATUS CONEX_NewLinearMatrixInequality(void* x, int order, int hyper_complex_dim,
                                             int* constraint_id) {
  CONEX_DEMAND(order >= 1, "Invalid LMI dimensions.");
  CONEX_DEMAND(constraint_id, "Received output null pointer.");
  CONEX_DEMAND(hyper_complex_dim == 1 || hyper_complex_dim == 2 || hyper_complex_dim == 4 ||
                   hyper_complex_dim == 8,
               "Hypercomplex dimension must be 1, 2, 4, or 8.");
  CAST_PROGRAM(x, p);
  if (hyper_complex_dim == 8)
    CONEX_DEMAND(order <= 3, "Order of octonion algebra cannot be greater than 3.");
  // (octonions: no real matrix representation -- a cone type of its own on the device, with the
  // reference's rules for it, hermitian_psd.cc:108-168: kernels_oct.hip.h)
  Cone k;
  k.kind = kLmi;
  k.order = order;
  k.hyper = hyper_complex_dim;
  k.hermitian = true;
  k.vars = AllVars(*p);
  *constraint_id = AddCone(p, std::move(k));
  return CONEX_SUCCESS;
}

CONEX_STATUS CONEX_NewLinearInequality(void* x, int num_rows, int* constraint_id) {
  CONEX_DEMAND(constraint_id, "Received output null pointer.");
  CAST_PROGRAM(x, p);
  CONEX_DEMAND(num_rows >= 1, "Number of rows must be positive.");
  Cone k;
  k.kind = kLinear;
  k.order = num_rows;
  k.cols = p->num_vars;
  k.vars = AllVars(*p);
  k.A.assign((size_t)num_rows * p->num_vars, 0.0);
  k.c.assign(num_rows, 0.0);
  *constraint_id = AddCone(p, std::move(k));
  return CONEX_SUCCESS;
}

CONEX_STATUS CONEX_NewLorentzConeConstraint(void* x, int order, int* constraint_id) {
  CONEX_DEMAND(order >= 1, "Received invalid n. Second order cone must have order (n + 1) >= 2.");
  CONEX_DEMAND(constraint_id, "Received output null pointer.");
  CAST_PROGRAM(x, p);
  Cone k;
  k.kind = kSoc;
  k.order = order;
  k.cols = 0;
  k.vars = AllVars(*p);
  k.c.assign(order + 1, 0.0);
  *constraint_id = AddCone(p, std::move(k));
  return CONEX_SUCCESS;
}

CONEX_STATUS CONEX_UpdateLinearOperator(void* x, int constraint, double value, int variable,
                                        int row, int col, int hyper_complex_dim) {
  CAST_PROGRAM(x, p);
  CONEX_DEMAND(constraint >= 0 && constraint < (int)p->cones.size(), "Invalid Constraint.");
  Cone& k = p->cones[constraint];
  const int dim = hyper_complex_dim;
  switch (k.kind) {
    case kLmi: {  // hermitian_psd.cc:249-275
      CONEX_DEMAND(!k.factored, "A constraint given by factors does not support updates of linear operator.");
      CONEX_DEMAND(!k.from_entries, "A constraint given by entries does not support updates of linear operator.");
      CONEX_DEMAND(dim >= 0 && dim < k.hyper, "Complex dimension out of bounds.");
      CONEX_DEMAND(row >= 0 && col >= 0 && row < k.order && col < k.order,
                   "Matrix dimension out of bounds.");
      CONEX_DEMAND(!(value != 0 && row == col && dim > 0),
                   "Imaginary components must be skew-symmetric.");
      CONEX_DEMAND(variable >= 0, "Indices cannot be negative.");
      // (hermitian_psd.cc:257-262 means to refuse dim >= 3 of an octonion matrix, but tests
      //  is_same<HermitianPsdConstraint<H>, Octonions>, which never holds: every plane is accepted)
      const size_t nn = (size_t)k.order * k.order;
      if ((int)k.mats.size() <= variable) k.mats.resize(variable + 1);
      if (k.mats[variable].empty()) k.mats[variable].assign(nn * k.hyper, 0.0);
      double* M = k.mats[variable].data() + nn * dim;
      M[row + (size_t)col * k.order] = value;
      M[col + (size_t)row * k.order] = dim == 0 ? value : -value;
      break;
    }
    case kLinear: {  // linear_constraint.cc:207-217
      CONEX_DEMAND(dim == 0, "Complex linear constraints not supported.");
      CONEX_DEMAND(col == 0, "Linear constraint is not matrix valued.");
      CONEX_DEMAND(row < k.order, "Row index out of bounds.");
      CONEX_DEMAND(variable >= 0 && row >= 0, "Indices cannot be negative.");
      CONEX_DEMAND(variable < k.cols, "Variable index out of bounds.");
      k.A[row + (size_t)variable * k.order] = value;
      break;
    }
    case kSoc: {  // soc_constraint.cc:314-324
      CONEX_DEMAND(dim == 0, "Complex second-order cone not supported.");
      CONEX_DEMAND(col == 0, "Second-order constraint is not matrix valued.");
      CONEX_DEMAND(row <= k.order, "Row index out of bounds.");
      CONEX_DEMAND(variable >= 0 && row >= 0, "Indices cannot be negative.");
      const int len = k.order + 1;
      if (variable >= k.cols) {  // ConservativeResizeHelper
        k.A.resize((size_t)len * (variable + 1), 0.0);
        k.cols = variable + 1;
      }
      k.A[row + (size_t)variable * len] = value;
      break;
    }
    case kQuadCost:
    case kEquality:  // constraint.h:13-18 default: not supported
      CONEX_DEMAND(false, "Constraint does not support updates of linear operator.");
    case kQuadCone:  // (as it has always been here: accepted, nothing updated)
      break;
  }
  p->dirty = true;
  return CONEX_SUCCESS;
}

CONEX_STATUS CONEX_UpdateAffineTerm(void* x, int constraint, double value, int row, int col,
                                    int hyper_complex_dim) {
  CAST_PROGRAM(x, p);
  CONEX_DEMAND(constraint >= 0 && constraint < (int)p->cones.size(), "Invalid Constraint.");
  Cone& k = p->cones[constraint];
  const int dim = hyper_complex_dim;
  switch (k.kind) {
    case kLmi: {  // hermitian_psd.cc:286-313
      CONEX_DEMAND(!k.factored, "A constraint given by factors does not support updates of affine term.");
      CONEX_DEMAND(!k.from_entries, "A constraint given by entries does not support updates of affine term.");
      CONEX_DEMAND(dim >= 0 && dim < k.hyper, "Complex dimension out of bounds.");
      CONEX_DEMAND(row >= 0 && col >= 0 && row < k.order && col < k.order,
                   "Matrix dimension out of bounds.");
      CONEX_DEMAND(!(value != 0 && row == col && dim > 0),
                   "Imaginary components must be skew-symmetric.");
      const size_t nn = (size_t)k.order * k.order;
      if (k.affine.empty()) k.affine.assign(nn * k.hyper, 0.0);
      double* M = k.affine.data() + nn * dim;
      M[row + (size_t)col * k.order] = value;
      M[col + (size_t)row * k.order] = dim == 0 ? value : -value;
      break;
    }
    case kLinear:  // linear_constraint.cc:219-228
      CONEX_DEMAND(dim == 0, "Complex linear cone not supported.");
      CONEX_DEMAND(col == 0, "Linear constraint is not matrix valued.");
      CONEX_DEMAND(row < k.order, "Row index out of bounds.");
      CONEX_DEMAND(row >= 0, "Indices cannot be negative.");
      k.c[row] = value;
      break;
    case kSoc:  // soc_constraint.cc:326-335
      CONEX_DEMAND(dim == 0, "Complex second-order cone not supported.");
      CONEX_DEMAND(col == 0, "Second-order constraint is not matrix valued.");
      CONEX_DEMAND(row <= k.order, "Row index out of bounds.");
      CONEX_DEMAND(row >= 0, "Indices cannot be negative.");
      k.c[row] = value;
      break;
    case kQuadCost:  // quadratic_cost.cc:33-39 (dim must be 0: "hyper complex dimension")
      CONEX_DEMAND(dim == 0, "Quadratic cost must be real valued matrix.");
      {
        const int m = static_cast<int>(k.vars.size());
        CONEX_DEMAND(row >= 0 && col >= 0 && row < m && col < m, "Index out of bounds");
        k.A[row + (size_t)col * m] = value;
      }
      break;
    case kEquality:  // constraint.h:20-24 default: not supported
      CONEX_DEMAND(false, "Constraint does not support updates of affine term.");
    case kQuadCone:  // (as it has always been here: accepted, nothing updated)
      break;
  }
  p->dirty = true;
  return CONEX_SUCCESS;
}

CONEX_STATUS CONEX_UpdateQuadraticCostMatrix(void* x, int constraint, double value, int row,
                                             int col) {
  return CONEX_UpdateAffineTerm(x, constraint, value, row, col, 0);
}

void CONEX_SetDefaultOptions(CONEX_SolverConfiguration* c) {  // cone_program.h:17-38
  if (c == NULL) {
    fprintf(stderr, "Received null pointer.");
    return;
  }
  c->prepare_dual_variables = 0;
  c->initialization_mode = 0;
  c->inv_sqrt_mu_max = 1000;
  c->minimum_mu = 1e-15;
  c->maximum_mu = 1e4;
  c->divergence_upper_bound = 1;
  c->enable_line_search = 0;
  c->dinf_upper_bound = 1;
  c->final_centering_steps = 5;
  c->final_centering_tolerance = .01;
  c->initial_centering_steps_warmstart = 0;
  c->initial_centering_steps_coldstart = 0;
  c->warmstart_abort_threshold = 2;
  c->max_iterations = 25;
  c->iterative_refinement_iterations = 0;
  c->infeasibility_threshold = 1e5;
  c->kkt_error_tolerance = 1e10;
  c->enable_rescaling = 1;
  c->kkt_solver = 0;
}

int CONEX_Solve(void* x, const CONEX_SolverConfiguration* config, double* y, int yr) {
  Program* p = static_cast<Program*>(x);
  if (!p || !config || !y || yr < p->num_vars) return 0;
  return SolveProgram(p, FromApi(config), y);
}

int CONEX_Maximize(void* x, const double* b, int br, const CONEX_SolverConfiguration* config,
                   double* y, int yr) {
  Program* p = static_cast<Program*>(x);
  if (!p || !config || !y || !b) return 0;
  if (br != p->num_vars) {  // Program::AddLinearCost CONEX_DEMAND
    fprintf(stderr, "%s line %d: %s\n", __FILE__, __LINE__,
            "Cost vector dimension does not equal number of variables");
  }
  // Solve(b, prog, ...): ClearLinearCosts(); AddLinearCost(-b)
  p->linear_cost.assign(p->num_vars, 0.0);
  if (br == p->num_vars)
    for (int i = 0; i < br; i++) p->linear_cost[i] = -b[i];
  if (yr < p->num_vars) return 0;
  return SolveProgram(p, FromApi(config), y);
}

int CONEX_GetDualVariableSize(void* x, int i) {
  Program* p = static_cast<Program*>(x);
  if (!p || i < 0 || i >= (int)p->cones.size()) {
    fprintf(stderr, "%s line %d: Invalid Constraint\n", __FILE__, __LINE__);
    return 1;
  }
  const Cone& k = p->cones[i];
  switch (k.kind) {
    case kLmi: return k.order * k.order;
    case kLinear: return k.order;
    case kSoc: return k.order + 1;
    case kQuadCone: return k.order + 1;
    default: return 0;
  }
}

void CONEX_GetDualVariable(void* x, int i, double* out, int xr, int xc) {
  Program* p = static_cast<Program*>(x);
  if (!p || !p->ctx || !out) return;
  const int n = CONEX_GetDualVariableSize(x, i);
  if (n != xr * xc || n == 0) return;
  if (p->cones[i].kind == kLmi && p->cones[i].hermitian) {
    // the reference exposes the real plane of W only (hermitian_psd.cc:24-29)
    std::vector<double> planes((size_t)n * p->cones[i].hyper);
    if (cxk_get_W(p->ctx, i, planes.data())) return;
    std::copy(planes.begin(), planes.begin() + n, out);
  } else if (cxk_get_W(p->ctx, i, out)) {
    return;
  }
  // Program::GetDualVariable cone_program.h:120-134
  if (!p->primal_infeasible && p->num_iter > 0) {
    const double s = p->sqrt_inv_mu[p->num_iter - 1] * p->b_scaling;
    for (int q = 0; q < n; q++) out[q] /= s;
  }
}

void CONEX_GetIterationStats(void* x, CONEX_IterationStats* stats, int iter_num_circular) {
  if ((x == NULL) || (stats == NULL)) {
    fprintf(stderr, "Received null pointer.");
    return;
  }
  Program* p = static_cast<Program*>(x);
  if (!p->stats_ready) {
    fprintf(stderr, "No statistics available.");
    return;
  }
  int iter_num = iter_num_circular;
  if (iter_num_circular < 0) iter_num = p->num_iter + iter_num_circular;
  if ((p->num_iter <= iter_num) || (iter_num < 0)) {
    fprintf(stderr, "Specified iteration is out of bounds.");
    return;
  }
  stats->mu = 1.0 / (p->sqrt_inv_mu[iter_num] * p->sqrt_inv_mu[iter_num]);
  stats->iteration_number = iter_num;
}

/* not part of conex.h (the reference reaches these cones through its C++ API only):
 *   CONEX_HIP_AddQuadraticConstraint   prog.AddConstraint(QuadraticConstraint(Q, A, c), vars)
 *       c - A y in { (x0, x1) : x0 >= sqrt(x1' Q x1) }   (quadratic_cone_constraint.h:11-86);
 *       Q: n x n column-major or NULL (identity), A: (n + 1) x num_vars column-major, c: n + 1,
 *       vars: num_vars variable ids (NULL: all variables in order)
 *   CONEX_HIP_AddQuadraticCostEpigraph  AddQuadraticCostEpigraph(&prog, Qi, z, epigraph)
 *       (quadratic_cone_constraint.h:88-117): y[epigraph] >= 1/2 y[z]' Qi y[z] as such a cone
 * Both return the constraint id, -1 on invalid arguments. */
int CONEX_HIP_AddQuadraticConstraint(void* x, const double* Q, int n, const double* A, int Ar, int Ac,
                                     const double* c, int cr, const long* vars, int num_vars) {
  Program* p = static_cast<Program*>(x);
  if (!p || p->magic != 0xC0DEC0DEu || n < 1 || !A || !c || Ar != n + 1 || cr != n + 1 || Ac < 1) return -1;
  if (vars ? num_vars != Ac : Ac != p->num_vars) return -1;
  Cone k;
  k.kind = kQuadCone;
  k.order = n;
  k.cols = Ac;
  k.A.assign(A, A + (size_t)(n + 1) * Ac);
  k.c.assign(c, c + n + 1);
  if (Q) k.Q.assign(Q, Q + (size_t)n * n);
  if (vars) {
    for (int i = 0; i < Ac; i++) {
      if (vars[i] < 0 || vars[i] >= p->num_vars) return -1;
      k.vars.push_back((int)vars[i]);
    }
  } else {
    k.vars = AllVars(*p);
  }
  return AddCone(p, std::move(k));
}

/* not part of conex.h: the cone of CONEX_HIP_AddQuadraticConstraint with Q = S + F diag(sigma) F' given by its parts and
 * never formed (cxk_add_quadratic_structured): S n x n in CSR (q_rowptr: n + 1 from 0, q_col, q_val; both triangles, as
 * given; NULL: no sparse part), F n x rank column-major (NULL when rank = 0), sigma rank entries (NULL: all +1).  Not
 * both parts absent.  A, c and vars as for CONEX_HIP_AddQuadraticConstraint.  Returns the constraint id, -1 on
 * invalid arguments (among them a decreasing q_rowptr, a column outside [0, n), a value that is not finite). */
static bool TakeStructuredQ(Cone* k, int n, const int* q_rowptr, const int* q_col, const double* q_val, int rank, const double* F,
                            const double* sigma) {
  if (rank < 0 || (rank > 0 && !F) || (!q_rowptr && rank == 0)) return false;
  k->structured_q = true;
  k->q_rank = rank;
  if (q_rowptr) {
    if (q_rowptr[0] != 0) return false;
    for (int r = 0; r < n; r++)
      if (q_rowptr[r + 1] < q_rowptr[r]) return false;
    const int nnz = q_rowptr[n];
    if (nnz > 0 && (!q_col || !q_val)) return false;
    for (int e = 0; e < nnz; e++)
      if (q_col[e] < 0 || q_col[e] >= n || !std::isfinite(q_val[e])) return false;
    k->q_ptr.assign(q_rowptr, q_rowptr + n + 1);
    k->q_col.assign(q_col, q_col + nnz);
    k->q_val.assign(q_val, q_val + nnz);
  }
  const size_t nr = (size_t)n * rank;
  for (size_t q = 0; q < nr; q++)
    if (!std::isfinite(F[q])) return false;
  for (int j = 0; sigma && j < rank; j++)
    if (!std::isfinite(sigma[j])) return false;
  if (rank > 0) k->F.assign(F, F + nr);
  if (sigma)
    k->sigma.assign(sigma, sigma + rank);
  else
    k->sigma.assign((size_t)rank, 1.0);
  return true;
}

int CONEX_HIP_AddStructuredQuadraticConstraint(void* x, int n, const int* q_rowptr, const int* q_col, const double* q_val,
                                               int rank, const double* F, const double* sigma, const double* A, int Ar,
                                               int Ac, const double* c, int cr, const long* vars, int num_vars) {
  Program* p = static_cast<Program*>(x);
  if (!p || p->magic != 0xC0DEC0DEu || n < 1 || !A || !c || Ar != n + 1 || cr != n + 1 || Ac < 1) return -1;
  if (vars ? num_vars != Ac : Ac != p->num_vars) return -1;
  Cone k;
  k.kind = kQuadCone;
  k.order = n;
  k.cols = Ac;
  if (!TakeStructuredQ(&k, n, q_rowptr, q_col, q_val, rank, F, sigma)) return -1;
  k.A.assign(A, A + (size_t)(n + 1) * Ac);
  k.c.assign(c, c + n + 1);
  if (vars) {
    for (int i = 0; i < Ac; i++) {
      if (vars[i] < 0 || vars[i] >= p->num_vars) return -1;
      k.vars.push_back((int)vars[i]);
    }
  } else {
    k.vars = AllVars(*p);
  }
  return AddCone(p, std::move(k));
}

/* not part of conex.h: the cone of CONEX_HIP_AddQuadraticConstraint or CONEX_HIP_AddStructuredQuadraticConstraint with its
 * (n + 1) x Ac matrix given by its nonzeros and never formed (cxk_add_quadratic_csr): a_rowptr has Ar + 1 = n + 2 entries
 * from 0 (row 0 is A0), a_col the columns in [0, Ac) in any order within a row, a_val the values; explicit zeros are
 * dropped.  Q: n x n dense (Q), or its parts as CONEX_HIP_AddStructuredQuadraticConstraint takes them, or neither (the
 * identity); not both.  c and vars as there.  Returns the constraint id, -1 on invalid arguments (among them a
 * decreasing a_rowptr, a column outside [0, Ac) or named twice in a row, a value that is not finite).  The program keeps
 * the nonzeros only. */
int CONEX_HIP_AddSparseQuadraticConstraint(void* x, int n, const double* Q, const int* q_rowptr, const int* q_col,
                                           const double* q_val, int rank, const double* F, const double* sigma,
                                           const int* a_rowptr, const int* a_col, const double* a_val, int Ar, int Ac,
                                           const double* c, int cr, const long* vars, int num_vars) {
  Program* p = static_cast<Program*>(x);
  if (!p || p->magic != 0xC0DEC0DEu || n < 1 || n == INT_MAX || !a_rowptr || !c || Ar != n + 1 || cr != n + 1 || Ac < 1) return -1;
  if (vars ? num_vars != Ac : Ac != p->num_vars) return -1;
  const bool parts = q_rowptr || rank != 0 || F || sigma;
  if (Q && parts) return -1;
  Cone k;
  k.kind = kQuadCone;
  k.order = n;
  k.cols = Ac;
  k.sparse_a = true;
  if (parts && !TakeStructuredQ(&k, n, q_rowptr, q_col, q_val, rank, F, sigma)) return -1;
  if (Q) {
    if ((long long)n * n > INT_MAX) return -1;
    for (size_t q = 0; q < (size_t)n * n; q++)
      if (!std::isfinite(Q[q])) return -1;
    k.Q.assign(Q, Q + (size_t)n * n);
  }
  if (a_rowptr[0] != 0) return -1;
  for (int r = 0; r < Ar; r++)
    if (a_rowptr[r + 1] < a_rowptr[r]) return -1;
  if (a_rowptr[Ar] > 0 && (!a_col || !a_val)) return -1;
  k.a_ptr.assign((size_t)Ar + 1, 0);
  std::vector<std::pair<int, double>> row;
  for (int r = 0; r < Ar; r++) {
    row.clear();
    for (int s = a_rowptr[r]; s < a_rowptr[r + 1]; s++) {
      if (a_col[s] < 0 || a_col[s] >= Ac || !std::isfinite(a_val[s])) return -1;
      row.emplace_back(a_col[s], a_val[s]);
    }
    std::sort(row.begin(), row.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
    for (size_t s = 1; s < row.size(); s++)
      if (row[s].first == row[s - 1].first) return -1;
    for (const auto& e : row)
      if (e.second != 0.0) {
        k.a_col.push_back(e.first);
        k.a_val.push_back(e.second);
      }
    k.a_ptr[(size_t)r + 1] = (int)k.a_col.size();
  }
  for (int r = 0; r <= n; r++)
    if (!std::isfinite(c[r])) return -1;
  k.c.assign(c, c + n + 1);
  if (vars) {
    for (int i = 0; i < Ac; i++) {
      if (vars[i] < 0 || vars[i] >= p->num_vars) return -1;
      k.vars.push_back((int)vars[i]);
    }
  } else {
    k.vars = AllVars(*p);
  }
  return AddCone(p, std::move(k));
}

/* not part of conex.h: a DenseLMIConstraint whose matrices are low-rank and given by their factors,
 *   A_v = sum_k sigma[k] f_k f_k',  k = rank_ptr[v] .. rank_ptr[v + 1] - 1,  v < num_vars,
 * f_k the columns of F (n x R column-major, R = rank_ptr[num_vars]); sigma NULL = all +1; c the n x n affine term
 * (symmetric); vars: num_vars variable ids (NULL: all variables in order).  The matrices are never formed
 * (cxk_add_lmi_factored).  CONEX_UpdateLinearOperator and CONEX_UpdateAffineTerm fail on such a constraint.
 * Returns the constraint id, -1 on invalid arguments. */
int CONEX_HIP_AddFactoredLMIConstraint(void* x, int n, const double* F, int R, const double* sigma, const int* rank_ptr,
                                       int num_vars, const double* c, const long* vars) {
  Program* p = static_cast<Program*>(x);
  if (!p || p->magic != 0xC0DEC0DEu || n < 1 || R < 0 || num_vars < 0 || !rank_ptr || !c || (R > 0 && !F)) return -1;
  if (vars ? false : num_vars != p->num_vars) return -1;
  if (rank_ptr[0] != 0 || rank_ptr[num_vars] != R) return -1;
  for (int v = 0; v < num_vars; v++)
    if (rank_ptr[v + 1] < rank_ptr[v]) return -1;
  const size_t nn = (size_t)n * n, nr = (size_t)n * R;
  for (size_t q = 0; q < nr; q++)
    if (!std::isfinite(F[q])) return -1;
  for (int k = 0; sigma && k < R; k++)
    if (!std::isfinite(sigma[k])) return -1;
  for (int col = 0; col < n; col++)
    for (int row = col; row < n; row++)
      if (!std::isfinite(c[row + (size_t)col * n]) || c[row + (size_t)col * n] != c[col + (size_t)row * n]) return -1;
  Cone k;
  k.kind = kLmi;
  k.order = n;
  k.factored = true;
  k.F.assign(F, F + nr);
  if (sigma)
    k.sigma.assign(sigma, sigma + R);
  else
    k.sigma.assign((size_t)R, 1.0);
  k.rank_ptr.assign(rank_ptr, rank_ptr + num_vars + 1);
  k.affine.assign(c, c + nn);
  if (vars) {
    for (int i = 0; i < num_vars; i++) {
      if (vars[i] < 0 || vars[i] >= p->num_vars) return -1;
      k.vars.push_back((int)vars[i]);
    }
  } else {
    k.vars = AllVars(*p);
  }
  return AddCone(p, std::move(k));
}

/* not part of conex.h: a DenseLMIConstraint whose matrices are sparse and given by their entries: list v < num_vars,
 * ptr[v] .. ptr[v + 1] - 1, holds A_v and list num_vars the affine term, as (row, col, val) with row >= col (the lower
 * triangle; the matrices are its symmetric completion; entries in any order, explicit zeros dropped, an empty list is
 * the zero matrix); vars: num_vars variable ids (NULL: all variables in order).  The matrices are never formed
 * (cxk_add_lmi_coo): a program with an LMI of order n over m variables holds its nonzeros and one n x n square, not
 * m n^2 doubles.  CONEX_UpdateLinearOperator and CONEX_UpdateAffineTerm fail on such a constraint;
 * CONEX_GetDualVariable works as for any LMI.  Returns the constraint id, -1 on invalid arguments (a position named
 * twice in a list is found when the program is initialized). */
int CONEX_HIP_AddLMIConstraintFromEntries(void* x, int n, const int* ptr, const int* row, const int* col, const double* val,
                                          int num_vars, const long* vars) {
  Program* p = static_cast<Program*>(x);
  if (!p || p->magic != 0xC0DEC0DEu || n < 1 || n > 32767 || num_vars < 0 || num_vars > 32767 || !ptr) return -1;
  if (vars ? false : num_vars != p->num_vars) return -1;
  if (ptr[0] != 0) return -1;
  for (int v = 0; v <= num_vars; v++)
    if (ptr[v + 1] < ptr[v]) return -1;
  const int nz = ptr[num_vars + 1];
  if (nz > 0 && (!row || !col || !val)) return -1;
  for (int e = 0; e < nz; e++)
    if (col[e] < 0 || row[e] < col[e] || row[e] >= n || !std::isfinite(val[e])) return -1;
  Cone k;
  k.kind = kLmi;
  k.order = n;
  k.from_entries = true;
  k.e_ptr.assign(ptr, ptr + num_vars + 2);
  k.e_row.assign(row, row + nz);
  k.e_col.assign(col, col + nz);
  k.e_val.assign(val, val + nz);
  if (vars) {
    for (int i = 0; i < num_vars; i++) {
      if (vars[i] < 0 || vars[i] >= p->num_vars) return -1;
      k.vars.push_back((int)vars[i]);
    }
  } else {
    k.vars = AllVars(*p);
  }
  return AddCone(p, std::move(k));
}

/* not part of conex.h: a HermitianPsdConstraint over R / C / H (d = 1, 2, 4) whose matrices are sparse and given by
 * their entries: the lists as for CONEX_HIP_AddLMIConstraintFromEntries (list v < num_vars holds A_v, list num_vars the
 * affine term, row >= col), the value of entry e being the d planes val[d e .. d e + d - 1] (d = 2: the memory of a
 * complex double); the matrices are the Hermitian completion of the lower triangle, so a diagonal entry is real (its
 * planes 1 .. d - 1 are zero).  Neither the matrices nor their real representations are formed
 * (cxk_add_hermitian_coo).  CONEX_UpdateLinearOperator and CONEX_UpdateAffineTerm fail on such a constraint;
 * CONEX_GetDualVariable gives the real plane, as for every Hermitian constraint.  Returns the constraint id, -1 on
 * invalid arguments (a position named twice in a list is found when the program is initialized). */
int CONEX_HIP_AddHermitianConstraintFromEntries(void* x, int n, int d, const int* ptr, const int* row, const int* col,
                                                const double* val, int num_vars, const long* vars) {
  Program* p = static_cast<Program*>(x);
  if (!p || p->magic != 0xC0DEC0DEu || n < 1 || num_vars < 0 || num_vars > 32767 || !ptr) return -1;
  if (d != 1 && d != 2 && d != 4) return -1;
  if ((long long)d * n > 32767) return -1;
  if (vars ? false : num_vars != p->num_vars) return -1;
  if (ptr[0] != 0) return -1;
  for (int v = 0; v <= num_vars; v++)
    if (ptr[v + 1] < ptr[v]) return -1;
  const int nz = ptr[num_vars + 1];
  if (nz > 0 && (!row || !col || !val)) return -1;
  for (int e = 0; e < nz; e++) {
    if (col[e] < 0 || row[e] < col[e] || row[e] >= n) return -1;
    for (int pl = 0; pl < d; pl++)
      if (!std::isfinite(val[(size_t)d * e + pl]) || (pl > 0 && row[e] == col[e] && val[(size_t)d * e + pl] != 0.0)) return -1;
  }
  Cone k;
  k.kind = kLmi;
  k.order = n;
  k.hyper = d;
  k.hermitian = true;
  k.from_entries = true;
  k.e_ptr.assign(ptr, ptr + num_vars + 2);
  k.e_row.assign(row, row + nz);
  k.e_col.assign(col, col + nz);
  k.e_val.assign(val, val + (size_t)d * nz);
  if (vars) {
    for (int i = 0; i < num_vars; i++) {
      if (vars[i] < 0 || vars[i] >= p->num_vars) return -1;
      k.vars.push_back((int)vars[i]);
    }
  } else {
    k.vars = AllVars(*p);
  }
  return AddCone(p, std::move(k));
}

/* not part of conex.h: a HermitianPsdConstraint over R / C / H (d = 1, 2, 4) whose matrices are low-rank and given by
 * their factors,  A_v = sum_k sigma[k] f_k f_k^*,  k = rank_ptr[v] .. rank_ptr[v + 1] - 1,  v < num_vars,
 * f_k the hyper-complex columns of F (d planes of n x R column-major, R = rank_ptr[num_vars]); sigma NULL = all +1; c
 * the affine term, d planes of n x n (plane 0 symmetric, the others skew); vars as above.  The matrices are never
 * formed (cxk_add_hermitian_factored).  CONEX_UpdateLinearOperator and CONEX_UpdateAffineTerm fail on such a
 * constraint; CONEX_GetDualVariable gives the real plane, as for every Hermitian constraint.
 * Returns the constraint id, -1 on invalid arguments. */
int CONEX_HIP_AddFactoredHermitianConstraint(void* x, int n, int d, const double* F, int R, const double* sigma,
                                             const int* rank_ptr, int num_vars, const double* c, const long* vars) {
  Program* p = static_cast<Program*>(x);
  if (!p || p->magic != 0xC0DEC0DEu || n < 1 || R < 0 || num_vars < 0 || !rank_ptr || !c || (R > 0 && !F)) return -1;
  if (d != 1 && d != 2 && d != 4) return -1;
  if (vars ? false : num_vars != p->num_vars) return -1;
  if (rank_ptr[0] != 0 || rank_ptr[num_vars] != R) return -1;
  for (int v = 0; v < num_vars; v++)
    if (rank_ptr[v + 1] < rank_ptr[v]) return -1;
  const size_t nn = (size_t)n * n, nr = (size_t)n * R;
  for (size_t q = 0; q < d * nr; q++)
    if (!std::isfinite(F[q])) return -1;
  for (int k = 0; sigma && k < R; k++)
    if (!std::isfinite(sigma[k])) return -1;
  for (int pl = 0; pl < d; pl++)
    for (int col = 0; col < n; col++)
      for (int row = col; row < n; row++) {
        const double lo = c[pl * nn + row + (size_t)col * n], up = c[pl * nn + col + (size_t)row * n];
        if (!std::isfinite(lo) || (pl == 0 ? lo != up : lo != -up)) return -1;
      }
  Cone k;
  k.kind = kLmi;
  k.order = n;
  k.hyper = d;
  k.hermitian = true;
  k.factored = true;
  k.F.assign(F, F + d * nr);
  if (sigma)
    k.sigma.assign(sigma, sigma + R);
  else
    k.sigma.assign((size_t)R, 1.0);
  k.rank_ptr.assign(rank_ptr, rank_ptr + num_vars + 1);
  k.affine.assign(c, c + d * nn);
  if (vars) {
    for (int i = 0; i < num_vars; i++) {
      if (vars[i] < 0 || vars[i] >= p->num_vars) return -1;
      k.vars.push_back((int)vars[i]);
    }
  } else {
    k.vars = AllVars(*p);
  }
  return AddCone(p, std::move(k));
}

int CONEX_HIP_AddQuadraticCostEpigraph(void* x, const double* Qi, int nz, const long* z, long epigraph) {
  if (!Qi || !z || nz < 1) return -1;
  // inner-product matrix Q = diag(1, Qi); (A, b) with b - A (z, t) in L  <=>  t >= 1/2 z' Qi z:
  //   (.5 t + 1)^2 >= (.5 t - 1)^2 + z' Qi z
  const int n = nz + 1, len = nz + 2, cols = nz + 1;
  std::vector<double> Q((size_t)n * n, 0.0), A((size_t)len * cols, 0.0), b((size_t)len, 0.0);
  Q[0] = 1;
  for (int j = 0; j < nz; j++)
    for (int i = 0; i < nz; i++) Q[(size_t)(j + 1) * n + (i + 1)] = Qi[(size_t)j * nz + i];
  A[(size_t)nz * len + 0] = -0.5;  // topRightCorner(2, 1) << -.5, -.5
  A[(size_t)nz * len + 1] = -0.5;
  for (int j = 0; j < nz; j++) A[(size_t)j * len + 2 + j] = 1;  // bottomLeftCorner = I
  b[0] = 1;
  b[1] = -1;
  std::vector<long> vars(z, z + nz);
  vars.push_back(epigraph);
  return CONEX_HIP_AddQuadraticConstraint(x, Q.data(), n, A.data(), len, cols, b.data(), len, vars.data(), cols);
}

/* not part of conex.h: lets a host pick the HIP device ordinal before the first solve */
int CONEX_HIP_SetDevice(void* x, int device) {
  Program* p = static_cast<Program*>(x);
  if (!p) return CONEX_FAILURE;
  p->device = device;
  p->dirty = true;
  return CONEX_SUCCESS;
}

/* not part of conex.h: device microseconds per phase {Assemble, Factor, Solve, Update, other}
 * accumulated by the solves of this program while CONEX_ENABLE_TIMER=1 */
int CONEX_HIP_GetPhaseTimes(void* x, double* us5) {
  Program* p = static_cast<Program*>(x);
  if (!p || !p->ctx || !us5) return CONEX_FAILURE;
  return cxk_phase_read(p->ctx, us5, 0) == CXK_SUCCESS ? CONEX_SUCCESS : CONEX_FAILURE;
}

/* not part of conex.h (bench.py's `newton_step`): hipEvent clocks on the kernels of the program's
 * device context (cxk_enable_timing / cxk_kernel_clock); the context must exist (after a first solve) */
int CONEX_HIP_KernelClocks(void* x, int period) {
  Program* p = static_cast<Program*>(x);
  if (!p || !p->ctx) return CONEX_FAILURE;
  return cxk_enable_timing(p->ctx, period) == CXK_SUCCESS ? CONEX_SUCCESS : CONEX_FAILURE;
}
/* avg_ms[CXK_CLOCK_COUNT], samples[CXK_CLOCK_COUNT] since the last call (the slots are reset) */
int CONEX_HIP_ReadKernelClocks(void* x, double* avg_ms, int* samples) {
  Program* p = static_cast<Program*>(x);
  if (!p || !p->ctx || !avg_ms || !samples) return CONEX_FAILURE;
  if (cxk_sync(p->ctx, nullptr) != CXK_SUCCESS) return CONEX_FAILURE;  // folds the finished event pairs
  for (int k = 0; k < CXK_CLOCK_COUNT; k++) samples[k] = cxk_kernel_clock(p->ctx, k, 1, &avg_ms[k]);
  return CONEX_SUCCESS;
}

/* not part of conex.h, test hook: cxk_debug_fused_timeout_at on the context the next solve builds (the
 * launch_index-th whole-tree factor launch of that solve reports a wait that ran out behind its launch `which`) */
int CONEX_HIP_DebugFusedTimeoutAt(void* x, int launch_index, int which) {
  Program* p = static_cast<Program*>(x);
  if (!p) return CONEX_FAILURE;
  p->debug_timeout_at = launch_index;
  p->debug_timeout_site = which;
  p->dirty = true;
  return CONEX_SUCCESS;
}

/* not part of conex.h: 1 (the default) = the reference as written, 0 = with the two corrections of
 * conex_kkt_hip.h (cxk_set_reference_identity); unset: CXK_REFERENCE_QUIRKS in the environment */
int CONEX_HIP_SetReferenceIdentity(void* x, int on) {
  Program* p = static_cast<Program*>(x);
  if (!p) return CONEX_FAILURE;
  p->reference_identity = on != 0;
  p->dirty = true;
  return CONEX_SUCCESS;
}

/* not part of conex.h: 1 (the default) = a second-order cone larger than LDS is held in HBM and runs on the
 * streamed kernels (conex_kkt_hip.h, cxk_set_streamed_cones); 0 = such a cone is refused when the program is
 * initialized, as the cxk_* interface does by default */
int CONEX_HIP_SetStreamedCones(void* x, int on) {
  Program* p = static_cast<Program*>(x);
  if (!p) return CONEX_FAILURE;
  p->streamed_cones = on != 0;
  p->dirty = true;
  return CONEX_SUCCESS;
}

/* not part of conex.h: which linear-inequality blocks run on the tiled kernels (conex_kkt_hip.h,
 * cxk_set_tiled_linear): -1 (the default) by size, 0 none, 1 every block */
int CONEX_HIP_SetTiledLinear(void* x, int mode) {
  Program* p = static_cast<Program*>(x);
  if (!p || mode < -1 || mode > 1) return CONEX_FAILURE;
  p->tiled_linear = mode;
  p->dirty = true;
  return CONEX_SUCCESS;
}

/* not part of conex.h: which linear-inequality blocks are evaluated from their nonzeros (conex_kkt_hip.h,
 * cxk_set_sparse_linear): -1 (the default) those whose pattern makes it pay, unless CONEX_HIP_SetTiledLinear made an
 * explicit choice; 0 none; 1 every block */
int CONEX_HIP_SetSparseLinear(void* x, int mode) {
  Program* p = static_cast<Program*>(x);
  if (!p || mode < -1 || mode > 1) return CONEX_FAILURE;
  p->sparse_linear = mode;
  p->dirty = true;
  return CONEX_SUCCESS;
}

/* not part of conex.h: which second-order cones are evaluated from their nonzeros (conex_kkt_hip.h,
 * cxk_set_sparse_soc): 0 (the default) none; 1 every cone; -1 those that can run nowhere else or whose pattern makes
 * it pay */
int CONEX_HIP_SetSparseSoc(void* x, int mode) {
  Program* p = static_cast<Program*>(x);
  if (!p || mode < -1 || mode > 1) return CONEX_FAILURE;
  p->sparse_soc = mode;
  p->dirty = true;
  return CONEX_SUCCESS;
}
/* second-order cones of the program's device context on the sparse route (cxk_count_sparse_soc); -1 before a first solve */
int CONEX_HIP_CountSparseSoc(void* x) {
  Program* p = static_cast<Program*>(x);
  return p && p->ctx ? cxk_count_sparse_soc(p->ctx) : -1;
}

/* not part of conex.h: how sparse matrix inequalities of order 64 and up evaluate an affine term of more than 64
 * nonzeros (conex_kkt_hip.h, cxk_set_sparse_affine): 1 from its nonzeros, 0 by two n^3 GEMMs, -1 from its nonzeros when
 * that pays.  Without a call a constraint added by CONEX_HIP_AddLMIConstraintFromEntries takes -1 and every other one 0. */
int CONEX_HIP_SetSparseAffine(void* x, int mode) {
  Program* p = static_cast<Program*>(x);
  if (!p || mode < -1 || mode > 1) return CONEX_FAILURE;
  p->sparse_affine = mode;
  p->dirty = true;
  return CONEX_SUCCESS;
}
/* matrix inequalities of the program's device context on those kernels (cxk_count_sparse_affine); -1 before a first solve */
int CONEX_HIP_CountSparseAffine(void* x) {
  Program* p = static_cast<Program*>(x);
  return p && p->ctx ? cxk_count_sparse_affine(p->ctx) : -1;
}

/* not part of conex.h: whether sparse Hermitian matrix inequalities over C or H sum over the top block row of their
 * real representations (conex_kkt_hip.h, cxk_set_sparse_fold): 1 every one, 0 none.  Without a call a constraint added
 * by CONEX_HIP_AddHermitianConstraintFromEntries folds and every other one does not. */
int CONEX_HIP_SetSparseFold(void* x, int mode) {
  Program* p = static_cast<Program*>(x);
  if (!p || (mode != 0 && mode != 1)) return CONEX_FAILURE;
  p->sparse_fold = mode;
  p->dirty = true;
  return CONEX_SUCCESS;
}
/* matrix inequalities of the program's device context on the folded kernels (cxk_count_sparse_fold); -1 before a first solve */
int CONEX_HIP_CountSparseFold(void* x) {
  Program* p = static_cast<Program*>(x);
  return p && p->ctx ? cxk_count_sparse_fold(p->ctx) : -1;
}

/* not part of conex.h: which quadratic cones are held in HBM and run on the streamed kernels (conex_kkt_hip.h,
 * cxk_set_streamed_quadratic): -1 (the default) those beyond LDS and those large enough to be faster there, 0 none
 * (a cone beyond LDS is then refused when the program is initialized), 1 every cone */
int CONEX_HIP_SetStreamedQuadratic(void* x, int mode) {
  Program* p = static_cast<Program*>(x);
  if (!p || mode < -1 || mode > 1) return CONEX_FAILURE;
  p->streamed_quadratic = mode;
  p->dirty = true;
  return CONEX_SUCCESS;
}

/* Multi-GPU, not part of conex.h (the reference is single process).  One process per GPU; every
 * rank builds the SAME program and calls CONEX_Maximize / CONEX_Solve with the same arguments;
 * constraints are dealt to the ranks by elimination subtree, the Schur sums that cross ranks go
 * through one RCCL all-reduce per factorization / solve, the step scalars through small ones
 * (conex_kkt_hip.h, "Collectives").  Every rank returns the same y; a dual variable
 * (CONEX_GetDualVariable) is current on the rank that owns its constraint.
 *   CONEX_HIP_GetUniqueId      128 bytes (ncclGetUniqueId) made by one rank, shipped to all
 *   CONEX_HIP_SetCommunicator  rank / world and the unique id: RCCL over xGMI
 *   CONEX_HIP_SetAllReduce     rank / world and a caller-supplied all-reduce (other transports, tests) */
int CONEX_HIP_GetUniqueId(void* out128) { return cxk_comm_unique_id(out128) == CXK_SUCCESS ? CONEX_SUCCESS : CONEX_FAILURE; }

int CONEX_HIP_SetCommunicator(void* x, const void* unique_id128, int rank, int world_size) {
  Program* p = static_cast<Program*>(x);
  if (!p || !unique_id128 || world_size < 1 || rank < 0 || rank >= world_size) return CONEX_FAILURE;
  p->shard_rank = rank;
  p->shard_world = world_size;
  memcpy(p->unique_id, unique_id128, 128);
  p->have_unique_id = true;
  p->allreduce_fn = nullptr;
  p->dirty = true;
  return CONEX_SUCCESS;
}

int CONEX_HIP_SetAllReduce(void* x, int rank, int world_size, cxk_allreduce_fn fn, void* user) {
  Program* p = static_cast<Program*>(x);
  if (!p || !fn || world_size < 1 || rank < 0 || rank >= world_size) return CONEX_FAILURE;
  p->shard_rank = rank;
  p->shard_world = world_size;
  p->allreduce_fn = fn;
  p->allreduce_user = user;
  p->dirty = true;
  return CONEX_SUCCESS;
}

}  // extern "C"
