// Which of its four iterations the interior-point loop of program.cc runs, as ONE pure function of
// what the loop knows before it enqueues the factorization.  Plain C++17: no HIP, no I/O, no
// allocation (tests/test_solve_route.py compiles it alone and walks all 128 inputs).
//
//   device mu   the barrier parameter is selected on the device; the host's first round trip of the
//               iteration is PrepareStep's.  With the triple right-hand side the factor sweep carries
//               the three solutions every Newton direction is a combination of; without it the
//               solve of the mu selection rides in the sweep and the direction is a sweep of its own.
//   host mu     selected on the host from the eigenvalue query (its solve rides in the factor sweep)
//   line search selected on the host by the line search, behind a plain factorization
//   kept        mu stays: the Newton direction itself rides in the factor sweep
#pragma once

namespace cxk_route {

struct Inputs {
  bool update_mu;            // this iteration selects a new barrier parameter
  bool line_search;          // SolverConfiguration::enable_line_search
  bool quadratic_costs;      // the program has a quadratic cost
  bool timers;               // CONEX_ENABLE_TIMER: the reference's phases are bracketed on the host
  bool warm_first;           // first iteration of a warm start: the step may yet be refused
  bool device_mu_supported;  // cxk_device_mu_supported(ctx) == 1, asked behind this iteration's assembly
  bool triple_supported;     // cxk_triple_supported(ctx) == 1, likewise
};

enum class Factor {
  kTriple,     // cxk_factor_solve_triple_async
  kSolve,      // cxk_factor_solve_async(-bs, cs, 0): the right-hand side of the mu selection
  kDirection,  // cxk_factor_direction_async
  kPlain       // cxk_factor_async
};
enum class Mu { kDevice, kHost, kKept };
enum class Direction {
  kDeviceMu,  // cxk_newton_direction_device_mu
  kNone,      // came with the factorization
  kHost       // cxk_newton_direction
};
enum class Step {
  kPrepareTakeDeviceMu,  // cxk_prepare_take_step_device_mu
  kPrepareTake,          // cxk_prepare_take_step
  kPrepare               // cxk_prepare_step, cxk_take_step from the host afterwards
};
// The factorization's outcome is read behind the first host round trip of the iteration.
enum class OutcomeRead { kAfterMuSelection, kAfterPrepare };

struct Route {
  bool mu_on_device;
  Factor factor;
  Mu mu;
  bool mu_solve_done;  // host selection: its solve came with the factorization
  Direction direction;
  Step step;
  OutcomeRead outcome_read;
};

constexpr Route Choose(const Inputs& in) {
  // Not with a line search or quadratic costs (the line search is the host's), not under the phase
  // timers (they bracket the host route's separate calls), not while a warm start may still be
  // aborted (the host has to see the step's norm before the step is taken).
  const bool mu_on_device = in.update_mu && !in.line_search && !in.quadratic_costs && !in.timers &&
                            !in.warm_first && in.device_mu_supported;
  Route r{};
  r.mu_on_device = mu_on_device;
  r.mu_solve_done = in.update_mu && !in.line_search;
  r.factor = mu_on_device && in.triple_supported ? Factor::kTriple
             : r.mu_solve_done                   ? Factor::kSolve
             : !in.update_mu                     ? Factor::kDirection
                                                 : Factor::kPlain;
  r.mu = mu_on_device ? Mu::kDevice : in.update_mu ? Mu::kHost : Mu::kKept;
  r.direction = mu_on_device ? Direction::kDeviceMu : !in.update_mu ? Direction::kNone : Direction::kHost;
  // TakeStep rides behind PrepareStep when the factorization's outcome is known by then (it came
  // back with the host's mu selection) or is looked at on the device (device mu).
  r.step = mu_on_device                      ? Step::kPrepareTakeDeviceMu
           : in.update_mu && !in.warm_first  ? Step::kPrepareTake
                                             : Step::kPrepare;
  r.outcome_read = r.mu == Mu::kHost ? OutcomeRead::kAfterMuSelection : OutcomeRead::kAfterPrepare;
  return r;
}

}  // namespace cxk_route
